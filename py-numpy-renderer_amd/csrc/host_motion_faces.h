// host_motion_faces.h -- the velocity of models that bend (motion_faces_def.h has the definition): the snapshot of the
// previous frame's vertices and its serial, the scene's description, the launch of k_face_homography and k_velocity_faces
// between a frame's k_velocity and k_mblur, the same arithmetic on the host, bit for bit (host_face_homographies,
// host_velocity_faces: plain C++, no device), and mr_debug_motion_faces_post, the two kernels on arrays a caller supplies.
//
// The library is stateless about cameras and poses, but deformed vertices live on the device only, so it holds ONE
// snapshot: while tracking is on (mr_scene_track_vertices), a pose pass that is about to rewrite d_verts first copies all
// of it to d_verts_prev, behind the pass's wait for the device, and notes the vertex serial of what it copied.  The serial
// counts the states d_verts has held: every commit that uploads vertices and every pass that rewrites them adds one.  A
// frame's description names the serial its caller saw when the previous frame was issued (prev_serial); the per-face pass
// runs only if the snapshot holds exactly that state, else the frame keeps k_velocity's U and the skip is counted.
#pragma once

namespace {

inline int motion_faces_linked()
{
    return linked("this library was linked without motion_faces.hip: no per-face velocity (build it with __graft_entry__.build())",
                  &mr_motion_faces::launch_homography, &mr_motion_faces::launch_velocity_faces);
}

inline bool motion_faces_finite(const double *s_now, const double *s_prev)
{
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(s_now[i]) || !std::isfinite(s_prev[i])) return false;
    return true;
}

// The int32 tables of the two kernels for these flags: hom_off and face_off of every model, then the first record and
// the first face of every range (a flagged model).  n_faces closes the last model.  False: the models' first faces do not
// ascend from 0 to n_faces.
bool motion_faces_tables(const int32_t *deforming, const int32_t *face_off, int32_t n_models, int64_t n_faces, std::vector<int32_t> &tables,
                         int32_t &n_ranges, int32_t &n_records)
{
    tables.assign((size_t)n_models * 2, -1);
    std::vector<int32_t> rec0, face0;
    int64_t records = 0;
    for (int32_t m = 0; m < n_models; ++m) {
        const int64_t first = face_off[m], end = m + 1 < n_models ? (int64_t)face_off[m + 1] : n_faces;
        if (first < 0 || end < first || (m == 0 && first != 0) || end > n_faces) return false;
        tables[(size_t)n_models + m] = (int32_t)first;
        if (!deforming[m] || end == first) continue;
        tables[m] = (int32_t)records;
        rec0.push_back((int32_t)records); face0.push_back((int32_t)first);
        records += end - first;
    }
    if (records > INT32_MAX) return false;
    n_ranges = (int32_t)rec0.size(); n_records = (int32_t)records;
    tables.insert(tables.end(), rec0.begin(), rec0.end());
    tables.insert(tables.end(), face0.begin(), face0.end());
    return true;
}

// every vertex index of the faces lies inside the vertex array
bool motion_faces_indices_ok(const int32_t *faces, int64_t n_faces, int64_t n_verts)
{
    for (int64_t f = 0; f < n_faces; ++f)
        for (int k = 0; k < 3; ++k) {
            const int32_t v = faces[f * 12 + k * 4];
            if (v < 0 || v >= n_verts) return false;
        }
    return true;
}

// H of every face, on the host
int host_face_homographies(const double *verts_now, const double *verts_prev, int32_t n_verts, const int32_t *faces, int32_t n_faces,
                           const double *s_now, const double *s_prev, double *out_h)
{
    if (!verts_now || !verts_prev || !faces || !s_now || !s_prev || !out_h) return fail(MR_E_INVALID, "mr_host_face_homographies: NULL argument");
    if (n_verts < 0 || n_faces < 0) return fail(MR_E_INVALID, "mr_host_face_homographies: a negative count");
    if (!motion_faces_finite(s_now, s_prev)) return fail(MR_E_INVALID, "per-face velocity: an entry of s_now or s_prev is not finite");
    if (!motion_faces_indices_ok(faces, n_faces, n_verts)) return fail(MR_E_INVALID, "per-face velocity: a vertex index lies outside the vertex array");
    for (int32_t f = 0; f < n_faces; ++f) {
        const int32_t *c = faces + (size_t)f * 12;
        const size_t a = (size_t)c[0] * 4, b = (size_t)c[4] * 4, d = (size_t)c[8] * 4;
        mr::motion_face_homography(verts_now + a, verts_now + b, verts_now + d, verts_prev + a, verts_prev + b, verts_prev + d, s_now, s_prev,
                                   out_h + (size_t)f * mr::MOTION_H);
    }
    return MR_OK;
}

// what both the mirror and the debug entry refuse of a winner map: a flagged model's face without a record
int motion_faces_check_map(const int32_t *winner, const int32_t *face_off, const int32_t *hom_off, int32_t n_models, int32_t n_records,
                           int32_t height, int32_t width)
{
    if (n_models < 1) return fail(MR_E_INVALID, "per-face velocity: at least one model");
    for (int32_t m = 0; m < n_models; ++m)
        if (face_off[m] < 0 || (m > 0 && face_off[m] < face_off[m - 1]) || (m == 0 && face_off[0] != 0))
            return fail(MR_E_INVALID, "per-face velocity: the models' first faces must ascend from 0");
    const size_t n = (size_t)height * width;
    for (size_t i = 0; i < n; ++i) {
        if (winner[i] < 0) continue;
        const int m = mr::motion_model_of(face_off, n_models, winner[i]);
        if (hom_off[m] < 0) continue;
        if ((int64_t)hom_off[m] + (winner[i] - face_off[m]) >= n_records)
            return fail(MR_E_INVALID, "per-face velocity: a winner of a flagged model has no record");
    }
    return MR_OK;
}

// k_velocity_faces on the host: U of the flagged models' samples overwritten, every other float left as it was
int host_velocity_faces(const int32_t *winner, const int32_t *face_off, const int32_t *hom_off, int32_t n_models, const double *h,
                        int32_t n_records, int32_t height, int32_t width, float *velocity)
{
    if (!winner || !face_off || !hom_off || !h || !velocity) return fail(MR_E_INVALID, "mr_host_velocity_faces: NULL argument");
    if (!frame_size_ok(height, width)) return fail(MR_E_INVALID, "mr_host_velocity_faces: resolution out of range");
    if (n_records < 0) return fail(MR_E_INVALID, "mr_host_velocity_faces: a negative count");
    if (int rc = motion_faces_check_map(winner, face_off, hom_off, n_models, n_records, height, width)) return rc;
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t i = (size_t)y * width + x;
            if (winner[i] < 0) continue;
            const int m = mr::motion_model_of(face_off, n_models, winner[i]);
            if (hom_off[m] < 0) continue;
            mr::motion_faces_velocity(h + (size_t)(hom_off[m] + (winner[i] - face_off[m])) * mr::MOTION_H, x, y, velocity[i * 2], velocity[i * 2 + 1]);
        }
    return MR_OK;
}

// What a frame slot owns for the pass: the staged tables and the records.
struct MotionFacesSlot {
    StagedTable tables;
    DevBuf d_hom;
    void release() { tables.release(); d_hom.release(); }
};

void motion_faces_release(mr_scene *sc)
{
    sc->d_verts_prev.release();
    release_pass(sc->mfaces);
}

// In a pose pass that is about to rewrite d_verts, behind its wait for the device: the snapshot, while tracking is on.
int snapshot_vertices(mr_scene *sc)
{
    if (!sc->track_verts) return MR_OK;
    const size_t bytes = sc->verts.size() * sizeof(double);
    HIP_TRY(sc->d_verts_prev.ensure(std::max<size_t>(bytes, 16)));
    if (bytes) HIP_TRY(hipMemcpyAsync(sc->d_verts_prev.p, sc->d_verts.p, bytes, hipMemcpyDeviceToDevice, g_stream));
    sc->snap_valid = true;
    sc->snap_serial = sc->vert_serial;
    sc->snap_verts = (int64_t)(sc->verts.size() / 4);
    sc->mfaces.snapshots += 1;
    return MR_OK;
}

// Whether this frame runs the pass: a flagged model that has faces, and the snapshot of exactly the state the description
// names.  Counts the skip otherwise.  (No flagged face: neither run nor skipped -- the frame enqueues what it did.)
bool motion_faces_due(mr_scene *sc)
{
    mr_scene::MotionFaces &a = sc->mfaces;
    if (!a.on || !sc->motion.on || a.deforming.size() != sc->model_face_off.size()) return false;
    bool any = false;
    const int32_t n_faces = (int32_t)(sc->faces.size() / 12);
    for (size_t m = 0; m < a.deforming.size(); ++m) {
        const int32_t end = m + 1 < a.deforming.size() ? sc->model_face_off[m + 1] : n_faces;
        any = any || (a.deforming[m] && end > sc->model_face_off[m]);
    }
    if (!any) return false;
    if (sc->snap_valid && sc->snap_serial == a.prev_serial && sc->snap_verts == (int64_t)(sc->verts.size() / 4)) return true;
    a.skipped += 1;
    return false;
}

// The two kernels on the frame's stream, between k_velocity and k_mblur, marked for mr_debug_motion_faces_times.
int launch_motion_faces(mr_scene *sc, hipStream_t stream, MotionFacesSlot &ms, const int32_t *winner, float *vel, int width, int height)
{
    mr_scene::MotionFaces &a = sc->mfaces;
    const int32_t n_models = (int32_t)sc->model_face_off.size();
    std::vector<int32_t> tables;
    mr::MotionFacesParams p;
    std::memcpy(p.s_now, a.s_now, sizeof p.s_now); std::memcpy(p.s_prev, a.s_prev, sizeof p.s_prev);
    p.n_models = n_models;
    if (!motion_faces_tables(a.deforming.data(), sc->model_face_off.data(), n_models, (int64_t)(sc->faces.size() / 12), tables, p.n_ranges, p.n_records))
        return fail(MR_E_INVALID, "per-face velocity: the models' first faces do not ascend");
    if (p.n_records == 0) return fail(MR_E_INVALID, "per-face velocity: no flagged face (motion_faces_due answers that)");
    if (int rc = a.marks.create()) return rc;
    HIP_TRY(ms.d_hom.ensure((size_t)p.n_records * mr::MOTION_H * sizeof(double)));
    if (int rc = ms.tables.stage(tables.data(), tables.size() * sizeof(int32_t), stream)) return rc;
    const int32_t *d_tables = ms.tables.d_tables.as<int32_t>();
    if (int rc = a.marks.record(0, stream)) return rc;
    mr_motion_faces::launch_homography(stream, sc->d_faces.as<int32_t>(), sc->d_verts.as<double>(), sc->d_verts_prev.as<double>(), d_tables,
                                       ms.d_hom.as<double>(), p);
    if (int rc = a.marks.record(1, stream)) return rc;
    mr_motion_faces::launch_velocity_faces(stream, winner, d_tables, ms.d_hom.as<double>(), vel, width, height, n_models);
    if (int rc = a.marks.record(2, stream)) return rc;
    a.marked = true;
    a.ran += 1; a.records = p.n_records;
    return MR_OK;
}

constexpr size_t MOTION_FACES_GUARD = 256;               // bytes of sentinel in front of and behind each output buffer
constexpr unsigned char MOTION_FACES_SENTINEL = 0xa5;

// mr_debug_motion_faces_post: both kernels on the caller's arrays through the library's own launches.  The two output
// buffers lie between guards of sentinel bytes on the device; out_guard receives the number of guard bytes that changed.
// Every refusal comes before any device call; the scene lends its error text only.
int debug_motion_faces_post(mr_scene *sc, const double *verts_now, const double *verts_prev, int32_t n_verts, const int32_t *faces,
                            int32_t n_faces, const int32_t *face_off, const int32_t *deforming, int32_t n_models, const double *s_now,
                            const double *s_prev, const int32_t *winner, int32_t height, int32_t width, float *velocity, double *out_h,
                            int32_t *out_guard)
{
    if (!sc || !verts_now || !verts_prev || !faces || !face_off || !deforming || !s_now || !s_prev || !winner || !velocity || !out_h || !out_guard)
        return fail(MR_E_INVALID, "mr_debug_motion_faces_post: NULL argument");
    if (!frame_size_ok(height, width)) return fail(MR_E_INVALID, "mr_debug_motion_faces_post: resolution out of range");
    if (n_verts < 0 || n_faces < 0 || n_models < 1) return fail(MR_E_INVALID, "mr_debug_motion_faces_post: a count out of range");
    if (!motion_faces_finite(s_now, s_prev)) return fail(MR_E_INVALID, "per-face velocity: an entry of s_now or s_prev is not finite");
    if (!motion_faces_indices_ok(faces, n_faces, n_verts)) return fail(MR_E_INVALID, "per-face velocity: a vertex index lies outside the vertex array");
    std::vector<int32_t> tables;
    mr::MotionFacesParams p;
    std::memcpy(p.s_now, s_now, sizeof p.s_now); std::memcpy(p.s_prev, s_prev, sizeof p.s_prev);
    p.n_models = n_models;
    if (!motion_faces_tables(deforming, face_off, n_models, n_faces, tables, p.n_ranges, p.n_records))
        return fail(MR_E_INVALID, "per-face velocity: the models' first faces must ascend from 0 to the number of faces");
    if (int rc = motion_faces_check_map(winner, face_off, tables.data(), n_models, p.n_records, height, width)) return rc;
    if (int rc = motion_faces_linked()) return rc;
    if (int rc = ensure_init()) return rc;
    const size_t n = (size_t)height * width, G = MOTION_FACES_GUARD;
    const size_t hom_bytes = (size_t)p.n_records * mr::MOTION_H * sizeof(double), vel_bytes = n * 2 * sizeof(float);
    const std::vector<int32_t> fv(faces, faces + (size_t)n_faces * 12), wv(winner, winner + n);
    const std::vector<double> vn(verts_now, verts_now + (size_t)n_verts * 4), vp(verts_prev, verts_prev + (size_t)n_verts * 4);
    std::vector<unsigned char> guards(4 * G);
    struct { DevBuf faces, verts, prev, tables, winner, hom, vel; } buf;
    Drained drained{ &buf.faces, &buf.verts, &buf.prev, &buf.tables, &buf.winner, &buf.hom, &buf.vel };      // (behind the vectors: it drains the stream before they go)
    if (int rc = upload(buf.faces, fv, g_stream)) return rc;
    if (int rc = upload(buf.verts, vn, g_stream)) return rc;
    if (int rc = upload(buf.prev, vp, g_stream)) return rc;
    if (int rc = upload(buf.tables, tables, g_stream)) return rc;
    if (int rc = upload(buf.winner, wv, g_stream)) return rc;
    HIP_TRY(buf.hom.ensure(hom_bytes + 2 * G));
    HIP_TRY(buf.vel.ensure(vel_bytes + 2 * G));
    HIP_TRY(hipMemsetAsync(buf.hom.p, MOTION_FACES_SENTINEL, hom_bytes + 2 * G, g_stream));
    HIP_TRY(hipMemsetAsync(buf.vel.p, MOTION_FACES_SENTINEL, vel_bytes + 2 * G, g_stream));
    HIP_TRY(hipMemcpyAsync(buf.vel.as<char>() + G, velocity, vel_bytes, hipMemcpyHostToDevice, g_stream));
    mr_motion_faces::launch_homography(g_stream, buf.faces.as<int32_t>(), buf.verts.as<double>(), buf.prev.as<double>(), buf.tables.as<int32_t>(),
                                       reinterpret_cast<double *>(buf.hom.as<char>() + G), p);
    mr_motion_faces::launch_velocity_faces(g_stream, buf.winner.as<int32_t>(), buf.tables.as<int32_t>(),
                                           reinterpret_cast<const double *>(buf.hom.as<char>() + G), reinterpret_cast<float *>(buf.vel.as<char>() + G),
                                           width, height, n_models);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(guards.data(), buf.hom.p, G, hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipMemcpyAsync(guards.data() + G, buf.hom.as<char>() + G + hom_bytes, G, hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipMemcpyAsync(guards.data() + 2 * G, buf.vel.p, G, hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipMemcpyAsync(guards.data() + 3 * G, buf.vel.as<char>() + G + vel_bytes, G, hipMemcpyDeviceToHost, g_stream));
    if (hom_bytes) HIP_TRY(hipMemcpyAsync(out_h, buf.hom.as<char>() + G, hom_bytes, hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipMemcpyAsync(velocity, buf.vel.as<char>() + G, vel_bytes, hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    int32_t touched = 0;
    for (unsigned char g : guards) touched += g != MOTION_FACES_SENTINEL;
    *out_guard = touched;
    return MR_OK;
}

}  // namespace
