// host_motion.h -- motion blur from a per-sample velocity buffer (motion_def.h has the definition): the scene's description
// as the kernels take it, the launch of k_velocity and k_mblur behind a frame's tile kernel (and behind k_ao and k_dof where
// they run), the same arithmetic on the host, bit for bit (host_velocity, host_motion_blur: plain C++, no device), and
// mr_debug_motion_post, the two kernels on buffers a caller supplies.  The library is stateless about time: it is handed
// the matrices that lead from this frame's samples to the previous frame's, as it is handed kf and focus.  The bytes of such
// a frame are the full resolve of its float frame, like a blurred or darkened frame's (host_frame.h, launch_post_resolve).
#pragma once

namespace {

struct MotionFacesSlot;                      // host_motion_faces.h: the per-face velocity of models that bend
bool motion_faces_due(mr_scene *sc);
int launch_motion_faces(mr_scene *sc, hipStream_t stream, MotionFacesSlot &ms, const int32_t *winner, float *vel, int width, int height);

// the two kernels are motion.hip's; the bytes of a blurred frame are the accumulation's resolve of its float frame (accum.hip)
inline int motion_linked()
{
    return linked("this library was linked without motion.hip or accum.hip: no motion blur (build it with __graft_entry__.build())",
                  &mr_motion::launch_velocity, &mr_motion::launch_blur, &mr_accum::launch_resolve);
}

// The description as the kernels and the mirrors take it, checked: the scalars, and the tables as one block -- the class
// matrices, the background's, then (int32) the models' first faces and their classes.
int motion_params(const mr_motion_desc *d, const int32_t *face_off, mr::MotionParams &p, std::vector<double> &tables)
{
    if (int rc = take_depth_map("motion blur", d->depth_map, p.m)) return rc;
    p.shutter = (float)d->shutter;
    if (!(std::isfinite(p.shutter) && p.shutter > 0.0f && p.shutter <= 1.0f))
        return fail(MR_E_INVALID, "motion blur: shutter must lie in (0, 1] as float32");
    if (d->n_classes < 1 || d->n_classes > (1 << 20) || !d->matrices) return fail(MR_E_INVALID, "motion blur: at least one class matrix (class 0, the camera's)");
    if (d->n_models < 0 || (d->n_models > 0 && (!d->class_of_model || !face_off))) return fail(MR_E_INVALID, "motion blur: class_of_model is NULL");
    const size_t n_t = (size_t)d->n_classes * mr::MOTION_T;
    for (size_t i = 0; i < n_t; ++i)
        if (!std::isfinite(d->matrices[i])) return fail(MR_E_INVALID, "motion blur: a matrix entry is not finite");
    for (int i = 0; i < mr::MOTION_B; ++i)
        if (!std::isfinite(d->background[i])) return fail(MR_E_INVALID, "motion blur: a matrix entry is not finite");
    for (int32_t m = 0; m < d->n_models; ++m) {
        if (d->class_of_model[m] < 0 || d->class_of_model[m] >= d->n_classes) return fail(MR_E_INVALID, "motion blur: a model's class is out of range");
        if (face_off[m] < 0 || (m > 0 && face_off[m] < face_off[m - 1]) || (m == 0 && face_off[0] != 0))
            return fail(MR_E_INVALID, "motion blur: the models' first faces must ascend from 0");
    }
    p.n_classes = d->n_classes; p.n_models = d->n_models;
    tables.assign(n_t + mr::MOTION_B + (size_t)d->n_models, 0.0);                    // (2 n_models int32 = n_models doubles)
    std::memcpy(tables.data(), d->matrices, n_t * sizeof(double));
    std::memcpy(tables.data() + n_t, d->background, mr::MOTION_B * sizeof(double));
    int32_t *ints = reinterpret_cast<int32_t *>(tables.data() + n_t + mr::MOTION_B);
    for (int32_t m = 0; m < d->n_models; ++m) { ints[m] = face_off[m]; ints[d->n_models + m] = d->class_of_model[m]; }
    return MR_OK;
}

// What a frame slot owns for the pass: the staged tables and the velocity buffer.
struct MotionSlot {
    StagedTable tables;
    DevBuf d_vel;
    void release() { tables.release(); d_vel.release(); }
};

// What k_velocity needs on the slot before it runs: the velocity buffer, and `tables` (a description's block) staged with
// the models' first faces of this moment.  The motion blur's pass and the temporal anti-aliasing's (host_taa.h) share it.
int stage_velocity(mr_scene *sc, hipStream_t stream, MotionSlot &ms, std::vector<double> &tables, const mr::MotionParams &p, int width, int height)
{
    // (the models' first faces are the scene's of this moment: a commit may have moved them since the description came)
    int32_t *off = reinterpret_cast<int32_t *>(tables.data() + (size_t)p.n_classes * mr::MOTION_T + mr::MOTION_B);
    for (int32_t m = 0; m < p.n_models; ++m) off[m] = sc->model_face_off[m];
    HIP_TRY(ms.d_vel.ensure((size_t)width * height * 2 * sizeof(float)));
    return ms.tables.stage(tables.data(), tables.size() * sizeof(double), stream);
}

// k_velocity and k_mblur from a frame's own z-buffer, winner map and float frame into the slot's velocity buffer and `out`,
// on the frame's stream behind its tile kernel, marked for mr_debug_motion_times.  `p` is the copy the frame's plan took, `shape` k_mblur's (Env::mblur_shape).
// Between the two, where the scene has flagged models and the snapshot they need (motion_faces_due), k_face_homography and
// k_velocity_faces overwrite those models' U; k_mblur's span then starts at a mark of its own.
// With vel_ready the slot's velocity buffer is this frame's already -- the temporal anti-aliasing ran k_velocity, and the
// per-face pair where due, from the same tables in front of k_taa -- and the pass goes straight to k_mblur.
int launch_motion(mr_scene *sc, hipStream_t stream, MotionSlot &ms, MotionFacesSlot &faces, const double *zbuf, const int32_t *winner, const float *frame, float *out,
                  int width, int height, const mr::MotionParams &p, int shape, bool vel_ready = false)
{
    mr_scene::Motion &a = sc->motion;
    if (!vel_ready)
        if (int rc = stage_velocity(sc, stream, ms, a.tables, p, width, height)) return rc;
    float *vel = ms.d_vel.as<float>();
    a.vel_skipped = vel_ready;
    return marked_launch(a, stream, width, height, [&]() -> int {
        if (!vel_ready) mr_motion::launch_velocity(stream, zbuf, winner, ms.tables.d_tables.as<double>(), vel, width, height, p);
        if (int rc = a.marks.record(1, stream)) return rc;
        a.blur_from = 1;
        if (!vel_ready && motion_faces_due(sc)) {
            if (int rc = launch_motion_faces(sc, stream, faces, winner, vel, width, height)) return rc;
            if (int rc = a.marks.record(2, stream)) return rc;
            a.blur_from = 2;
        }
        mr_motion::launch_blur(stream, zbuf, vel, frame, out, width, height, p, shape);
        return MR_OK;
    });
}

// The velocity's definition on the host.
int host_velocity(const double *z, const int32_t *winner, const int32_t *face_off, int32_t height, int32_t width, const mr_motion_desc *d, float *out)
{
    if (!z || !winner || !d || !out) return fail(MR_E_INVALID, "mr_host_velocity: NULL argument");
    if (!frame_size_ok(height, width)) return fail(MR_E_INVALID, "mr_host_velocity: resolution out of range");
    mr::MotionParams p;
    std::vector<double> tables;
    if (int rc = motion_params(d, face_off, p, tables)) return rc;
    const double *B = tables.data() + (size_t)p.n_classes * mr::MOTION_T;
    const int32_t *off = reinterpret_cast<const int32_t *>(B + mr::MOTION_B), *class_of = off + p.n_models;
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t i = (size_t)y * width + x;
            int cls = 0;
            if (winner[i] >= 0 && p.n_models > 0) cls = class_of[mr::motion_model_of(off, p.n_models, winner[i])];
            mr::motion_velocity(tables.data() + (size_t)cls * mr::MOTION_T, B, z[i], x, y, out[i * 2], out[i * 2 + 1]);
        }
    return MR_OK;
}

// The blur's definition on the host.  (Its loops are bounded by the frame's largest h, as the kernel's are by its
// rectangle's: the taps left out fail the test.)
int host_motion_blur(const double *z, const float *vel, const float *frame, int32_t height, int32_t width, const mr_motion_desc *d, float *out)
{
    if (!z || !vel || !frame || !d || !out) return fail(MR_E_INVALID, "mr_host_motion_blur: NULL argument");
    if (frame == out) return fail(MR_E_INVALID, "mr_host_motion_blur: out_frame must not be the frame (neighbours' colours are read)");
    if (!frame_size_ok(height, width)) return fail(MR_E_INVALID, "mr_host_motion_blur: resolution out of range");
    mr_motion_desc scalars = *d;                       // (the blur reads the depth map and the shutter only)
    scalars.n_models = 0; scalars.class_of_model = nullptr;
    mr::MotionParams p;
    std::vector<double> tables;
    if (int rc = motion_params(&scalars, nullptr, p, tables)) return rc;
    const size_t n = (size_t)height * width;
    std::vector<float> e(n), h(n), dx(n), dy(n), inv(n);
    float top = 0.0f;
    for (size_t i = 0; i < n; ++i) {
        e[i] = host_eye_depth(p.m, z[i]);
        mr::motion_segment(p.shutter, vel[i * 2], vel[i * 2 + 1], h[i], dx[i], dy[i], inv[i]);
        top = h[i] > top ? h[i] : top;
    }
    const int bound = mr::motion_bound(top);
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t i = (size_t)y * width + x;
            float W = 0.0f, S[3] = { 0.0f, 0.0f, 0.0f };
            for (int oy = -bound; oy <= bound; ++oy) {
                if (y + oy < 0 || y + oy >= height) continue;
                for (int ox = -bound; ox <= bound; ++ox) {
                    if (x + ox < 0 || x + ox >= width) continue;
                    const size_t q = (size_t)(y + oy) * width + (x + ox);
                    float w;
                    if (!mr::motion_tap(ox, oy, e[i], h[i], inv[i], e[q], h[q], inv[q], dx[q], dy[q], w)) continue;
                    W = W + w;
                    for (int c = 0; c < 3; ++c) S[c] = S[c] + w * frame[q * 3 + c];
                }
            }
            for (int c = 0; c < 3; ++c) out[i * 3 + c] = S[c] / W;
        }
    return MR_OK;
}

// mr_debug_motion_post: the two kernels on the caller's arrays through the library's own launches, the workgroup shape an
// argument and not the environment's.  Every refusal comes before any device call; the scene's slots, its last frame and
// what mr_debug_motion reports stay as they were.
int debug_motion_post(mr_scene *sc, const double *z, const int32_t *winner, const float *frame, const int32_t *face_off, int32_t height,
                      int32_t width, const mr_motion_desc *d, int32_t shape, float *out_velocity, float *out_frame)
{
    if (!sc || !z || !winner || !frame || !d || !out_velocity || !out_frame) return fail(MR_E_INVALID, "mr_debug_motion_post: NULL argument");
    if (!frame_size_ok(height, width)) return fail(MR_E_INVALID, "mr_debug_motion_post: resolution out of range");
    if (shape < 0 || shape > 2) return fail(MR_E_INVALID, "mr_debug_motion_post: the workgroup shape of k_mblur is 0, 1 or 2");
    mr::MotionParams p;
    std::vector<double> tables;
    if (int rc = motion_params(d, face_off, p, tables)) return rc;
    if (int rc = motion_linked()) return rc;
    if (int rc = ensure_init()) return rc;
    const size_t n = (size_t)height * width;
    struct { DevBuf z, winner, tables, vel, a, b; } buf;
    Drained drained{ &buf.z, &buf.winner, &buf.tables, &buf.vel, &buf.a, &buf.b };
    HIP_TRY(buf.z.ensure(n * sizeof(double)));
    HIP_TRY(buf.winner.ensure(n * sizeof(int32_t)));
    HIP_TRY(buf.vel.ensure(n * 2 * sizeof(float)));
    HIP_TRY(buf.a.ensure(n * 3 * sizeof(float)));
    HIP_TRY(buf.b.ensure(n * 3 * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(buf.z.p, z, n * sizeof(double), hipMemcpyHostToDevice, g_stream));
    HIP_TRY(hipMemcpyAsync(buf.winner.p, winner, n * sizeof(int32_t), hipMemcpyHostToDevice, g_stream));
    HIP_TRY(hipMemcpyAsync(buf.a.p, frame, n * 3 * sizeof(float), hipMemcpyHostToDevice, g_stream));
    if (int rc = upload(buf.tables, tables, g_stream)) return rc;
    mr_motion::launch_velocity(g_stream, buf.z.as<double>(), buf.winner.as<int32_t>(), buf.tables.as<double>(), buf.vel.as<float>(), width, height, p);
    mr_motion::launch_blur(g_stream, buf.z.as<double>(), buf.vel.as<float>(), buf.a.as<float>(), buf.b.as<float>(), width, height, p, shape);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_velocity, buf.vel.p, n * 2 * sizeof(float), hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipMemcpyAsync(out_frame, buf.b.p, n * 3 * sizeof(float), hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    return MR_OK;
}

}  // namespace
