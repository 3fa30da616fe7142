// host_motion.h -- motion blur from a per-sample velocity buffer (motion_def.h has the definition): the scene's description
// as the kernels take it, the launch of k_velocity and k_mblur behind a frame's tile kernel (and behind k_ao and k_dof where
// they run), the same arithmetic on the host, bit for bit (host_velocity, host_motion_blur: plain C++, no device), and
// mr_debug_motion_post, the two kernels on buffers a caller supplies.  The library is stateless about time: it is handed
// the matrices that lead from this frame's samples to the previous frame's, as it is handed kf and focus.  The bytes of such
// a frame are the full resolve of its float frame, like a blurred or darkened frame's (host_frame.h, launch_post_resolve).
#pragma once

// the launches of motion.hip, the library's fifth translation unit; weak, so that a library linked without it still loads:
// it refuses the motion blur instead (the resolve, accum.hip's, is declared in host_ao.h)
namespace mr_motion {
__attribute__((weak)) void launch_velocity(hipStream_t stream, const double *zbuf, const int32_t *winner, const double *tables, float *vel,
                                           int width, int height, const mr::MotionParams &p);
__attribute__((weak)) void launch_blur(hipStream_t stream, const double *zbuf, const float *vel, const float *frame, float *out, int width,
                                       int height, const mr::MotionParams &p, int shape);
}  // namespace mr_motion

namespace {

struct MotionFacesSlot;                      // host_motion_faces.h: the per-face velocity of models that bend
bool motion_faces_due(mr_scene *sc);
int launch_motion_faces(mr_scene *sc, hipStream_t stream, MotionFacesSlot &ms, const int32_t *winner, float *vel, int width, int height);

inline int motion_linked()
{
    if (&mr_motion::launch_velocity && &mr_motion::launch_blur && &mr_accum::launch_resolve) return MR_OK;
    return fail(MR_E_UNSUPPORTED, "this library was linked without motion.hip or accum.hip: no motion blur (build it with __graft_entry__.build())");
}

// The description as the kernels and the mirrors take it, checked: the scalars, and the tables as one block -- the class
// matrices, the background's, then (int32) the models' first faces and their classes.
int motion_params(const mr_motion_desc *d, const int32_t *face_off, mr::MotionParams &p, std::vector<double> &tables)
{
    for (int i = 0; i < 4; ++i) {
        if (!std::isfinite(d->depth_map[i])) return fail(MR_E_INVALID, "motion blur: the depth map must be finite");
        p.m[i] = d->depth_map[i];
    }
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

void motion_release(mr_scene::Motion &a)
{
    if (a.ev_ok)
        for (hipEvent_t &e : a.ev) (void)hipEventDestroy(e);
    a = mr_scene::Motion();
}

// workgroup shape of k_mblur (motion.hip, launch_blur): MR_MBLUR_TILE=32x32 | 32x32x256 | 16x16 forces one (host_env.h)
constexpr int MBLUR_DEFAULT_SHAPE = 0;
inline int mblur_shape()
{
    static const int shape = [] {
        const char *e = getenv("MR_MBLUR_TILE");
        return !e ? MBLUR_DEFAULT_SHAPE : !strcmp(e, "32x32") ? 0 : !strcmp(e, "32x32x256") ? 1 : !strcmp(e, "16x16") ? 2 : MBLUR_DEFAULT_SHAPE;
    }();
    return shape;
}

// What a frame slot owns for the pass: the velocity buffer, the tables on the device and a page-locked copy of them that
// the upload reads, with an event behind the upload -- the host waits for it before it writes the next frame's tables
// there (a frame in flight on the slot's stream keeps its own; frames on other streams have other slots).
struct MotionSlot {
    DevBuf d_tables, d_vel;
    void *h_tables = nullptr;
    size_t h_cap = 0;
    hipEvent_t copied = nullptr;
    bool pending = false;
    void release()
    {
        d_tables.release(); d_vel.release();
        if (h_tables) (void)hipHostFree(h_tables);
        if (copied) (void)hipEventDestroy(copied);
        h_tables = nullptr; h_cap = 0; copied = nullptr; pending = false;
    }
};

// k_velocity and k_mblur from a frame's own z-buffer, winner map and float frame into the slot's velocity buffer and `out`,
// on the frame's stream behind its tile kernel, marked for mr_debug_motion_times.  `p` is the copy the frame's plan took.
// Between the two, where the scene has flagged models and the snapshot they need (motion_faces_due), k_face_homography and
// k_velocity_faces overwrite those models' U; k_mblur's span then starts at a mark of its own.
int launch_motion(mr_scene *sc, hipStream_t stream, MotionSlot &ms, MotionFacesSlot &faces, const double *zbuf, const int32_t *winner, const float *frame, float *out,
                  int width, int height, const mr::MotionParams &p)
{
    mr_scene::Motion &a = sc->motion;
    if (!a.ev_ok) {
        for (hipEvent_t &e : a.ev) HIP_TRY(hipEventCreate(&e));
        a.ev_ok = true;
    }
    const size_t bytes = a.tables.size() * sizeof(double);
    if (!ms.copied) HIP_TRY(hipEventCreateWithFlags(&ms.copied, hipEventDisableTiming));
    if (ms.pending) { HIP_TRY(hipEventSynchronize(ms.copied)); ms.pending = false; }
    if (bytes > ms.h_cap) {
        if (ms.h_tables) HIP_TRY(hipHostFree(ms.h_tables));
        ms.h_tables = nullptr; ms.h_cap = 0;
        HIP_TRY(hipHostMalloc(&ms.h_tables, bytes * 2, hipHostMallocDefault));
        ms.h_cap = bytes * 2;
    }
    // (the models' first faces are the scene's of this moment: a commit may have moved them since the description came)
    int32_t *off = reinterpret_cast<int32_t *>(a.tables.data() + (size_t)p.n_classes * mr::MOTION_T + mr::MOTION_B);
    for (int32_t m = 0; m < p.n_models; ++m) off[m] = sc->model_face_off[m];
    std::memcpy(ms.h_tables, a.tables.data(), bytes);
    HIP_TRY(ms.d_tables.ensure(bytes));
    HIP_TRY(ms.d_vel.ensure((size_t)width * height * 2 * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(ms.d_tables.p, ms.h_tables, bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(ms.copied, stream));
    ms.pending = true;
    HIP_TRY(hipEventRecord(a.ev[0], stream));
    mr_motion::launch_velocity(stream, zbuf, winner, ms.d_tables.as<double>(), ms.d_vel.as<float>(), width, height, p);
    HIP_TRY(hipEventRecord(a.ev[1], stream));
    a.blur_from = 1;
    if (motion_faces_due(sc)) {
        if (int rc = launch_motion_faces(sc, stream, faces, winner, ms.d_vel.as<float>(), width, height)) return rc;
        HIP_TRY(hipEventRecord(a.ev[3], stream));
        a.blur_from = 3;
    }
    mr_motion::launch_blur(stream, zbuf, ms.d_vel.as<float>(), frame, out, width, height, p, mblur_shape());
    HIP_TRY(hipEventRecord(a.ev[2], stream));
    a.marked = true;
    a.frames += 1; a.rows = height; a.cols = width;
    return MR_OK;
}

inline bool motion_size_ok(int32_t height, int32_t width) { return height > 0 && width > 0 && height <= 32767 && width <= 32767; }

// The velocity's definition on the host.
int host_velocity(const double *z, const int32_t *winner, const int32_t *face_off, int32_t height, int32_t width, const mr_motion_desc *d, float *out)
{
    if (!z || !winner || !d || !out) return fail(MR_E_INVALID, "mr_host_velocity: NULL argument");
    if (!motion_size_ok(height, width)) return fail(MR_E_INVALID, "mr_host_velocity: resolution out of range");
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
    if (!motion_size_ok(height, width)) return fail(MR_E_INVALID, "mr_host_motion_blur: resolution out of range");
    mr_motion_desc scalars = *d;                       // (the blur reads the depth map and the shutter only)
    scalars.n_models = 0; scalars.class_of_model = nullptr;
    mr::MotionParams p;
    std::vector<double> tables;
    if (int rc = motion_params(&scalars, nullptr, p, tables)) return rc;
    const size_t n = (size_t)height * width;
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<float> e(n), h(n), dx(n), dy(n), inv(n);
    float top = 0.0f;
    for (size_t i = 0; i < n; ++i) {
        const float v = mr::ao_eye_depth(p.m, z[i]);
        e[i] = std::isfinite(z[i]) && std::isfinite(v) ? v : inf;                    // +inf: background
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

// the entry's device buffers: released when it returns, by whichever way, once the stream has drained
struct MotionPostBuffers {
    DevBuf z, winner, tables, vel, a, b;
    ~MotionPostBuffers()
    {
        if (g_initialised) (void)hipStreamSynchronize(g_stream);
        for (DevBuf *d : { &z, &winner, &tables, &vel, &a, &b }) d->release();
    }
};

// mr_debug_motion_post: the two kernels on the caller's arrays through the library's own launches, the workgroup shape an
// argument and not the environment's.  Every refusal comes before any device call; the scene's slots, its last frame and
// what mr_debug_motion reports stay as they were.
int debug_motion_post(mr_scene *sc, const double *z, const int32_t *winner, const float *frame, const int32_t *face_off, int32_t height,
                      int32_t width, const mr_motion_desc *d, int32_t shape, float *out_velocity, float *out_frame)
{
    if (!sc || !z || !winner || !frame || !d || !out_velocity || !out_frame) return fail(MR_E_INVALID, "mr_debug_motion_post: NULL argument");
    if (!motion_size_ok(height, width)) return fail(MR_E_INVALID, "mr_debug_motion_post: resolution out of range");
    if (shape < 0 || shape > 2) return fail(MR_E_INVALID, "mr_debug_motion_post: the workgroup shape of k_mblur is 0, 1 or 2");
    mr::MotionParams p;
    std::vector<double> tables;
    if (int rc = motion_params(d, face_off, p, tables)) return rc;
    if (int rc = motion_linked()) return rc;
    if (int rc = ensure_init()) return rc;
    const size_t n = (size_t)height * width;
    MotionPostBuffers buf;
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
