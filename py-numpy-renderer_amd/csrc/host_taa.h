// host_taa.h -- temporal anti-aliasing (taa_def.h has the definition): the scene's description as the kernels take it,
// the history the scene owns and when a frame's result becomes it, the launch of k_velocity and k_taa behind a frame's tile
// kernel (and behind k_ao where that runs; in front of k_dof and k_mblur, which gather from the stabilised frame), the same
// arithmetic on the host, bit for bit (host_taa: plain C++, no device), and mr_debug_taa_post, the kernel on buffers a
// caller supplies.  The library keeps the colours of the previous frame; it stays stateless about where things were: it
// is handed the velocity's matrices as the motion blur is (host_motion.h).  The bytes of such a frame are the full resolve
// of its float frame (host_frame.h, launch_post_resolve).
#pragma once

namespace {

// The description as the kernels take it, checked: the blend, and the velocity's tables as one block laid out as the motion
// blur's (motion_params: the depth map and the shutter are the blur's own, and filled in here).
int taa_params(const mr_taa_desc *d, const int32_t *face_off, mr::TaaParams &p, mr::MotionParams &vel, std::vector<double> &tables)
{
    p.blend = (float)d->blend;
    if (!(std::isfinite(p.blend) && p.blend > 0.0f && p.blend <= 1.0f))
        return fail(MR_E_INVALID, "temporal anti-aliasing: blend must lie in (0, 1] as float32");
    mr_motion_desc m = {};
    m.depth_map[3] = 1.0; m.shutter = 1.0;
    m.matrices = d->matrices; m.class_of_model = d->class_of_model;
    std::memcpy(m.background, d->background, sizeof m.background);
    m.n_classes = d->n_classes; m.n_models = d->n_models;
    return motion_params(&m, face_off, vel, tables);
}

// whether two table blocks hold the same matrices, background and classes (the models' first faces are the scene's own)
bool same_velocity_tables(const mr::MotionParams &a, const std::vector<double> &ta, const mr::MotionParams &b, const std::vector<double> &tb)
{
    if (a.n_classes != b.n_classes || a.n_models != b.n_models || ta.size() != tb.size()) return false;
    const size_t head = ((size_t)a.n_classes * mr::MOTION_T + mr::MOTION_B) * sizeof(double);
    if (std::memcmp(ta.data(), tb.data(), head)) return false;
    const char *ia = reinterpret_cast<const char *>(ta.data()) + head, *ib = reinterpret_cast<const char *>(tb.data()) + head;
    const size_t offs = (size_t)a.n_models * sizeof(int32_t);
    return std::memcmp(ia + offs, ib + offs, offs) == 0;
}

// the history is forgotten: the next frame has none, and a frame still in flight adopts nothing
void taa_forget(mr_scene *sc)
{
    sc->taa.valid = false;
    sc->taa.epoch += 1;
}

void taa_release(mr_scene *sc)
{
    for (DevBuf &b : sc->taa.d_hist) b.release();
    release_pass(sc->taa);
}

// What a frame with the pass needs of the scene before its first kernel: both history buffers at the frame's size; a
// history of another grid is none.
int grow_history(mr_scene *sc, int width, int height)
{
    mr_scene::Taa &a = sc->taa;
    if (a.valid && (a.hist_rows != height || a.hist_cols != width)) taa_forget(sc);
    for (DevBuf &b : a.d_hist) HIP_TRY(b.ensure((size_t)width * height * 3 * sizeof(float)));
    return MR_OK;
}

// k_velocity (and the per-face pair where due) and k_taa from a frame's own z-buffer, winner map and float frame into the
// slot's velocity buffer, `out` and the history buffer the scene is not reading, on the frame's stream, marked for
// mr_debug_taa_times.  `p` and `vel` are the copies the frame's plan took, `shape` k_taa's (Env::taa_shape).
int launch_taa(mr_scene *sc, hipStream_t stream, MotionSlot &ms, MotionFacesSlot &faces, const double *zbuf, const int32_t *winner, const float *frame,
               float *out, int width, int height, const mr::TaaParams &p, const mr::MotionParams &vel, int shape)
{
    mr_scene::Taa &a = sc->taa;
    if (int rc = stage_velocity(sc, stream, ms, a.tables, vel, width, height)) return rc;
    float *u = ms.d_vel.as<float>();
    const float *hist = a.valid ? a.d_hist[a.cur].as<float>() : nullptr;
    return marked_launch(a, stream, width, height, [&]() -> int {
        mr_motion::launch_velocity(stream, zbuf, winner, ms.tables.d_tables.as<double>(), u, width, height, vel);
        a.velocities += 1;
        if (motion_faces_due(sc))
            if (int rc = launch_motion_faces(sc, stream, faces, winner, u, width, height)) return rc;
        if (int rc = a.marks.record(1, stream)) return rc;
        mr_taa::launch(stream, frame, u, hist, out, a.d_hist[a.cur ^ 1].as<float>(), width, height, p, shape);
        return MR_OK;
    });
}

// A frame with the pass has been enqueued on `fs`: its history waits for the frame's verdict.
void taa_enqueued(mr_scene *sc, const FrameSlot *fs, int width, int height)
{
    mr_scene::Taa &a = sc->taa;
    a.pending = true; a.pending_slot = fs;
    a.pending_rows = height; a.pending_cols = width;
    a.pending_epoch = a.epoch;
}

// The verdict of the frame on `fs` is in (mr_render, mr_render_wait): a frame that was complete hands its history over,
// one that overflowed a work list (or failed) leaves the scene the history it read.
void taa_settle(mr_scene *sc, const FrameSlot *fs, bool complete)
{
    mr_scene::Taa &a = sc->taa;
    if (!a.pending || a.pending_slot != fs) return;
    a.pending = false; a.pending_slot = nullptr;
    if (!complete || a.pending_epoch != a.epoch) return;
    a.cur ^= 1;
    a.valid = true;
    a.hist_rows = a.pending_rows; a.hist_cols = a.pending_cols;
    a.adopted += 1;
}

// The definition on the host.
int host_taa(const float *frame, const float *vel, const float *hist, int32_t height, int32_t width, double blend, float *out)
{
    if (!frame || !vel || !out) return fail(MR_E_INVALID, "mr_host_taa: NULL argument");
    if (out == frame || out == hist) return fail(MR_E_INVALID, "mr_host_taa: out_frame must be neither the frame nor the history (neighbours are read)");
    if (!frame_size_ok(height, width)) return fail(MR_E_INVALID, "mr_host_taa: resolution out of range");
    const float a = (float)blend;
    if (!(std::isfinite(a) && a > 0.0f && a <= 1.0f)) return fail(MR_E_INVALID, "temporal anti-aliasing: blend must lie in (0, 1] as float32");
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t i = (size_t)y * width + x;
            float *o = out + i * 3;
            for (int c = 0; c < 3; ++c) o[c] = frame[i * 3 + c];
            int x0, x1, y0, y1;
            float fx, fy;
            if (!hist || !mr::taa_target(x, y, vel[i * 2], vel[i * 2 + 1], width, height, x0, x1, y0, y1, fx, fy)) continue;
            const float *r0 = hist + (size_t)y0 * width * 3, *r1 = hist + (size_t)y1 * width * 3;
            for (int c = 0; c < 3; ++c) {
                const float h = mr::taa_fetch(r0[x0 * 3 + c], r0[x1 * 3 + c], r1[x0 * 3 + c], r1[x1 * 3 + c], fx, fy);
                auto at = [&](int dx, int dy) {
                    const int qx = std::min(std::max(x + dx, 0), width - 1), qy = std::min(std::max(y + dy, 0), height - 1);
                    return frame[((size_t)qy * width + qx) * 3 + c];
                };
                float mn = at(-1, -1), mx = mn;
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) { const float v = at(dx, dy); mn = fminf(mn, v); mx = fmaxf(mx, v); }
                o[c] = mr::taa_blend(h, mn, mx, o[c], a);
            }
        }
    return MR_OK;
}

constexpr size_t TAA_GUARD = 256;                        // bytes of sentinel in front of and behind each output buffer
constexpr unsigned char TAA_SENTINEL = 0xa5;

// mr_debug_taa_post: k_taa on the caller's arrays through the library's own launch, the workgroup shape an argument and not
// the environment's.  The two output buffers lie between guards of sentinel bytes on the device; out_guard receives the
// number of guard bytes that changed.  Every refusal comes before any device call; the scene's slots, its history and what
// mr_debug_taa reports stay as they were.
int debug_taa_post(mr_scene *sc, const float *frame, const float *vel, const float *hist, int32_t height, int32_t width, double blend,
                   int32_t shape, float *out_frame, float *out_history, int32_t *out_guard)
{
    if (!sc || !frame || !vel || !out_frame || !out_history || !out_guard) return fail(MR_E_INVALID, "mr_debug_taa_post: NULL argument");
    if (!frame_size_ok(height, width)) return fail(MR_E_INVALID, "mr_debug_taa_post: resolution out of range");
    if (shape < 0 || shape > 2) return fail(MR_E_INVALID, "mr_debug_taa_post: the workgroup shape of k_taa is 0, 1 or 2");
    mr::TaaParams p;
    p.blend = (float)blend;
    if (!(std::isfinite(p.blend) && p.blend > 0.0f && p.blend <= 1.0f))
        return fail(MR_E_INVALID, "temporal anti-aliasing: blend must lie in (0, 1] as float32");
    if (int rc = taa_linked()) return rc;
    if (int rc = ensure_init()) return rc;
    const size_t n = (size_t)height * width, G = TAA_GUARD, bytes = n * 3 * sizeof(float);
    std::vector<unsigned char> guards(4 * G);
    struct { DevBuf f, u, h, a, b; } buf;
    Drained drained{ &buf.f, &buf.u, &buf.h, &buf.a, &buf.b };
    HIP_TRY(buf.f.ensure(bytes));
    HIP_TRY(buf.u.ensure(n * 2 * sizeof(float)));
    if (hist) HIP_TRY(buf.h.ensure(bytes));
    HIP_TRY(buf.a.ensure(bytes + 2 * G));
    HIP_TRY(buf.b.ensure(bytes + 2 * G));
    HIP_TRY(hipMemcpyAsync(buf.f.p, frame, bytes, hipMemcpyHostToDevice, g_stream));
    HIP_TRY(hipMemcpyAsync(buf.u.p, vel, n * 2 * sizeof(float), hipMemcpyHostToDevice, g_stream));
    if (hist) HIP_TRY(hipMemcpyAsync(buf.h.p, hist, bytes, hipMemcpyHostToDevice, g_stream));
    HIP_TRY(hipMemsetAsync(buf.a.p, TAA_SENTINEL, bytes + 2 * G, g_stream));
    HIP_TRY(hipMemsetAsync(buf.b.p, TAA_SENTINEL, bytes + 2 * G, g_stream));
    mr_taa::launch(g_stream, buf.f.as<float>(), buf.u.as<float>(), hist ? buf.h.as<float>() : nullptr, reinterpret_cast<float *>(buf.a.as<char>() + G),
                   reinterpret_cast<float *>(buf.b.as<char>() + G), width, height, p, shape);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(guards.data(), buf.a.p, G, hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipMemcpyAsync(guards.data() + G, buf.a.as<char>() + G + bytes, G, hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipMemcpyAsync(guards.data() + 2 * G, buf.b.p, G, hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipMemcpyAsync(guards.data() + 3 * G, buf.b.as<char>() + G + bytes, G, hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipMemcpyAsync(out_frame, buf.a.as<char>() + G, bytes, hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipMemcpyAsync(out_history, buf.b.as<char>() + G, bytes, hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    int32_t touched = 0;
    for (unsigned char g : guards) touched += g != TAA_SENTINEL;
    *out_guard = touched;
    return MR_OK;
}

}  // namespace
