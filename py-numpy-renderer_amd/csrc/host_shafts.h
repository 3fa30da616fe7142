// host_shafts.h -- light shafts, the sky's light marched towards a light's place on the screen (shafts_def.h has the
// definition): the scene's description as the kernels take it, the layout of S and R in a frame slot, the three launches
// behind a frame's motion blur and in front of its bloom, the same arithmetic on the host, bit for bit (host_light_shafts:
// plain C++, no device), and mr_debug_light_shafts_post, the kernels on buffers a caller supplies.  The pass keeps nothing
// from frame to frame.  The bytes of such a frame are the full resolve of its float frame (host_frame.h,
// launch_post_resolve).
#pragma once

namespace {

// The description as the kernels and the mirror take it, checked.
int shafts_params(const mr_light_shafts_desc *d, mr::ShaftsParams &p)
{
    p = mr::ShaftsParams();
    if (!std::isfinite(d->light_x) || !std::isfinite(d->light_y)) return fail(MR_E_INVALID, "light shafts: the light's position must be finite");
    if (!(std::isfinite(d->threshold) && d->threshold >= 0.0f)) return fail(MR_E_INVALID, "light shafts: threshold must be finite and >= 0");
    if (!(std::isfinite(d->gain) && d->gain > 0.0f)) return fail(MR_E_INVALID, "light shafts: gain must be finite and > 0");
    if (!(std::isfinite(d->step) && d->step > 0.0f)) return fail(MR_E_INVALID, "light shafts: step must be finite and > 0");
    if (d->samples < 1 || d->samples > mr::SHAFTS_MAX_SAMPLES) return fail(MR_E_INVALID, "light shafts: samples must lie in 1 .. 128");
    if (d->halvings < 1 || d->halvings > mr::SHAFTS_MAX_LEVELS) return fail(MR_E_INVALID, "light shafts: halvings must lie in 1 .. 4");
    for (int i = 0; i < d->samples; ++i)
        if (!(std::isfinite(d->weights[i]) && d->weights[i] >= 0.0f)) return fail(MR_E_INVALID, "light shafts: the weights must be finite and >= 0");
    p.light_x = d->light_x; p.light_y = d->light_y; p.threshold = d->threshold; p.gain = d->gain; p.step = d->step;
    p.samples = d->samples; p.levels = d->halvings;
    for (int i = 0; i < d->samples; ++i) p.weights[i] = d->weights[i];      // (the others stay +0: no tap reads them)
    return MR_OK;
}

// S and R of a sample grid: (h x w) samples each, the grid halved `levels` times with rounding up.  On the device a
// sample is 16 bytes, (r, g, b, 0), S in front of R in the slot's one buffer.
struct ShaftsLevel {
    int w, h;
    size_t samples() const { return (size_t)w * h; }
    size_t device_floats() const { return samples() * 4; }        // of S, and of R
};

ShaftsLevel shafts_level(int width, int height, int levels)
{
    ShaftsLevel lv = { width, height };
    for (int l = 0; l < levels; ++l) { lv.w = mr::bloom_half(lv.w); lv.h = mr::bloom_half(lv.h); }
    return lv;
}

// The three launches on one stream; `between(mark)` is called with 1 behind the source and 2 behind the march.
template <class Between>
int shafts_chain(hipStream_t stream, float *frame, const double *zbuf, float *d_s, float *d_r, int width, int height, const mr::ShaftsParams &p,
                 Between &&between)
{
    const ShaftsLevel lv = shafts_level(width, height, p.levels);
    mr_shafts::launch_source(stream, frame, zbuf, d_s, width, height, lv.w, lv.h, p.threshold, p.levels);
    if (int rc = between(1)) return rc;
    mr_shafts::launch_march(stream, d_s, d_r, lv.w, lv.h, p);
    if (int rc = between(2)) return rc;
    mr_shafts::launch_composite(stream, frame, d_r, width, height, lv.w, lv.h, p.levels, p.gain);
    return MR_OK;
}

// The pass on a frame's own float frame, z-buffer and its slot's buffer, on the frame's stream, marked for
// mr_debug_light_shafts_times: round the source, the march and the composite.  `p` is the copy the frame's plan took.
int launch_light_shafts(mr_scene *sc, hipStream_t stream, float *frame, const double *zbuf, float *buf, int width, int height, const mr::ShaftsParams &p)
{
    mr_scene::Shafts &a = sc->shafts;
    const ShaftsLevel lv = shafts_level(width, height, p.levels);
    a.last_levels = p.levels;
    return marked_launch(a, stream, width, height, [&]() -> int {
        return shafts_chain(stream, frame, zbuf, buf, buf + lv.device_floats(), width, height, p, [&](int mark) { return a.marks.record(mark, stream); });
    });
}

// fetch(A, qx, qy) on the host, A (h x w x 3); false: outside, v untouched
bool host_shafts_fetch(const float *level, int w, int h, float qx, float qy, float v[3])
{
    mr::ShaftsTap t;
    if (!mr::shafts_tap(qx, qy, w, h, t)) return false;
    const float *r0 = level + (size_t)t.y0 * w * 3, *r1 = level + (size_t)t.y1 * w * 3;
    for (int c = 0; c < 3; ++c) v[c] = mr::shafts_bilerp(r0[t.x0 * 3 + c], r0[t.x1 * 3 + c], r1[t.x0 * 3 + c], r1[t.x1 * 3 + c], t.fx, t.fy);
    return true;
}

// The definition on the host: every level of the tree is an array here.  out_source and out_march (may be NULL) receive S
// and R, (H_d, W_d, 3).
int host_light_shafts(const float *frame, const double *zbuf, int32_t height, int32_t width, const mr_light_shafts_desc *d, float *out, float *out_source,
                      float *out_march)
{
    if (!frame || !zbuf || !d || !out) return fail(MR_E_INVALID, "mr_host_light_shafts: NULL argument");
    if (frame == out) return fail(MR_E_INVALID, "mr_host_light_shafts: out_frame must not be the frame");
    if (!frame_size_ok(height, width)) return fail(MR_E_INVALID, "mr_host_light_shafts: resolution out of range");
    mr::ShaftsParams p;
    if (int rc = shafts_params(d, p)) return rc;
    int w = width, h = height;
    std::vector<float> level((size_t)w * h * 3), next;
    for (size_t i = 0; i < (size_t)w * h; ++i) {
        const float *q = frame + i * 3;
        const float k = mr::bloom_bright(q[0], q[1], q[2], p.threshold);
        const bool sky = mr::shafts_sky(zbuf[i]);
        for (int c = 0; c < 3; ++c) level[i * 3 + c] = sky ? q[c] * k : 0.0f;
    }
    for (int l = 0; l < p.levels; ++l) {
        const int nw = mr::bloom_half(w), nh = mr::bloom_half(h);
        next.assign((size_t)nw * nh * 3, 0.0f);
        auto at = [&](int x, int y, int c) { return x < w && y < h ? level[((size_t)y * w + x) * 3 + c] : 0.0f; };
        for (int y = 0; y < nh; ++y)
            for (int x = 0; x < nw; ++x)
                for (int c = 0; c < 3; ++c)
                    next[((size_t)y * nw + x) * 3 + c] = mr::shafts_quad(mr::shafts_pair(at(2 * x, 2 * y, c), at(2 * x + 1, 2 * y, c)),
                                                                         mr::shafts_pair(at(2 * x, 2 * y + 1, c), at(2 * x + 1, 2 * y + 1, c)));
        level.swap(next);
        w = nw; h = nh;
    }
    if (out_source) std::memcpy(out_source, level.data(), level.size() * sizeof(float));
    std::vector<float> march((size_t)w * h * 3);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const float cx = (float)x, cy = (float)y;
            const float dx = mr::shafts_ray_delta(p.light_x, cx, p.step), dy = mr::shafts_ray_delta(p.light_y, cy, p.step);
            float acc[3] = { 0.0f, 0.0f, 0.0f }, v[3];
            for (int i = 0; i < p.samples; ++i)
                if (host_shafts_fetch(level.data(), w, h, mr::shafts_ray_at(cx, dx, i), mr::shafts_ray_at(cy, dy, i), v))
                    for (int c = 0; c < 3; ++c) acc[c] = mr::shafts_add(acc[c], p.weights[i], v[c]);
            for (int c = 0; c < 3; ++c) march[((size_t)y * w + x) * 3 + c] = acc[c];
        }
    if (out_march) std::memcpy(out_march, march.data(), march.size() * sizeof(float));
    const float inv = mr::shafts_inv_scale(p.levels);
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            float v[3] = { 0.0f, 0.0f, 0.0f };
            (void)host_shafts_fetch(march.data(), w, h, mr::shafts_coarse_at(x, inv), mr::shafts_coarse_at(y, inv), v);
            for (int c = 0; c < 3; ++c) {
                const size_t i = ((size_t)y * width + x) * 3 + c;
                out[i] = mr::bloom_composite(frame[i], p.gain, v[c]);
            }
        }
    return MR_OK;
}

constexpr size_t SHAFTS_GUARD = 256;                     // bytes of sentinel in front of and behind every device buffer of the debug entry
constexpr unsigned char SHAFTS_SENTINEL = 0xa5;

// mr_debug_light_shafts_post: the three kernels on the caller's frame and z-buffer through the library's own launches.  The
// frame, the z-buffer, S and R each lie between guards of sentinel bytes on the device; a guard byte that changed is
// MR_E_DEVICE.  Every refusal comes before any device call; the scene's slots and what mr_debug_light_shafts reports stay
// as they were.
int debug_light_shafts_post(mr_scene *sc, const float *frame, const double *zbuf, int32_t height, int32_t width, const mr_light_shafts_desc *d,
                            float *out_frame, float *out_source, float *out_march)
{
    if (!sc || !frame || !zbuf || !d || !out_frame) return fail(MR_E_INVALID, "mr_debug_light_shafts_post: NULL argument");
    if (!frame_size_ok(height, width)) return fail(MR_E_INVALID, "mr_debug_light_shafts_post: resolution out of range");
    mr::ShaftsParams p;
    if (int rc = shafts_params(d, p)) return rc;
    if (int rc = shafts_linked()) return rc;
    if (int rc = ensure_init()) return rc;
    const ShaftsLevel lv = shafts_level(width, height, p.levels);
    const size_t G = SHAFTS_GUARD, n = (size_t)height * width;
    const size_t bytes[4] = { n * 3 * sizeof(float), n * sizeof(double), lv.device_floats() * sizeof(float), lv.device_floats() * sizeof(float) };
    DevBuf buf[4];                                       // the frame, the z-buffer, S, R
    Drained drained{ &buf[0], &buf[1], &buf[2], &buf[3] };
    char *at[4];
    for (int i = 0; i < 4; ++i) {
        HIP_TRY(buf[i].ensure(bytes[i] + 2 * G));
        HIP_TRY(hipMemsetAsync(buf[i].p, SHAFTS_SENTINEL, bytes[i] + 2 * G, g_stream));
        at[i] = buf[i].as<char>() + G;
    }
    HIP_TRY(hipMemcpyAsync(at[0], frame, bytes[0], hipMemcpyHostToDevice, g_stream));
    HIP_TRY(hipMemcpyAsync(at[1], zbuf, bytes[1], hipMemcpyHostToDevice, g_stream));
    const int rc = shafts_chain(g_stream, reinterpret_cast<float *>(at[0]), reinterpret_cast<const double *>(at[1]), reinterpret_cast<float *>(at[2]),
                                reinterpret_cast<float *>(at[3]), width, height, p, [](int) { return MR_OK; });
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    std::vector<unsigned char> guards(8 * G);
    std::vector<float> s4(lv.device_floats()), r4(lv.device_floats());
    for (int i = 0; i < 4; ++i) {
        HIP_TRY(hipMemcpyAsync(guards.data() + 2 * i * G, buf[i].p, G, hipMemcpyDeviceToHost, g_stream));
        HIP_TRY(hipMemcpyAsync(guards.data() + (2 * i + 1) * G, at[i] + bytes[i], G, hipMemcpyDeviceToHost, g_stream));
    }
    HIP_TRY(hipMemcpyAsync(out_frame, at[0], bytes[0], hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipMemcpyAsync(s4.data(), at[2], bytes[2], hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipMemcpyAsync(r4.data(), at[3], bytes[3], hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    int touched = 0;
    for (unsigned char g : guards) touched += g != SHAFTS_SENTINEL;
    if (touched)
        return fail(MR_E_DEVICE, "mr_debug_light_shafts_post: " + std::to_string(touched) + " guard bytes round the frame, the z-buffer, S and R changed: a kernel wrote out of bounds");
    // (16 bytes a sample on the device, three floats for the caller; the fourth is the +0 the kernels wrote)
    for (size_t i = 0; i < lv.samples(); ++i) {
        if (s4[i * 4 + 3] != 0.0f || r4[i * 4 + 3] != 0.0f) return fail(MR_E_DEVICE, "mr_debug_light_shafts_post: the padding of a sample of S or R is not 0");
        for (int c = 0; c < 3; ++c) {
            if (out_source) out_source[i * 3 + c] = s4[i * 4 + c];
            if (out_march) out_march[i * 3 + c] = r4[i * 4 + c];
        }
    }
    return MR_OK;
}

}  // namespace
