// host_bloom.h -- bloom, a glow round bright samples from a resolution pyramid (bloom_def.h has the definition): the scene's
// description as the kernels take it, the pyramid's layout, the 2 L launches behind a frame's motion blur and in front of
// its overlay, the same arithmetic on the host, bit for bit (host_bloom: plain C++, no device), and mr_debug_bloom_post,
// the kernels on buffers a caller supplies.  The pass keeps nothing from frame to frame.  The bytes of such a frame are the
// full resolve of its float frame (host_frame.h, launch_post_resolve).
#pragma once

namespace {

// The description as the kernels and the mirror take it: every float32 it uses, checked.
int bloom_params(const mr_bloom_desc *d, mr::BloomParams &p)
{
    if (!(positive_f32(d->threshold, p.threshold) || p.threshold == 0.0f))
        return fail(MR_E_INVALID, "bloom: threshold must be finite and >= 0 as float32");
    if (!positive_f32(d->gain, p.gain)) return fail(MR_E_INVALID, "bloom: gain must be finite and > 0 as float32");
    if (d->levels < 1 || d->levels > mr::BLOOM_MAX_LEVELS) return fail(MR_E_INVALID, "bloom: levels must lie in 1 .. 8");
    p.levels = d->levels;
    return MR_OK;
}

// The pyramid of a sample grid: level l = 1 .. n is h[l] x w[l] samples, three floats each, at float offset off[l] of the
// slot's buffer ([0] is the grid itself and has no place there); `floats` is the buffer's size.
struct BloomPyramid {
    int n;
    int w[mr::BLOOM_MAX_LEVELS + 1], h[mr::BLOOM_MAX_LEVELS + 1];
    size_t off[mr::BLOOM_MAX_LEVELS + 1], floats;
    size_t level_floats(int l) const { return (size_t)w[l] * h[l] * 3; }
};

BloomPyramid bloom_pyramid(int width, int height, int levels)
{
    BloomPyramid py = {};
    py.n = levels;
    py.w[0] = width; py.h[0] = height;
    for (int l = 1; l <= levels; ++l) {
        py.w[l] = mr::bloom_half(py.w[l - 1]); py.h[l] = mr::bloom_half(py.h[l - 1]);
        py.off[l] = py.floats;
        py.floats += py.level_floats(l);
    }
    return py;
}

// The down chain into `pyr` (the frame's slot's, bloom_pyramid's layout), the up chain in place over it and the composite
// in place on `frame`, on one stream; between the chains `between(mark)` is called with 1 and 2.
template <class Between>
int bloom_chain(hipStream_t stream, float *frame, float *pyr, const BloomPyramid &py, const mr::BloomParams &p, int shape, Between &&between)
{
    for (int l = 1; l <= py.n; ++l)
        mr_bloom::launch_down(stream, l == 1 ? frame : pyr + py.off[l - 1], pyr + py.off[l], py.w[l - 1], py.h[l - 1], p.threshold, l == 1, shape);
    if (int rc = between(1)) return rc;
    for (int l = py.n - 1; l >= 1; --l) mr_bloom::launch_up(stream, pyr + py.off[l], pyr + py.off[l + 1], py.w[l], py.h[l]);
    if (int rc = between(2)) return rc;
    mr_bloom::launch_composite(stream, frame, pyr + py.off[1], py.w[0], py.h[0], p.gain);
    return MR_OK;
}

// The 2 L launches on a frame's own float frame and its slot's pyramid buffer, on the frame's stream, marked for
// mr_debug_bloom_times: round the down chain, the up chain and the composite.  `p` is the copy the frame's plan took;
// `shape` is k_bloom_down's (Env::bloom_shape).
int launch_bloom(mr_scene *sc, hipStream_t stream, float *frame, float *pyr, int width, int height, const mr::BloomParams &p, int shape)
{
    mr_scene::Bloom &a = sc->bloom;
    const BloomPyramid py = bloom_pyramid(width, height, p.levels);
    a.last_levels = p.levels;
    return marked_launch(a, stream, width, height, [&]() -> int {
        return bloom_chain(stream, frame, pyr, py, p, shape, [&](int mark) { return a.marks.record(mark, stream); });
    });
}

// one level down on the host; `first`: src is the frame and the bright pass is applied on the way in
void host_bloom_down(const float *src, float *dst, int sw, int sh, float threshold, bool first)
{
    const int dw = mr::bloom_half(sw), dh = mr::bloom_half(sh);
    auto clampi = [](int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); };
    for (int y = 0; y < dh; ++y)
        for (int x = 0; x < dw; ++x) {
            float r[3][4];
            for (int j = 0; j < 4; ++j) {
                const float *row = src + (size_t)clampi(2 * y - 1 + j, sh) * sw * 3;
                float a[4][3];
                for (int i = 0; i < 4; ++i) {
                    const float *q = row + (size_t)clampi(2 * x - 1 + i, sw) * 3;
                    const float k = first ? mr::bloom_bright(q[0], q[1], q[2], threshold) : 1.0f;
                    for (int c = 0; c < 3; ++c) a[i][c] = first ? q[c] * k : q[c];
                }
                for (int c = 0; c < 3; ++c) r[c][j] = mr::bloom_down4(a[0][c], a[1][c], a[2][c], a[3][c]);
            }
            for (int c = 0; c < 3; ++c)
                dst[((size_t)y * dw + x) * 3 + c] = mr::bloom_down_scale(mr::bloom_down4(r[c][0], r[c][1], r[c][2], r[c][3]));
        }
}

// one channel of up(coarse) at fine sample (x, y)
float host_bloom_up(const float *coarse, int cw, int ch, int x, int y, int c)
{
    const int nx = x >> 1, ny = y >> 1, fx = mr::bloom_far(x, cw), fy = mr::bloom_far(y, ch);
    const float *rn = coarse + (size_t)ny * cw * 3, *rf = coarse + (size_t)fy * cw * 3;
    return mr::bloom_up(rn[nx * 3 + c], rn[fx * 3 + c], rf[nx * 3 + c], rf[fx * 3 + c]);
}

// The definition on the host.  out_pyramid (may be NULL) receives D_1 .. D_L and then U_{L-1} .. U_1, packed.
int host_bloom(const float *frame, int32_t height, int32_t width, const mr_bloom_desc *d, float *out, float *out_pyramid)
{
    if (!frame || !d || !out) return fail(MR_E_INVALID, "mr_host_bloom: NULL argument");
    if (frame == out) return fail(MR_E_INVALID, "mr_host_bloom: out_frame must not be the frame");
    if (!frame_size_ok(height, width)) return fail(MR_E_INVALID, "mr_host_bloom: resolution out of range");
    mr::BloomParams p;
    if (int rc = bloom_params(d, p)) return rc;
    const BloomPyramid py = bloom_pyramid(width, height, p.levels);
    std::vector<float> pyr(py.floats);
    for (int l = 1; l <= py.n; ++l)
        host_bloom_down(l == 1 ? frame : pyr.data() + py.off[l - 1], pyr.data() + py.off[l], py.w[l - 1], py.h[l - 1], p.threshold, l == 1);
    if (out_pyramid) std::memcpy(out_pyramid, pyr.data(), py.floats * sizeof(float));
    float *u_out = out_pyramid ? out_pyramid + py.floats : nullptr;
    for (int l = py.n - 1; l >= 1; --l) {
        float *fine = pyr.data() + py.off[l];
        const float *coarse = pyr.data() + py.off[l + 1];
        for (int y = 0; y < py.h[l]; ++y)
            for (int x = 0; x < py.w[l]; ++x)
                for (int c = 0; c < 3; ++c) {
                    float &v = fine[((size_t)y * py.w[l] + x) * 3 + c];
                    v = v + host_bloom_up(coarse, py.w[l + 1], py.h[l + 1], x, y, c);
                }
        if (u_out) {
            std::memcpy(u_out, fine, py.level_floats(l) * sizeof(float));
            u_out += py.level_floats(l);
        }
    }
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x)
            for (int c = 0; c < 3; ++c) {
                const size_t i = ((size_t)y * width + x) * 3 + c;
                out[i] = mr::bloom_composite(frame[i], p.gain, host_bloom_up(pyr.data() + py.off[1], py.w[1], py.h[1], x, y, c));
            }
    return MR_OK;
}

constexpr size_t BLOOM_GUARD = 256;                      // bytes of sentinel in front of and behind the frame and the pyramid
constexpr unsigned char BLOOM_SENTINEL = 0xa5;

// mr_debug_bloom_post: the three kernels on the caller's frame through the library's own launches, the workgroup shape an
// argument and not the environment's.  The frame and the pyramid lie between guards of sentinel bytes on the device; a
// guard byte that changed is MR_E_DEVICE.  Every refusal comes before any device call; the scene's slots and what
// mr_debug_bloom reports stay as they were.
int debug_bloom_post(mr_scene *sc, const float *frame, int32_t height, int32_t width, const mr_bloom_desc *d, int32_t shape, float *out_frame,
                     float *out_pyramid)
{
    if (!sc || !frame || !d || !out_frame) return fail(MR_E_INVALID, "mr_debug_bloom_post: NULL argument");
    if (!frame_size_ok(height, width)) return fail(MR_E_INVALID, "mr_debug_bloom_post: resolution out of range");
    if (shape < 0 || shape > 2) return fail(MR_E_INVALID, "mr_debug_bloom_post: the workgroup shape of k_bloom_down is 0, 1 or 2");
    mr::BloomParams p;
    if (int rc = bloom_params(d, p)) return rc;
    if (int rc = bloom_linked()) return rc;
    if (int rc = ensure_init()) return rc;
    const BloomPyramid py = bloom_pyramid(width, height, p.levels);
    const size_t G = BLOOM_GUARD, f_bytes = (size_t)height * width * 3 * sizeof(float), p_bytes = py.floats * sizeof(float);
    std::vector<unsigned char> guards(4 * G);
    struct { DevBuf f, p; } buf;
    Drained drained{ &buf.f, &buf.p };
    HIP_TRY(buf.f.ensure(f_bytes + 2 * G));
    HIP_TRY(buf.p.ensure(p_bytes + 2 * G));
    float *d_frame = reinterpret_cast<float *>(buf.f.as<char>() + G), *d_pyr = reinterpret_cast<float *>(buf.p.as<char>() + G);
    HIP_TRY(hipMemsetAsync(buf.f.p, BLOOM_SENTINEL, f_bytes + 2 * G, g_stream));
    HIP_TRY(hipMemsetAsync(buf.p.p, BLOOM_SENTINEL, p_bytes + 2 * G, g_stream));
    HIP_TRY(hipMemcpyAsync(d_frame, frame, f_bytes, hipMemcpyHostToDevice, g_stream));
    const int rc = bloom_chain(g_stream, d_frame, d_pyr, py, p, shape, [&](int mark) -> int {
        // (the up chain overwrites D_{L-1} .. D_1: the D's leave in front of it; then the U's, coarsest first)
        if (mark == 1 && out_pyramid) HIP_TRY(hipMemcpyAsync(out_pyramid, d_pyr, p_bytes, hipMemcpyDeviceToHost, g_stream));
        float *u_out = out_pyramid ? out_pyramid + py.floats : nullptr;
        for (int l = py.n - 1; mark == 2 && u_out && l >= 1; --l) {
            HIP_TRY(hipMemcpyAsync(u_out, d_pyr + py.off[l], py.level_floats(l) * sizeof(float), hipMemcpyDeviceToHost, g_stream));
            u_out += py.level_floats(l);
        }
        return MR_OK;
    });
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(guards.data(), buf.f.p, G, hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipMemcpyAsync(guards.data() + G, buf.f.as<char>() + G + f_bytes, G, hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipMemcpyAsync(guards.data() + 2 * G, buf.p.p, G, hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipMemcpyAsync(guards.data() + 3 * G, buf.p.as<char>() + G + p_bytes, G, hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipMemcpyAsync(out_frame, d_frame, f_bytes, hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    int touched = 0;
    for (unsigned char g : guards) touched += g != BLOOM_SENTINEL;
    if (touched) return fail(MR_E_DEVICE, "mr_debug_bloom_post: " + std::to_string(touched) + " guard bytes round the frame and the pyramid changed: a kernel wrote out of bounds");
    return MR_OK;
}

}  // namespace
