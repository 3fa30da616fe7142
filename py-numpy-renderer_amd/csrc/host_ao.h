// host_ao.h -- ambient obscurance from the z-buffer (ao_def.h has the definition): the scene's description as the kernel
// takes it, the launch of k_ao behind a frame's tile kernel and of the full resolve that follows it, and the same
// arithmetic on the host, bit for bit (host_ao: plain C++, no device).
#pragma once

// the launch of ao.hip, the library's third translation unit, and the accumulation's resolve (accum.hip), which turns the
// darkened float frame into the frame's bytes; weak, so that a library linked without them still loads: it refuses the
// obscurance instead
namespace mr_ao {
__attribute__((weak)) void launch(hipStream_t stream, const double *zbuf, float *frame, int width, int height, const mr::AoParams &p,
                                  int shape);
}  // namespace mr_ao
namespace mr_accum {
__attribute__((weak)) void launch_resolve(hipStream_t stream, const float *acc, int width, int height, int shift, float scale,
                                          const float *gamma_lut, uint8_t *out);
}  // namespace mr_accum

namespace {

inline int ao_linked()
{
    if (&mr_ao::launch && &mr_accum::launch_resolve) return MR_OK;
    return fail(MR_E_UNSUPPORTED, "this library was linked without ao.hip or accum.hip: no ambient obscurance (build it with __graft_entry__.build())");
}

// The description as the kernel and the mirror take it: every float32 it uses, checked.
int ao_params(const mr_ao_desc *d, mr::AoParams &p)
{
    auto positive = [](double v, float &out) { out = (float)v; return std::isfinite(out) && out > 0.0f; };
    for (int i = 0; i < 4; ++i) {
        if (!std::isfinite(d->depth_map[i])) return fail(MR_E_INVALID, "ambient occlusion: the depth map must be finite");
        p.m[i] = d->depth_map[i];
    }
    float radius;
    if (!positive(d->radius, radius)) return fail(MR_E_INVALID, "ambient occlusion: radius must be finite and > 0 as float32");
    if (!positive(d->strength, p.strength) || p.strength > 8.0f)
        return fail(MR_E_INVALID, "ambient occlusion: strength must be finite, > 0 and <= 8 as float32");
    if (!positive(d->depth_range, p.range)) return fail(MR_E_INVALID, "ambient occlusion: depth_range must be finite and > 0 as float32");
    p.bias = (float)d->bias;
    if (!std::isfinite(p.bias) || p.bias < 0.0f) return fail(MR_E_INVALID, "ambient occlusion: bias must be finite and >= 0 as float32");
    if (!positive(d->k, p.k)) return fail(MR_E_INVALID, "ambient occlusion: k must be finite and > 0 as float32");
    if (d->perspective != 0 && d->perspective != 1) return fail(MR_E_INVALID, "ambient occlusion: perspective is 0 or 1");
    p.inv_fall = (float)(1.0 / d->radius);
    if (!std::isfinite(p.inv_fall)) return fail(MR_E_INVALID, "ambient occlusion: radius must be finite and > 0 as float32");
    p.perspective = d->perspective;
    return MR_OK;
}

void ao_release(mr_scene::Ao &a)
{
    if (a.ev_ok)
        for (hipEvent_t &e : a.ev) (void)hipEventDestroy(e);
    a = mr_scene::Ao();
}

// workgroup shape of k_ao (ao.hip, launch): MR_AO_TILE=64x64 | 32x32 | 64x16 forces one (host_env.h)
constexpr int AO_DEFAULT_SHAPE = 0;
inline int ao_shape()
{
    static const int shape = [] {
        const char *e = getenv("MR_AO_TILE");
        return !e ? AO_DEFAULT_SHAPE : !strcmp(e, "64x64") ? 0 : !strcmp(e, "32x32") ? 1 : !strcmp(e, "64x16") ? 2 : AO_DEFAULT_SHAPE;
    }();
    return shape;
}

// k_ao on a frame's own z-buffer and float frame, on the frame's stream behind its tile kernel, marked for
// mr_debug_ao_times.  `p` is the copy the frame's plan took: the scene's description may change while it is in flight.
int launch_ao(mr_scene *sc, hipStream_t stream, const double *zbuf, float *frame, int width, int height, const mr::AoParams &p)
{
    mr_scene::Ao &a = sc->ao;
    if (!a.ev_ok) {
        for (hipEvent_t &e : a.ev) HIP_TRY(hipEventCreate(&e));
        a.ev_ok = true;
    }
    HIP_TRY(hipEventRecord(a.ev[0], stream));
    mr_ao::launch(stream, zbuf, frame, width, height, p, ao_shape());
    HIP_TRY(hipEventRecord(a.ev[1], stream));
    a.marked = true;
    a.frames += 1; a.rows = height; a.cols = width;
    return MR_OK;
}

// The definition on the host.
int host_ao(const double *z, const float *frame, int32_t height, int32_t width, const mr_ao_desc *d, float *out)
{
    if (!z || !frame || !d || !out) return fail(MR_E_INVALID, "mr_host_ao: NULL argument");
    if (height <= 0 || width <= 0 || height > 32767 || width > 32767) return fail(MR_E_INVALID, "mr_host_ao: resolution out of range");
    mr::AoParams p;
    if (int rc = ao_params(d, p)) return rc;
    const size_t n = (size_t)height * width;
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<float> e(n);
    for (size_t i = 0; i < n; ++i) {
        const float v = mr::ao_eye_depth(p.m, z[i]);
        e[i] = std::isfinite(z[i]) && std::isfinite(v) ? v : inf;            // +inf: background
    }
    const float taps[mr::AO_PAIRS][2] = MR_AO_TAP_TABLE;
    auto at = [&](int x, int y) { return x >= 0 && x < width && y >= 0 && y < height ? e[(size_t)y * width + x] : inf; };
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t i = (size_t)y * width + x;
            const float ep = e[i];
            float ao = 1.0f;
            if (ep < inf) {
                const float rp = mr::ao_footprint(p, ep);
                float sum = 0.0f;
                for (int t = 0; t < mr::AO_PAIRS; ++t) {
                    const int dx = (int)rintf(taps[t][0] * rp), dy = (int)rintf(taps[t][1] * rp);
                    sum = sum + mr::ao_pair(p, ep, at(x + dx, y + dy), at(x - dx, y - dy));
                }
                ao = mr::ao_factor(p, sum);
            }
            for (int c = 0; c < 3; ++c) out[i * 3 + c] = ep < inf ? frame[i * 3 + c] * ao : frame[i * 3 + c];
        }
    return MR_OK;
}

}  // namespace
