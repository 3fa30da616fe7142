// host_ao.h -- ambient obscurance from the z-buffer (ao_def.h has the definition): the scene's description as the kernel
// takes it, the launch of k_ao behind a frame's tile kernel and of the full resolve that follows it, and the same
// arithmetic on the host, bit for bit (host_ao: plain C++, no device).
#pragma once

namespace {

// k_ao is ao.hip's; the bytes of a darkened frame are the accumulation's resolve of its float frame (accum.hip)
inline int ao_linked()
{
    return linked("this library was linked without ao.hip or accum.hip: no ambient obscurance (build it with __graft_entry__.build())",
                  &mr_ao::launch, &mr_accum::launch_resolve);
}

// The description as the kernel and the mirror take it: every float32 it uses, checked.
int ao_params(const mr_ao_desc *d, mr::AoParams &p)
{
    if (int rc = take_depth_map("ambient occlusion", d->depth_map, p.m)) return rc;
    float radius;
    if (!positive_f32(d->radius, radius)) return fail(MR_E_INVALID, "ambient occlusion: radius must be finite and > 0 as float32");
    if (!positive_f32(d->strength, p.strength) || p.strength > 8.0f)
        return fail(MR_E_INVALID, "ambient occlusion: strength must be finite, > 0 and <= 8 as float32");
    if (!positive_f32(d->depth_range, p.range)) return fail(MR_E_INVALID, "ambient occlusion: depth_range must be finite and > 0 as float32");
    p.bias = (float)d->bias;
    if (!std::isfinite(p.bias) || p.bias < 0.0f) return fail(MR_E_INVALID, "ambient occlusion: bias must be finite and >= 0 as float32");
    if (!positive_f32(d->k, p.k)) return fail(MR_E_INVALID, "ambient occlusion: k must be finite and > 0 as float32");
    if (d->perspective != 0 && d->perspective != 1) return fail(MR_E_INVALID, "ambient occlusion: perspective is 0 or 1");
    p.inv_fall = (float)(1.0 / d->radius);
    if (!std::isfinite(p.inv_fall)) return fail(MR_E_INVALID, "ambient occlusion: radius must be finite and > 0 as float32");
    p.perspective = d->perspective;
    return MR_OK;
}

// k_ao on a frame's own z-buffer and float frame, on the frame's stream behind its tile kernel, marked for
// mr_debug_ao_times.  `p` is the copy the frame's plan took: the scene's description may change while it is in flight;
// `shape` is the plan's too (Env::ao_shape).
int launch_ao(mr_scene *sc, hipStream_t stream, const double *zbuf, float *frame, int width, int height, const mr::AoParams &p, int shape)
{
    return marked_launch(sc->ao, stream, width, height, [&] { mr_ao::launch(stream, zbuf, frame, width, height, p, shape); return MR_OK; });
}

// The definition on the host.
int host_ao(const double *z, const float *frame, int32_t height, int32_t width, const mr_ao_desc *d, float *out)
{
    if (!z || !frame || !d || !out) return fail(MR_E_INVALID, "mr_host_ao: NULL argument");
    if (!frame_size_ok(height, width)) return fail(MR_E_INVALID, "mr_host_ao: resolution out of range");
    mr::AoParams p;
    if (int rc = ao_params(d, p)) return rc;
    const size_t n = (size_t)height * width;
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<float> e(n);
    for (size_t i = 0; i < n; ++i) e[i] = host_eye_depth(p.m, z[i]);
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
