// host_dof.h -- thin-lens depth of field from the z-buffer (dof_def.h has the definition): the scene's description as the
// kernel takes it, the launch of k_dof behind a frame's tile kernel (and behind k_ao where that runs), and the same
// arithmetic on the host, bit for bit (host_dof: plain C++, no device).  The bytes of such a frame are the full resolve
// of its float frame, like an obscured frame's (host_frame.h, launch_post_resolve).
#pragma once

namespace {

// k_dof is dof.hip's; the bytes of a blurred frame are the accumulation's resolve of its float frame (accum.hip)
inline int dof_linked()
{
    return linked("this library was linked without dof.hip or accum.hip: no depth of field (build it with __graft_entry__.build())",
                  &mr_dof::launch, &mr_accum::launch_resolve);
}

// The description as the kernel and the mirror take it: every float32 it uses, checked.
int dof_params(const mr_dof_desc *d, mr::DofParams &p)
{
    if (int rc = take_depth_map("depth of field", d->depth_map, p.m)) return rc;
    if (!positive_f32(d->focus, p.focus)) return fail(MR_E_INVALID, "depth of field: focus must be finite and > 0 as float32");
    if (!positive_f32(d->kf, p.kf)) return fail(MR_E_INVALID, "depth of field: kf must be finite and > 0 as float32");
    if (d->perspective != 0 && d->perspective != 1) return fail(MR_E_INVALID, "depth of field: perspective is 0 or 1");
    p.perspective = d->perspective;
    return MR_OK;
}

// k_dof from a frame's own z-buffer and float frame into `out`, on the frame's stream behind its tile kernel, marked for
// mr_debug_dof_times.  `p` is the copy the frame's plan took: the scene's description may change while it is in flight;
// `shape` is the plan's too (Env::dof_shape).
int launch_dof(mr_scene *sc, hipStream_t stream, const double *zbuf, const float *frame, float *out, int width, int height,
               const mr::DofParams &p, int shape)
{
    return marked_launch(sc->dof, stream, width, height, [&] { mr_dof::launch(stream, zbuf, frame, out, width, height, p, shape); return MR_OK; });
}

// The definition on the host.  (Its loops are bounded by the frame's largest rr, as the kernel's are by its rectangle's:
// the taps left out fail the test.)
int host_dof(const double *z, const float *frame, int32_t height, int32_t width, const mr_dof_desc *d, float *out)
{
    if (!z || !frame || !d || !out) return fail(MR_E_INVALID, "mr_host_dof: NULL argument");
    if (frame == out) return fail(MR_E_INVALID, "mr_host_dof: out_frame must not be the frame (neighbours' colours are read)");
    if (!frame_size_ok(height, width)) return fail(MR_E_INVALID, "mr_host_dof: resolution out of range");
    mr::DofParams p;
    if (int rc = dof_params(d, p)) return rc;
    const size_t n = (size_t)height * width;
    std::vector<float> s(n), rr(n);
    float top = 0.25f;
    for (size_t i = 0; i < n; ++i) {
        s[i] = mr::dof_coc(p, host_eye_depth(p.m, z[i]));
        rr[i] = mr::dof_rr(s[i]);
        top = rr[i] > top ? rr[i] : top;
    }
    int bound = 0;
    while (bound < mr::DOF_MAX_RADIUS && (float)((bound + 1) * (bound + 1)) <= top) ++bound;
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t i = (size_t)y * width + x;
            float W = 0.0f, S[3] = { 0.0f, 0.0f, 0.0f };
            for (int dy = -bound; dy <= bound; ++dy) {
                if (y + dy < 0 || y + dy >= height) continue;
                for (int dx = -bound; dx <= bound; ++dx) {
                    if (x + dx < 0 || x + dx >= width) continue;
                    const size_t q = (size_t)(y + dy) * width + (x + dx);
                    const float rr_t = mr::dof_tap_rr(s[i], rr[i], s[q], rr[q]);
                    if (!((float)(dx * dx + dy * dy) <= rr_t)) continue;
                    const float w = 1.0f / rr_t;
                    W = W + w;
                    for (int c = 0; c < 3; ++c) S[c] = S[c] + w * frame[q * 3 + c];
                }
            }
            for (int c = 0; c < 3; ++c) out[i * 3 + c] = S[c] / W;
        }
    return MR_OK;
}

}  // namespace
