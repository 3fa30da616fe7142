// host_dof.h -- thin-lens depth of field from the z-buffer (dof_def.h has the definition): the scene's description as the
// kernel takes it, the launch of k_dof behind a frame's tile kernel (and behind k_ao where that runs), and the same
// arithmetic on the host, bit for bit (host_dof: plain C++, no device).  The bytes of such a frame are the full resolve
// of its float frame, like an obscured frame's (host_frame.h, launch_post_resolve).
#pragma once

// the launch of dof.hip, the library's fourth translation unit; weak, so that a library linked without it still loads: it
// refuses the depth of field instead (the resolve, accum.hip's, is declared in host_ao.h)
namespace mr_dof {
__attribute__((weak)) void launch(hipStream_t stream, const double *zbuf, const float *frame, float *out, int width, int height,
                                  const mr::DofParams &p, int shape);
}  // namespace mr_dof

namespace {

inline int dof_linked()
{
    if (&mr_dof::launch && &mr_accum::launch_resolve) return MR_OK;
    return fail(MR_E_UNSUPPORTED, "this library was linked without dof.hip or accum.hip: no depth of field (build it with __graft_entry__.build())");
}

// The description as the kernel and the mirror take it: every float32 it uses, checked.
int dof_params(const mr_dof_desc *d, mr::DofParams &p)
{
    auto positive = [](double v, float &out) { out = (float)v; return std::isfinite(out) && out > 0.0f; };
    for (int i = 0; i < 4; ++i) {
        if (!std::isfinite(d->depth_map[i])) return fail(MR_E_INVALID, "depth of field: the depth map must be finite");
        p.m[i] = d->depth_map[i];
    }
    if (!positive(d->focus, p.focus)) return fail(MR_E_INVALID, "depth of field: focus must be finite and > 0 as float32");
    if (!positive(d->kf, p.kf)) return fail(MR_E_INVALID, "depth of field: kf must be finite and > 0 as float32");
    if (d->perspective != 0 && d->perspective != 1) return fail(MR_E_INVALID, "depth of field: perspective is 0 or 1");
    p.perspective = d->perspective;
    return MR_OK;
}

void dof_release(mr_scene::Dof &a)
{
    if (a.ev_ok)
        for (hipEvent_t &e : a.ev) (void)hipEventDestroy(e);
    a = mr_scene::Dof();
}

// workgroup shape of k_dof (dof.hip, launch): MR_DOF_TILE=32x32 | 32x32x256 | 16x16 forces one (host_env.h)
constexpr int DOF_DEFAULT_SHAPE = 0;
inline int dof_shape()
{
    static const int shape = [] {
        const char *e = getenv("MR_DOF_TILE");
        return !e ? DOF_DEFAULT_SHAPE : !strcmp(e, "32x32") ? 0 : !strcmp(e, "32x32x256") ? 1 : !strcmp(e, "16x16") ? 2 : DOF_DEFAULT_SHAPE;
    }();
    return shape;
}

// k_dof from a frame's own z-buffer and float frame into `out`, on the frame's stream behind its tile kernel, marked for
// mr_debug_dof_times.  `p` is the copy the frame's plan took: the scene's description may change while it is in flight.
int launch_dof(mr_scene *sc, hipStream_t stream, const double *zbuf, const float *frame, float *out, int width, int height,
               const mr::DofParams &p)
{
    mr_scene::Dof &a = sc->dof;
    if (!a.ev_ok) {
        for (hipEvent_t &e : a.ev) HIP_TRY(hipEventCreate(&e));
        a.ev_ok = true;
    }
    HIP_TRY(hipEventRecord(a.ev[0], stream));
    mr_dof::launch(stream, zbuf, frame, out, width, height, p, dof_shape());
    HIP_TRY(hipEventRecord(a.ev[1], stream));
    a.marked = true;
    a.frames += 1; a.rows = height; a.cols = width;
    return MR_OK;
}

// The definition on the host.  (Its loops are bounded by the frame's largest rr, as the kernel's are by its rectangle's:
// the taps left out fail the test.)
int host_dof(const double *z, const float *frame, int32_t height, int32_t width, const mr_dof_desc *d, float *out)
{
    if (!z || !frame || !d || !out) return fail(MR_E_INVALID, "mr_host_dof: NULL argument");
    if (frame == out) return fail(MR_E_INVALID, "mr_host_dof: out_frame must not be the frame (neighbours' colours are read)");
    if (height <= 0 || width <= 0 || height > 32767 || width > 32767) return fail(MR_E_INVALID, "mr_host_dof: resolution out of range");
    mr::DofParams p;
    if (int rc = dof_params(d, p)) return rc;
    const size_t n = (size_t)height * width;
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<float> s(n), rr(n);
    float top = 0.25f;
    for (size_t i = 0; i < n; ++i) {
        const float v = mr::ao_eye_depth(p.m, z[i]);
        const float e = std::isfinite(z[i]) && std::isfinite(v) ? v : inf;            // +inf: background
        s[i] = mr::dof_coc(p, e);
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
