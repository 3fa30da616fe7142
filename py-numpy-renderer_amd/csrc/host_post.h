// host_post.h -- mr_debug_post: the four post-frame kernels (k_ao, k_dof, k_accum_add, k_accum_resolve) on buffers a
// caller supplies, through the library's own launches, with the workgroup shape an argument and not the environment's.
// No frame is rendered: the tests show the kernels depth fields and colours no camera produces (tests/post_fields.py).
// Device buffers of its own, from the allocator the frame slots use; the scene's slots, its last frame and the counters
// of mr_debug_ao / mr_debug_dof / mr_debug_accum stay as they were.
#pragma once

namespace {

int debug_post(mr_scene *sc, const float *frames, const double *z, int32_t n, int32_t height, int32_t width, const mr_ao_desc *ao,
               int32_t ao_shape, const mr_dof_desc *dof, int32_t dof_shape, const double *weights, int32_t shift, double scale,
               float *out_f32, uint8_t *out_rgb)
{
    // ---- every refusal, before any device call
    if (!sc || !frames || !z || !out_f32) return fail(MR_E_INVALID, "mr_debug_post: NULL argument");
    if (n < 1) return fail(MR_E_INVALID, "mr_debug_post: n must be at least 1");
    if (!frame_size_ok(height, width)) return fail(MR_E_INVALID, "mr_debug_post: resolution out of range");
    if (n > 1 && !weights) return fail(MR_E_INVALID, "mr_debug_post: several frames need weights (their sum is the result)");
    if (ao && (ao_shape < 0 || ao_shape > 2)) return fail(MR_E_INVALID, "mr_debug_post: the workgroup shape of k_ao is 0, 1 or 2");
    if (dof && (dof_shape < 0 || dof_shape > 2)) return fail(MR_E_INVALID, "mr_debug_post: the workgroup shape of k_dof is 0, 1 or 2");
    if (shift < 0 || shift > 2) return fail(MR_E_INVALID, "mr_debug_post: shift is 0, 1 or 2");
    if (height % (1 << shift) || width % (1 << shift)) return fail(MR_E_INVALID, "mr_debug_post: height and width must be multiples of 1 << shift");
    float s;
    if (!positive_f32(scale, s)) return fail(MR_E_INVALID, "the scale must be finite and > 0 as float32");
    std::vector<float> w(weights ? (size_t)n : 0);
    for (size_t k = 0; k < w.size(); ++k)
        if (!positive_f32(weights[k], w[k])) return fail(MR_E_INVALID, "a sub-frame's weight must be finite and > 0 as float32");
    mr::AoParams ap;
    mr::DofParams dp;
    if (ao)
        if (int rc = ao_params(ao, ap)) return rc;
    if (dof)
        if (int rc = dof_params(dof, dp)) return rc;
    if (ao)
        if (int rc = ao_linked()) return rc;
    if (dof)
        if (int rc = dof_linked()) return rc;
    if (weights || out_rgb)
        if (int rc = accum_linked()) return rc;

    // ---- the device
    if (int rc = ensure_init()) return rc;
    if (out_rgb)
        if (int rc = ensure_gamma(sc)) return rc;
    const size_t n_samples = (size_t)height * width, n_floats = n_samples * 3;
    struct { DevBuf z, a, b, sum, rgb; } buf;
    Drained drained{ &buf.z, &buf.a, &buf.b, &buf.sum, &buf.rgb };
    HIP_TRY(buf.z.ensure(n_samples * sizeof(double)));
    HIP_TRY(buf.a.ensure(n_floats * sizeof(float)));
    if (dof) HIP_TRY(buf.b.ensure(n_floats * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(buf.z.p, z, n_samples * sizeof(double), hipMemcpyHostToDevice, g_stream));
    if (weights) {
        HIP_TRY(buf.sum.ensure(n_floats * sizeof(float)));
        HIP_TRY(hipMemsetAsync(buf.sum.p, 0xFF, n_floats * sizeof(float), g_stream));      // NaNs: a `first` add that read them would show
    }
    const float *result = nullptr;
    for (int32_t k = 0; k < n; ++k) {
        HIP_TRY(hipMemcpyAsync(buf.a.p, frames + (size_t)k * n_floats, n_floats * sizeof(float), hipMemcpyHostToDevice, g_stream));
        result = buf.a.as<float>();
        if (ao) mr_ao::launch(g_stream, buf.z.as<double>(), buf.a.as<float>(), width, height, ap, ao_shape);
        if (dof) {
            mr_dof::launch(g_stream, buf.z.as<double>(), buf.a.as<float>(), buf.b.as<float>(), width, height, dp, dof_shape);
            result = buf.b.as<float>();
        }
        if (weights) mr_accum::launch_add(g_stream, result, buf.sum.as<float>(), n_floats, w[k], k == 0 ? 1 : 0);
        HIP_TRY(hipGetLastError());
    }
    if (weights) result = buf.sum.as<float>();
    HIP_TRY(hipMemcpyAsync(out_f32, result, n_floats * sizeof(float), hipMemcpyDeviceToHost, g_stream));
    if (out_rgb) {
        const size_t n_bytes = (size_t)(height >> shift) * (width >> shift) * 3;
        HIP_TRY(buf.rgb.ensure(n_bytes));
        mr_accum::launch_resolve(g_stream, result, width, height, shift, s, sc->d_gamma.as<float>(), buf.rgb.as<uint8_t>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out_rgb, buf.rgb.p, n_bytes, hipMemcpyDeviceToHost, g_stream));
    }
    HIP_TRY(hipStreamSynchronize(g_stream));
    return MR_OK;
}

}  // namespace
