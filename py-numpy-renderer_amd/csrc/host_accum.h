// host_accum.h -- the accumulation: sub-frames rendered like mr_render's on the library's stream, their float frames
// summed with weights into a buffer of the scene's (kernels_accum.h), the sum finalised when asked for; and the same
// arithmetic on the host, bit for bit (host_accum: plain C++, no device).
//
//   A_0 = w_0 * F_0,   A_k = A_{k-1} + (w_k * F_k)
//   M = block mean of A (the order of ss_block_mean),  R = min(M * scale, 1),  out = uint8(R ** 0.8 * 255), rows flipped
//
// F_k is what mr_read_frame_f32 would hand out after sub-frame k: after the overlay, after the sum over the lights,
// on the sample grid.
#pragma once

namespace {

inline int accum_linked()
{
    return linked("this library was linked without accum.hip: no accumulation kernels (build it with __graft_entry__.build())",
                  &mr_accum::launch_add, &mr_accum::launch_resolve);
}

void accum_release(mr_scene::Accum &a)
{
    a.d_acc.release();
    release_pass(a);
}

// One sub-frame: rendered on the library's stream and its slot with the float frame kept (no bytes leave the device),
// again after an overflow like mr_render's frames, and added only once its work lists are known to have held.  The add
// kernel is not waited for: the host prepares the next sub-frame beside it, whose kernels follow it in stream order.
int accum_add(mr_scene *sc, const mr_frame_desc *fr, double weight)
{
    int rc = validate_frame(sc, fr);
    if (rc) return rc;
    if (is_partial(fr)) return fail(MR_E_INVALID, "an accumulation takes whole frames (no row band, no stripes)");
    if (fr->flags & MR_FRAME_FACE_STATUS) return fail(MR_E_INVALID, "MR_FRAME_FACE_STATUS is not available for the sub-frames of an accumulation");
    if (sc->motion.on) return fail(MR_E_INVALID, "motion blur is not available for the sub-frames of an accumulation: the sum is the other way to blur motion");
    if (sc->taa.on) return fail(MR_E_INVALID, "temporal anti-aliasing is not available for the sub-frames of an accumulation: the sum is the other way to spread samples over frames");
    if (sc->layers.on) return fail(MR_E_INVALID, "data layers are not available for the sub-frames of an accumulation: a sum of frames has no one winner a sample");
    if (sc->tone.on && sc->tone.params.adaptive())
        return fail(MR_E_INVALID, "adaptive tone mapping (speed < 1) is not available for the sub-frames of an accumulation: they have no previous frame (speed = 1 or a fixed exposure is)");
    float w;
    if (!positive_f32(weight, w)) return fail(MR_E_INVALID, "a sub-frame's weight must be finite and > 0 as float32");
    if ((rc = accum_linked())) return rc;
    mr_scene::Accum &a = sc->accum;
    const int32_t ss_flags = fr->flags & (MR_FRAME_SUPERSAMPLE2 | MR_FRAME_SUPERSAMPLE4);
    if (a.count > 0 && (fr->width != a.width || fr->height != a.height || ss_flags != a.ss_flags))
        return fail(MR_E_INVALID, "the sub-frames of an accumulation share one resolution and one supersample factor: "
                                  "mr_accum_begin starts another");
    if ((rc = ensure_init())) return rc;
    FrameSlot *fs = slot_for(sc, g_stream);
    if (!fs) return fail(MR_E_DEVICE, "out of frame slots");
    mr_frame_desc kept = *fr;
    kept.flags |= MR_FRAME_KEEP_FLOAT;
    HIP_TRY(fs->d_out.ensure(out_bytes(&kept)));
    rc = MR_E_OVERFLOW;
    for (int attempt = 0; attempt < 6 && rc == MR_E_OVERFLOW; ++attempt) {
        if (attempt > 0) a.rerendered += 1;            // work lists were grown: render the sub-frame again
        if ((rc = enqueue_frame(sc, fs, &kept, fs->d_out.as<uint8_t>(), true))) return rc;
        if ((rc = finish_overlay(sc, fs, fs->d_out.as<uint8_t>()))) return rc;
        if ((rc = fetch_counters(fs, false))) return rc;
        HIP_TRY(hipStreamSynchronize(g_stream));
        rc = collect(sc, fs, false);
        if (rc != MR_OK && rc != MR_E_OVERFLOW) return rc;
    }
    if (rc != MR_OK) return fail(MR_E_OVERFLOW, "work lists kept overflowing");
    const size_t n_floats = (size_t)kept.width * kept.height * 3;
    if (a.count == 0) {                                // (the stream is idle: growing the buffer frees nothing in use)
        HIP_TRY(a.d_acc.ensure(n_floats * sizeof(float)));
        a.width = kept.width; a.height = kept.height; a.ss_flags = ss_flags;
    }
    if ((rc = a.marks.create())) return rc;
    if ((rc = a.marks.record(0, g_stream))) return rc;
    mr_accum::launch_add(g_stream, fs->d_frame.as<float>(), a.d_acc.as<float>(), n_floats, w, a.count == 0 ? 1 : 0);
    if ((rc = a.marks.record(1, g_stream))) return rc;
    HIP_TRY(hipGetLastError());
    a.add_marked = true;
    a.count += 1;
    return MR_OK;
}

// The sum as it stands, finalised into the slot's uint8 rows and copied to the host; the sum itself stays, so adds may
// follow.
int accum_resolve(mr_scene *sc, double scale, uint8_t *out_rgb)
{
    mr_scene::Accum &a = sc->accum;
    if (a.count == 0) return fail(MR_E_INVALID, "nothing accumulated yet");
    float s;
    if (!positive_f32(scale, s)) return fail(MR_E_INVALID, "the scale must be finite and > 0 as float32");
    if (int rc = accum_linked()) return rc;
    FrameSlot *fs = slot_for(sc, g_stream);
    if (!fs) return fail(MR_E_DEVICE, "out of frame slots");
    const int shift = (a.ss_flags & MR_FRAME_SUPERSAMPLE4) ? 2 : (a.ss_flags & MR_FRAME_SUPERSAMPLE2) ? 1 : 0;
    const long long n_px = (long long)(a.width >> shift) * (a.height >> shift);
    HIP_TRY(fs->d_out.ensure((size_t)n_px * 3));
    if (int rc = a.marks.record(2, g_stream)) return rc;
    mr_accum::launch_resolve(g_stream, a.d_acc.as<float>(), a.width, a.height, shift, s, sc->d_gamma.as<float>(), fs->d_out.as<uint8_t>());
    if (int rc = a.marks.record(3, g_stream)) return rc;
    HIP_TRY(hipGetLastError());
    a.resolve_marked = true;
    HIP_TRY(hipMemcpyAsync(out_rgb, fs->d_out.p, (size_t)n_px * 3, hipMemcpyDeviceToHost, g_stream));
    HIP_TRY(hipStreamSynchronize(g_stream));
    return MR_OK;
}

// ss_block_mean (kernels_tile.h) on the host: the block whose bottom-left sample is rgb[0], rows `row` floats apart
inline void host_block_mean(const float *rgb, size_t row, int shift, float m[3])
{
    const int s = 1 << shift;
    float acc[3] = { 0.f, 0.f, 0.f };
    for (int j = 0; j < s; ++j)
        for (int i = 0; i < s; ++i)
            for (int c = 0; c < 3; ++c) acc[c] += rgb[(size_t)j * row + (size_t)i * 3 + c];
    const float inv = 1.0f / (float)(s * s);
    for (int c = 0; c < 3; ++c) m[c] = acc[c] * inv;
}

// The definition on the host: n frames (n, height, width, 3) and their weights -> the sum (out_acc, may be NULL) and
// its finalised bytes (out_rgb, (height >> shift, width >> shift, 3), row 0 = top; may be NULL).
int host_accum(const float *frames, const double *weights, int32_t n, int32_t height, int32_t width, int32_t shift, double scale,
               float *out_acc, uint8_t *out_rgb)
{
    if (!frames || !weights || n < 1 || height <= 0 || width <= 0) return fail(MR_E_INVALID, "mr_host_accum: bad argument");
    if (shift < 0 || shift > 2) return fail(MR_E_INVALID, "mr_host_accum: shift is 0, 1 or 2");
    if (height % (1 << shift) || width % (1 << shift)) return fail(MR_E_INVALID, "mr_host_accum: height and width must be multiples of 1 << shift");
    float s;
    if (!positive_f32(scale, s)) return fail(MR_E_INVALID, "the scale must be finite and > 0 as float32");
    std::vector<float> w((size_t)n);
    for (int32_t k = 0; k < n; ++k)
        if (!positive_f32(weights[k], w[k])) return fail(MR_E_INVALID, "a sub-frame's weight must be finite and > 0 as float32");
    const size_t n_floats = (size_t)height * width * 3;
    std::vector<float> own;
    float *acc = out_acc;
    if (!acc) { own.resize(n_floats); acc = own.data(); }
    for (int32_t k = 0; k < n; ++k) {
        const float *f = frames + (size_t)k * n_floats;
        for (size_t i = 0; i < n_floats; ++i) {
            const float p = w[k] * f[i];
            acc[i] = k == 0 ? p : acc[i] + p;
        }
    }
    if (!out_rgb) return MR_OK;
    const int ow = width >> shift, oh = height >> shift;
    for (int orow = 0; orow < oh; ++orow)
        for (int ox = 0; ox < ow; ++ox) {
            const int py = height - ((orow + 1) << shift), px = ox << shift;
            float m[3];
            host_block_mean(acc + ((size_t)py * width + px) * 3, (size_t)width * 3, shift, m);
            for (int c = 0; c < 3; ++c) {
                const float r = m[c] * s;
                out_rgb[((size_t)orow * ow + ox) * 3 + c] = (uint8_t)(powf(r < 1.0f ? r : 1.0f, 0.8f) * 255.0f);
            }
        }
    return MR_OK;
}

}  // namespace
