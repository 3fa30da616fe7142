// host_tonemap.h -- tone mapping, an exposure metered from a luminance histogram and a tone curve (tonemap_def.h has the
// definition): the scene's description as the kernels take it, the layout of a frame slot's words (histogram, exposure
// cell, slab), the scene's previous exposure and when a frame's e becomes it (the hand-over rule of host_taa.h), the three
// launches behind a frame's bloom and in front of its overlay, the same arithmetic on the host, bit for bit
// (host_tone_map: plain C++, no device), and mr_debug_tone_map_post, the kernels on a frame a caller supplies.  The bytes
// of such a frame are the full resolve of its float frame (host_frame.h, launch_post_resolve).
#pragma once

namespace {

// The description as the kernels and the mirror take it: every float32 it uses, checked.
int tone_params(const mr_tone_map_desc *d, mr::ToneParams &p)
{
    p = mr::ToneParams();
    mr::ToneMeter &m = p.meter;
    float white;
    if (d->op < mr::TONE_LINEAR || d->op > mr::TONE_ACES) return fail(MR_E_INVALID, "tone mapping: the operator must be 0 (linear), 1 (reinhard) or 2 (aces)");
    if (d->fixed != 0 && d->fixed != 1) return fail(MR_E_INVALID, "tone mapping: fixed is 0 or 1");
    if (!positive_f32(d->exposure, p.exposure)) return fail(MR_E_INVALID, "tone mapping: exposure must be finite and > 0 as float32");
    if (!positive_f32(d->key, m.key)) return fail(MR_E_INVALID, "tone mapping: key must be finite and > 0 as float32");
    if (!positive_f32(d->white, white)) return fail(MR_E_INVALID, "tone mapping: white must be finite and > 0 as float32");
    if (!positive_f32(d->min_exposure, m.min_exposure) || !positive_f32(d->max_exposure, m.max_exposure))
        return fail(MR_E_INVALID, "tone mapping: min_exposure and max_exposure must be finite and > 0 as float32");
    if (m.min_exposure > m.max_exposure) return fail(MR_E_INVALID, "tone mapping: min_exposure must not exceed max_exposure");
    if (!positive_f32(d->speed, m.speed) || m.speed > 1.0f) return fail(MR_E_INVALID, "tone mapping: speed must lie in (0, 1] as float32");
    if (d->low_pm < 0 || d->low_pm >= d->high_pm || d->high_pm > 1000)
        return fail(MR_E_INVALID, "tone mapping: the trims must satisfy 0 <= low_pm < high_pm <= 1000");
    for (int f = 0; f < mr::TONE_BINS; ++f) {
        const float v = d->exp2[f], before = f ? d->exp2[f - 1] : 1.0f;
        if (!(f ? v > before : v == 1.0f) || !(v < 2.0f))
            return fail(MR_E_INVALID, "tone mapping: exp2 must be float32(2^(f/256)): exp2[0] == 1, strictly increasing, < 2");
        m.exp2[f] = v;
    }
    p.op = d->op; p.fixed = d->fixed;
    p.white2 = white * white;
    m.low_pm = d->low_pm; m.high_pm = d->high_pm;
    return MR_OK;
}

// A frame slot's words for the pass, one buffer: the 256 counts, the exposure cell, and behind them the slab k_lum_hist
// writes and k_exposure sums, `rows` x 256 (every part 256-byte aligned).
constexpr size_t TONE_SLOT_HIST = 0, TONE_SLOT_CELL = 256, TONE_SLOT_SLAB = 320;
inline size_t tone_slot_bytes(unsigned rows) { return (TONE_SLOT_SLAB + (size_t)rows * mr::TONE_BINS) * sizeof(uint32_t); }

// the previous exposure is forgotten: the next frame has none, and a frame still in flight hands nothing over
void tone_forget(mr_scene *sc)
{
    sc->tone.valid = false;
    sc->tone.epoch += 1;
}

void tone_release(mr_scene *sc)
{
    sc->tone.d_state.release();
    release_pass(sc->tone);
}

// The launches on one stream: k_lum_hist and k_exposure where the exposure is metered, k_tone_apply; `between(mark)` is
// called with 1 behind k_lum_hist and 2 behind k_exposure (both in front of k_tone_apply where nothing is metered).
// `words` is a slot's buffer (tone_slot_bytes(grid)); e_prev: the scene's previous exposure or nullptr; e_next: its next
// state cell or nullptr.
template <class Between>
int tone_chain(hipStream_t stream, float *frame, size_t n_samples, uint32_t *words, const mr::ToneParams &p, unsigned grid, int form,
               const float *e_prev, float *e_next, Between &&between)
{
    float *cell = reinterpret_cast<float *>(words + TONE_SLOT_CELL);
    if (!p.fixed) mr_tonemap::launch_hist(stream, frame, n_samples, words + TONE_SLOT_SLAB, grid, form);
    if (int rc = between(1)) return rc;
    if (!p.fixed) mr_tonemap::launch_exposure(stream, words + TONE_SLOT_SLAB, grid, p.meter, e_prev, words + TONE_SLOT_HIST, cell, e_next);
    if (int rc = between(2)) return rc;
    mr_tonemap::launch_apply(stream, frame, n_samples * 3, p.op, p.fixed ? nullptr : cell, p.exposure, p.white2);
    return MR_OK;
}

// the grid of k_lum_hist for a frame: what grow_slot sizes the slab for and launch_tone_map launches
inline unsigned tone_grid(int width, int height, const Env &env) { return mr_tonemap::hist_grid((size_t)width * height, (unsigned)env.tone_grid); }

// The pass on a frame's own float frame and its slot's words, on the frame's stream, marked for mr_debug_tone_map_times:
// round k_lum_hist, k_exposure and k_tone_apply.  `p` is the copy the frame's plan took.  An adaptive frame reads the
// scene's previous exposure where there is one and writes the state cell the scene is not reading.
int launch_tone_map(mr_scene *sc, hipStream_t stream, float *frame, uint32_t *words, int width, int height, const mr::ToneParams &p, const Env &env)
{
    mr_scene::Tone &a = sc->tone;
    const float *e_prev = nullptr;
    float *e_next = nullptr;
    if (p.adaptive()) {
        HIP_TRY(a.d_state.ensure(2 * sizeof(float)));
        if (a.valid) e_prev = a.d_state.as<float>() + a.cur;
        e_next = a.d_state.as<float>() + (a.cur ^ 1);
    }
    const unsigned grid = tone_grid(width, height, env);
    a.last_grid = p.fixed ? 0 : (int32_t)grid;
    return marked_launch(a, stream, width, height, [&]() -> int {
        return tone_chain(stream, frame, (size_t)width * height, words, p, grid, env.tone_form, e_prev, e_next,
                          [&](int mark) { return a.marks.record(mark, stream); });
    });
}

// An adaptive frame has been enqueued on `fs`: its exposure waits for the frame's verdict.
void tone_enqueued(mr_scene *sc, const FrameSlot *fs)
{
    mr_scene::Tone &a = sc->tone;
    a.pending = true; a.pending_slot = fs;
    a.pending_epoch = a.epoch;
}

// The verdict of the frame on `fs` is in (mr_render, mr_render_wait): a frame that was complete hands its exposure over,
// one that overflowed a work list (or failed) leaves the scene the exposure it read.
void tone_settle(mr_scene *sc, const FrameSlot *fs, bool complete)
{
    mr_scene::Tone &a = sc->tone;
    if (!a.pending || a.pending_slot != fs) return;
    a.pending = false; a.pending_slot = nullptr;
    if (!complete || a.pending_epoch != a.epoch) return;
    a.cur ^= 1;
    a.valid = true;
    a.adopted += 1;
}

// what the scene keeps from frame to frame, settled together: the history of the temporal anti-aliasing and the exposure
void frame_settled(mr_scene *sc, const FrameSlot *fs, bool complete)
{
    taa_settle(sc, fs, complete);
    tone_settle(sc, fs, complete);
}

int tone_checked(const char *entry, const float *frame, int32_t height, int32_t width, const mr_tone_map_desc *d, int32_t has_prev, float e_prev,
                 mr::ToneParams &p)
{
    if (!frame || !d) return fail(MR_E_INVALID, std::string(entry) + ": NULL argument");
    if (!frame_size_ok(height, width)) return fail(MR_E_INVALID, std::string(entry) + ": resolution out of range");
    if (int rc = tone_params(d, p)) return rc;
    if (has_prev && !(std::isfinite(e_prev) && e_prev > 0.0f)) return fail(MR_E_INVALID, std::string(entry) + ": a previous exposure must be finite and > 0");
    return MR_OK;
}

// The definition on the host.
int host_tone_map(const float *frame, int32_t height, int32_t width, const mr_tone_map_desc *d, int32_t has_prev, float e_prev, float *out,
                  uint32_t *out_hist, float *out_exposure)
{
    if (!out) return fail(MR_E_INVALID, "mr_host_tone_map: NULL argument");
    mr::ToneParams p;
    if (int rc = tone_checked("mr_host_tone_map", frame, height, width, d, has_prev, e_prev, p)) return rc;
    const size_t n = (size_t)height * width;
    uint32_t hist[mr::TONE_BINS] = {};
    float e = p.exposure;
    if (!p.fixed) {
        for (size_t i = 0; i < n; ++i) hist[mr::tone_bin(frame[3 * i], frame[3 * i + 1], frame[3 * i + 2])] += 1;
        hist[0] = 0;
        int64_t total = 0, c = 0, s = 0, m = 0;
        for (uint32_t v : hist) total += v;
        const int64_t lo = total * p.meter.low_pm / 1000, hi = total * p.meter.high_pm / 1000;
        for (int i = 0; i < mr::TONE_BINS; ++i) {
            const int64_t u = mr::tone_kept(c, hist[i], lo, hi);
            s += u * mr::tone_centre(i);
            m += u;
            c += hist[i];
        }
        e = mr::tone_exposure(s, m, p.meter, has_prev != 0, e_prev);
    }
    for (size_t i = 0; i < n * 3; ++i)
        out[i] = p.op == mr::TONE_ACES       ? mr::tone_curve<mr::TONE_ACES>(frame[i], e, p.white2)
                 : p.op == mr::TONE_REINHARD ? mr::tone_curve<mr::TONE_REINHARD>(frame[i], e, p.white2)
                                             : mr::tone_curve<mr::TONE_LINEAR>(frame[i], e, p.white2);
    if (out_hist) std::memcpy(out_hist, hist, sizeof hist);
    if (out_exposure) *out_exposure = e;
    return MR_OK;
}

constexpr size_t TONE_GUARD = 256;                       // bytes of sentinel in front of and behind each device buffer
constexpr unsigned char TONE_SENTINEL = 0xa5;

// mr_debug_tone_map_post: the kernels on the caller's frame through the library's own launches, the grid cap and the form
// of k_lum_hist arguments and not the environment's.  The frame, the slot's words and the two state cells lie between
// guards of sentinel bytes on the device, and the words are sentinel before the kernels run -- the slab gets no memset in
// a frame either; a guard byte that changed is MR_E_DEVICE.  out_ms (may be NULL) receives the three kernels' device times
// between events of the entry's own.  Every refusal comes before any device call; the scene's
// slots, its previous exposure and what mr_debug_tone_map reports stay as they were.
int debug_tone_map_post(mr_scene *sc, const float *frame, int32_t height, int32_t width, const mr_tone_map_desc *d, int32_t has_prev, float e_prev,
                        int32_t grid_cap, int32_t form, float *out_frame, uint32_t *out_hist, float *out_exposure, float *out_ms)
{
    if (!sc || !out_frame || !out_hist || !out_exposure) return fail(MR_E_INVALID, "mr_debug_tone_map_post: NULL argument");
    mr::ToneParams p;
    if (int rc = tone_checked("mr_debug_tone_map_post", frame, height, width, d, has_prev, e_prev, p)) return rc;
    if (grid_cap < 0 || grid_cap > (int32_t)mr::TONE_MAX_BLOCKS) return fail(MR_E_INVALID, "mr_debug_tone_map_post: the grid cap of k_lum_hist is 0 (the default) or 1 .. 1024");
    if (form < -1 || form > 1) return fail(MR_E_INVALID, "mr_debug_tone_map_post: the form of k_lum_hist is 0, 1 or -1 (the default)");
    if (int rc = tonemap_linked()) return rc;
    if (int rc = ensure_init()) return rc;
    const Env env = read_env();
    const size_t n = (size_t)height * width, G = TONE_GUARD, f_bytes = n * 3 * sizeof(float);
    const unsigned grid = mr_tonemap::hist_grid(n, grid_cap ? (unsigned)grid_cap : (unsigned)env.tone_grid);
    const size_t w_bytes = tone_slot_bytes(grid), s_bytes = 2 * sizeof(float);
    std::vector<unsigned char> guards(6 * G);
    struct { DevBuf f, w, s; } buf;
    Drained drained{ &buf.f, &buf.w, &buf.s };
    HIP_TRY(buf.f.ensure(f_bytes + 2 * G));
    HIP_TRY(buf.w.ensure(w_bytes + 2 * G));
    HIP_TRY(buf.s.ensure(s_bytes + 2 * G));
    float *d_frame = reinterpret_cast<float *>(buf.f.as<char>() + G), *d_state = reinterpret_cast<float *>(buf.s.as<char>() + G);
    uint32_t *d_words = reinterpret_cast<uint32_t *>(buf.w.as<char>() + G);
    HIP_TRY(hipMemsetAsync(buf.f.p, TONE_SENTINEL, f_bytes + 2 * G, g_stream));
    HIP_TRY(hipMemsetAsync(buf.w.p, TONE_SENTINEL, w_bytes + 2 * G, g_stream));
    HIP_TRY(hipMemsetAsync(buf.s.p, TONE_SENTINEL, s_bytes + 2 * G, g_stream));
    HIP_TRY(hipMemcpyAsync(d_frame, frame, f_bytes, hipMemcpyHostToDevice, g_stream));
    if (has_prev) HIP_TRY(hipMemcpyAsync(d_state, &e_prev, sizeof(float), hipMemcpyHostToDevice, g_stream));
    Marks<4> marks;                                          // (the entry's own, where the caller asks for times: the scene's stay as they were)
    struct Release { Marks<4> &m; ~Release() { m.release(); } } release{ marks };
    if (out_ms) {
        if (int rc = marks.create()) return rc;
        if (int rc = marks.record(0, g_stream)) return rc;
    }
    if (int rc = tone_chain(g_stream, d_frame, n, d_words, p, grid, form < 0 ? env.tone_form : form, has_prev ? d_state : nullptr, d_state + 1,
                            [&](int mark) { return out_ms ? marks.record(mark, g_stream) : (int)MR_OK; }))
        return rc;
    if (out_ms)
        if (int rc = marks.record(3, g_stream)) return rc;
    HIP_TRY(hipGetLastError());
    const struct { const DevBuf &b; size_t bytes; } guarded[] = { { buf.f, f_bytes }, { buf.w, w_bytes }, { buf.s, s_bytes } };
    for (int k = 0; k < 3; ++k) {
        HIP_TRY(hipMemcpyAsync(guards.data() + 2 * k * G, guarded[k].b.p, G, hipMemcpyDeviceToHost, g_stream));
        HIP_TRY(hipMemcpyAsync(guards.data() + (2 * k + 1) * G, guarded[k].b.as<char>() + G + guarded[k].bytes, G, hipMemcpyDeviceToHost, g_stream));
    }
    HIP_TRY(hipMemcpyAsync(out_frame, d_frame, f_bytes, hipMemcpyDeviceToHost, g_stream));
    if (p.fixed) {
        std::memset(out_hist, 0, mr::TONE_BINS * sizeof(uint32_t));
        out_exposure[0] = out_exposure[1] = p.exposure;
    } else {
        HIP_TRY(hipMemcpyAsync(out_hist, d_words + TONE_SLOT_HIST, mr::TONE_BINS * sizeof(uint32_t), hipMemcpyDeviceToHost, g_stream));
        HIP_TRY(hipMemcpyAsync(out_exposure, d_words + TONE_SLOT_CELL, sizeof(float), hipMemcpyDeviceToHost, g_stream));
        HIP_TRY(hipMemcpyAsync(out_exposure + 1, d_state + 1, sizeof(float), hipMemcpyDeviceToHost, g_stream));
    }
    HIP_TRY(hipStreamSynchronize(g_stream));
    for (int k = 0; out_ms && k < 3; ++k)
        if (int rc = marks.elapsed(k, k + 1, out_ms + k)) return rc;
    int touched = 0;
    for (unsigned char g : guards) touched += g != TONE_SENTINEL;
    if (touched)
        return fail(MR_E_DEVICE, "mr_debug_tone_map_post: " + std::to_string(touched) + " guard bytes round the frame, the slot's words and the state cells changed: a kernel wrote out of bounds");
    return MR_OK;
}

}  // namespace
