// host_overlay_dev.h -- the debug-frustum overlay's device plumbing: building the scene's lists from the cameras left by
// the caller, a frame slot's device copy of them, and the launches of k_overlay and of the resolve that follows it.
#pragma once

namespace {

// A frame slot's device copy of the scene's overlay lists: ONE buffer filled with one asynchronous copy from a
// page-locked staging buffer on the slot's stream (behind the slot's earlier frames, in front of the next one),
// and the overlay kernel's scratch.
struct OverlayCopy {
    DevBuf lists, scratch;
    DevBuf apply_scratch;                // mr_overlay_apply's compact state and bidding words, per slot of the touched pixels
    size_t apply_slots = 0;              // the layout `apply_scratch` was last cleared for: number of slots ...
    uint64_t apply_serial = 0;           // ... of the lists with this ov_serial
    void *staging = nullptr;
    size_t staging_cap = 0;
    size_t off[6] = {};                  // byte offsets of z, targets, segments, tile mask (+ slot ids, touched pixels) in `lists`
    bool with_slots = false;             // `lists` also holds the slot lists of a split frame
    size_t state_entries = 0;            // entries of win / any in `scratch` (zero between frames)
    uint64_t serial = 0;                 // the scene's ov_serial this copy holds
    hipEvent_t copied = nullptr;         // the last copy out of the staging buffer

    template <class T> const T *list(int i) const { return reinterpret_cast<const T *>(static_cast<const char *>(lists.p) + off[i]); }
    void release()
    {
        lists.release(); scratch.release(); apply_scratch.release();
        apply_slots = 0; apply_serial = 0;
        if (staging) (void)hipHostFree(staging);
        if (copied) (void)hipEventDestroy(copied);
        staging = nullptr; staging_cap = 0; serial = 0; copied = nullptr;
    }
};

// the corners of a frustum's six faces (obj/frustums.py)
const int32_t FRUSTUM_FACES[24] = { 2, 4, 5, 3,  0, 1, 7, 6,  0, 2, 3, 1,  5, 4, 6, 7,  3, 5, 7, 1,  4, 2, 0, 6 };

// Marks, in the scene's segment list, the segments whose targets would overfill k_overlay's LDS table: the kernel replays
// them with its bidding words in global memory (kernels_overlay.h, OVERLAY_SEG_GLOBAL).  For every list the scene takes,
// from the cameras or from mr_scene_set_overlay.
void mark_global_segments(mr_scene *sc)
{
    mr_host::mark_overlay_segments(sc->ov_target.data(), sc->ov_z.size(), sc->ov_seg.data(), sc->ov_seg.size() / 2, mr::OVERLAY_LDS_POINTS,
                                   mr::OVERLAY_LDS_TARGETS, mr::OVERLAY_SEG_GLOBAL, sc->ov_count_work);
}

// Builds the overlay's lists from the cameras mr_scene_set_overlay_cameras left (host_overlay.h: clipping, projection,
// DDA, dashes, index wrapping -- obj/frustums.py:61-103, obj/line.py:6-16), if that has not happened yet.
void realize_overlay(mr_scene *sc)
{
    mr_scene::OvPending &p = sc->ov_pending;
    if (!p.set) return;
    p.set = false;
    static thread_local mr_host::OverlayLists lists;            // (its vectors keep their capacity from call to call)
    lists.seg_first.clear(); lists.seg_count.clear(); lists.z.clear();
    mr_host::build_overlay_lists(p.corners, FRUSTUM_FACES, p.planes, p.mvp, p.viewport, p.near_, p.far_, p.inside != 0, p.height, p.width, 13,
                                 lists, false, true);
    sc->ov_points = sc->ov_segments = 0;
    sc->ov_serial += 1;
    if (lists.z.empty()) return;
    const size_t np = lists.z.size();
    sc->ov_target.resize((size_t)mr::OVERLAY_TARGETS * np);
    for (int k = 0; k < mr::OVERLAY_TARGETS; ++k) std::copy(lists.target[k].begin(), lists.target[k].end(), sc->ov_target.begin() + (size_t)k * np);
    sc->ov_z.assign(lists.z.begin(), lists.z.end());
    sc->ov_seg.resize(2 * lists.seg_first.size());
    for (size_t i = 0; i < lists.seg_first.size(); ++i) { sc->ov_seg[2 * i] = lists.seg_first[i]; sc->ov_seg[2 * i + 1] = lists.seg_count[i]; }
    mark_global_segments(sc);
    sc->ov_tile_mask.swap(lists.tile_mask);
    sc->ov_height = p.height; sc->ov_width = p.width;
    sc->ov_points = (int32_t)np; sc->ov_segments = (int32_t)lists.seg_first.size();
}

// The lists' targets as slots of the list of touched pixels (host_overlay.h, build_overlay_slots), if the lists have
// changed since they were last built.
void ensure_overlay_slots(mr_scene *sc)
{
    if (sc->ov_slots_serial == sc->ov_serial) return;
    mr_host::build_overlay_slots(sc->ov_target.data(), (size_t)sc->ov_points, (size_t)sc->ov_height * sc->ov_width, sc->ov_slot_work,
                                 sc->ov_slot_of, sc->ov_touched);
    sc->ov_slots_serial = sc->ov_serial;
}

// Brings the slot's device copy of the overlay lists up to date: packed into the slot's page-locked staging buffer
// and copied with ONE asynchronous copy on the slot's stream (behind the slot's earlier frames, which read the old
// lists, and in front of the frame that needs the new ones).  The staging buffer is rewritten only after the copy
// that last read it has completed (an event; mr_render and mr_render_wait have drained the stream long before).
int sync_slot_overlay(mr_scene *sc, OverlayCopy &ov, hipStream_t stream, bool with_slots)
{
    if (sc->ov_points == 0 || (ov.serial == sc->ov_serial && (ov.with_slots || !with_slots))) return MR_OK;
    if (with_slots) ensure_overlay_slots(sc);
    const int n_src = with_slots ? 6 : 4;
    const void *src[6] = { sc->ov_z.data(), sc->ov_target.data(), sc->ov_seg.data(), sc->ov_tile_mask.data(),
                           sc->ov_slot_of.data(), sc->ov_touched.data() };
    const size_t bytes[6] = { sc->ov_z.size() * 8, sc->ov_target.size() * 4, sc->ov_seg.size() * 4, sc->ov_tile_mask.size(),
                              with_slots ? sc->ov_slot_of.size() * 4 : 0, with_slots ? sc->ov_touched.size() * 4 : 0 };
    size_t total = 0;
    for (int i = 0; i < 6; ++i) { ov.off[i] = total; total += (bytes[i] + 15) & ~(size_t)15; }
    // scratch: win and any (one word per pixel of the frame each, zero between segments and frames)
    const size_t entries = (size_t)sc->ov_height * sc->ov_width;
    const size_t scratch = entries * 8 + (size_t)sc->ov_points + 16;
    if (total > ov.staging_cap || total > ov.lists.cap || scratch > ov.scratch.cap)
        HIP_TRY(hipStreamSynchronize(stream));          // (growing frees the old buffers: nothing may still use them)
    if (total > ov.staging_cap) {
        if (ov.staging) (void)hipHostFree(ov.staging);
        ov.staging = nullptr; ov.staging_cap = 0;
        HIP_TRY(hipHostMalloc(&ov.staging, total + total / 2, hipHostMallocDefault));
        ov.staging_cap = total + total / 2;
    }
    if (!ov.copied) HIP_TRY(hipEventCreateWithFlags(&ov.copied, hipEventDisableTiming));
    else HIP_TRY(hipEventSynchronize(ov.copied));
    for (int i = 0; i < n_src; ++i) std::memcpy(static_cast<char *>(ov.staging) + ov.off[i], src[i], bytes[i]);
    HIP_TRY(ov.lists.ensure(total));
    // the kernel leaves win / any zeroed; a new layout starts so
    if (int rc = ensure_cleared(ov.scratch, scratch, stream, 0, ov.state_entries != entries)) return rc;
    ov.state_entries = entries;
    HIP_TRY(hipMemcpyAsync(ov.lists.p, ov.staging, total, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(ov.copied, stream));
    ov.serial = sc->ov_serial;
    ov.with_slots = with_slots;
    return MR_OK;
}

// k_overlay's lists and bidding words: the targets as pixels of the frame, or (`slots`, an assembled frame) as slots of
// the list of touched pixels; `state` holds win and any, n_state words each (zero between frames), and keep behind them.
mr::OverlayArgs overlay_args(const mr_scene *sc, const OverlayCopy &ov, bool slots, uint32_t *state, size_t n_state)
{
    mr::OverlayArgs oa;
    oa.z = ov.list<double>(0); oa.idx = ov.list<int32_t>(slots ? 4 : 1); oa.seg = ov.list<int32_t>(2);
    oa.pixel_of = slots ? ov.list<int32_t>(5) : nullptr;
    oa.n_points = sc->ov_points; oa.n_segments = sc->ov_segments;
    oa.win = state; oa.any = state + n_state; oa.keep = reinterpret_cast<uint8_t *>(oa.any + n_state);
    oa.gamma_lut = sc->d_gamma.as<float>();
    return oa;
}

// The overlay kernel on a slot's own z-buffer and float frame (so the debug taps show them after the overlay, like
// upstream's), finalising the touched pixels into d_out.
void launch_overlay(mr_scene *sc, const OverlayCopy &ov, double *zbuf, float *frame, uint8_t *d_out, int width, int height,
                    int system, hipStream_t stream)
{
    mr::OverlayArgs oa = overlay_args(sc, ov, false, ov.scratch.as<uint32_t>(), ov.state_entries);
    oa.st_z = zbuf; oa.st_f = frame; oa.out = d_out; oa.out_width = width; oa.out_height = height;
    hipLaunchKernelGGL(mr::k_overlay, dim3(1), dim3(mr::OVERLAY_BLOCK), 0, stream, oa, (double)system);
}

// The output of a supersampled frame that k_tile did not finalise in full, after the overlay (which, on such a frame,
// blends into the float frame only): the output pixels of the touched samples (k_resolve_touched), or with
// MR_RESOLVE_PATH=separate every output pixel of the band (k_resolve_full).  Nothing to do for other frames.
void launch_resolve(mr_scene *sc, const OverlayCopy &ov, const float *frame, const mr_frame_desc &fr, int ss_mode,
                    bool overlay_drawn, uint8_t *d_out, hipStream_t stream)
{
    const int shift = ss_mode & mr::SS_SHIFT_MASK;
    if (!shift) return;
    const int band_y0 = fr.height - fr.row_end, band_y1 = fr.height - fr.row_begin;
    if (ss_mode & mr::SS_SEPARATE) {
        const long long n = (long long)(fr.width >> shift) * ((band_y1 - band_y0) >> shift);
        hipLaunchKernelGGL(mr::k_resolve_full, dim3(blocks_for(n, 256)), dim3(256), 0, stream, frame, fr.width,
                           band_y0, band_y1, shift, sc->d_gamma.as<float>(), d_out);
    } else if (overlay_drawn && !sc->ov_touched.empty()) {
        const int n_slots = (int)sc->ov_touched.size();
        hipLaunchKernelGGL(mr::k_resolve_touched, dim3(blocks_for(n_slots, 256)), dim3(256), 0, stream,
                           ov.list<int32_t>(5), n_slots, frame, fr.width, band_y1, shift, sc->d_gamma.as<float>(), d_out);
    }
}

}  // namespace
