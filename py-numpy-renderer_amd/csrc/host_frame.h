// host_frame.h -- a frame: the slot that holds everything one in-flight frame writes, the frame's constants, and
// enqueue_frame(), which puts the frame on the slot's stream as a sequence of steps.
#pragma once

namespace {

// Event marks of one frame:
//   0 start | 1 after k_vertex_mfma (optional) | 2 after k_setup | 3 after k_bin_work | 4 after k_tile | 5 device->host copy
constexpr int EVENT_RING = 512, N_MARKS = 6;     // (bench.py marks one frame in 13: ~40 marked frames per stream to average over)

// Everything one in-flight frame writes.
struct FrameSlot {
    hipStream_t stream = nullptr;                 // the stream this slot serves
    int id = 0;                                   // its index among the scene's slots
    DevBuf d_vout, d_vclip, d_tris, d_clips, d_status, d_count_list, d_quads, d_sil, d_counters;
    DevBuf d_bin_count, d_items[mr::BIN_CLASSES], d_quad_bound, d_work, d_tile_stats, d_hist, d_split;
    DevBuf d_z, d_winner, d_stencil, d_frame, d_out;
    DevBuf d_frame_b;                             // the float frame k_taa, k_dof or k_mblur writes; then swapped with d_frame, which stays THE float frame
    DevBuf d_bloom;                               // the pyramid of a frame with bloom: levels 1 .. L, three floats a sample (host_bloom.h, bloom_pyramid)
    DevBuf d_shafts;                              // S and R of a frame with light shafts, 16 bytes a sample (host_shafts.h, shafts_level)
    DevBuf d_tone;                                // the words of a frame with tone mapping: histogram, exposure cell, slab (host_tonemap.h, tone_slot_bytes)
    int last_tone = 0;                            // the last frame ran the tone mapping: 1 metered, 2 with a fixed exposure ...
    float last_tone_exposure = 0.f;               // ... which was this
    MotionSlot motion;                            // the velocity buffer and the tables of a frame with motion blur or temporal anti-aliasing (host_motion.h)
    MotionFacesSlot motion_faces;                 // the face records and the tables of its per-face pass (host_motion_faces.h)
    LayersSlot layers;                            // the data layers of a frame that computes some, one buffer a layer (host_layers.h)
    int last_layers = 0;                          // the mask of the layers the last frame computed: mr_read_layers has those to read
    bool last_motion = false;                     // the last frame ran k_velocity: mr_read_velocity has something to read
    DevBuf d_stencil_x[mr::MAX_LIGHTS - 1];       // stencil taps of lights 1.. of a frame with several lights
    static_assert(mr::MAX_LIGHTS == MR_MAX_LIGHTS, "the ABI's light count is the kernels'");
    int last_n_lights = 1;                        // lights of the last frame
    // capacities this slot's buffers were last bound with (the scene holds the current ones)
    uint32_t bin_cap[mr::BIN_CLASSES] = { 0, 0, 0 }, work_cap = 0, quad_cap = 0;
    int bins_zeroed_for = 0;

    mr::Counters *h_counters = nullptr;           // pinned: the last frame's counters, then (h_sticky) the slot's sticky record
    mr::Sticky *h_sticky = nullptr;
    hipEvent_t ev_ring[EVENT_RING][N_MARKS] = {};
    uint8_t ev_marks[EVENT_RING] = {};            // 0: the frame recorded no events, 1: frame + tile kernel, 2: every stage
    hipEvent_t *ev = ev_ring[0];
    uint64_t frames_enqueued = 0;
    uint64_t last_serial = 0;                // the scene's frame serial when this slot last took a frame
    bool events_ok = false;
    OverlayCopy ov;                          // this slot's device copy of the scene's overlay lists

    mr_frame_desc last_frame = {};
    int last_n_tiles = 0;
    bool last_ordered = false;               // the last frame's tile kernel followed the order buffer (else row-major)
    bool last_full = false, last_split = false;   // the kernels the last frame launched (mr_debug_frame_path)
    bool overlay_deferred = false;           // the last enqueue_frame left the overlay to finish_overlay
    int last_ss_mode = 0;                    // FrameConst::ss_mode of the last frame (finish_overlay resolves after the overlay)
    bool last_post = false;                  // the last frame ran k_ao or k_dof: its bytes are the full resolve of the float frame
    bool have_frame = false, stats_reduced = false;
    bool last_copied = false;                // the last frame was followed by a timed device-to-host copy (mr_render, mr_render_async)

    void reset_caps() { bins_zeroed_for = 0; have_frame = false; }
    void release()
    {
        for (DevBuf *b : { &d_vout, &d_vclip, &d_count_list, &d_tris, &d_clips, &d_status, &d_quads, &d_sil, &d_counters,
                           &d_bin_count, &d_quad_bound, &d_work, &d_tile_stats, &d_hist, &d_split, &d_z, &d_winner, &d_stencil, &d_frame, &d_frame_b, &d_bloom, &d_shafts, &d_tone, &d_out })
            b->release();
        for (DevBuf &b : d_items) b.release();
        for (DevBuf &b : d_stencil_x) b.release();
        motion.release();
        motion_faces.release();
        layers.release();
        ov.release();
        if (events_ok) {
            for (auto &set : ev_ring) for (auto &e : set) (void)hipEventDestroy(e);
            (void)hipHostFree(h_counters);
            events_ok = false;
        }
    }
    // the counters are double-buffered by frame parity: a frame's tile kernel clears the next frame's
    mr::Counters *ctr(uint64_t frame) const { return d_counters.as<mr::Counters>() + (frame & 1); }
    // overflow verdicts of the frames before the last one (rast_types.h, Sticky): behind the two counter blocks
    mr::Sticky *sticky() const { return reinterpret_cast<mr::Sticky *>(d_counters.as<mr::Counters>() + 2); }
};

FrameSlot *slot_for(mr_scene *sc, hipStream_t stream)
{
    for (auto &s : sc->slots)
        if (s->stream == stream) return s.get();
    if ((int)sc->slots.size() >= MAX_SLOTS) return nullptr;
    sc->slots.emplace_back(new (std::nothrow) FrameSlot());
    if (!sc->slots.back()) { sc->slots.pop_back(); return nullptr; }
    sc->slots.back()->stream = stream;
    sc->slots.back()->id = (int)sc->slots.size() - 1;
    return sc->slots.back().get();
}

FrameSlot *last_slot(mr_scene *sc)
{
    if (!sc || !sc->last || !sc->last->have_frame) { fail(MR_E_INVALID, "nothing rendered yet"); return nullptr; }
    return sc->last;
}

// last_slot, for the entry points that read what only a frame rendered with `flag` has left
FrameSlot *last_slot_with(mr_scene *sc, int flag, const char *flag_name)
{
    FrameSlot *fs = last_slot(sc);
    if (fs && !(fs->last_frame.flags & flag)) { fail(MR_E_INVALID, std::string("the last frame was rendered without ") + flag_name); return nullptr; }
    return fs;
}

// One of the last frame's taps to the host: a buffer of `per_px` T per pixel that only a frame rendered with `flag` writes.
template <class T>
int read_tap(mr_scene *sc, int flag, const char *flag_name, DevBuf FrameSlot::*buf, T *out, int per_px, const char *what)
{
    FrameSlot *fs = last_slot_with(sc, flag, flag_name);
    if (!fs) return MR_E_INVALID;
    return read_back(fs->*buf, out, (size_t)fs->last_frame.width * fs->last_frame.height * per_px, what);
}

// The entries of `light` among the first `fetch` of the last frame's silhouette list (a frame with one light tags none:
// its light bits are zero), as (model, raw id, raw id) triples into out, at most cap of them; returns how many there are.
int decode_silhouette(mr_scene *sc, FrameSlot *fs, int light, int fetch, int32_t *out, int32_t cap)
{
    std::vector<int32_t> raw((size_t)std::max(fetch, 1) * 2);
    HIP_TRY(hipDeviceSynchronize());
    if (fetch > 0) HIP_TRY(hipMemcpy(raw.data(), fs->d_sil.p, (size_t)fetch * 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
    int n = 0;
    for (int i = 0; i < fetch; ++i) {
        const int face = raw[i * 2], word = raw[i * 2 + 1], k = word & 3;
        if ((word >> mr::SIL_LIGHT_SHIFT) != light) continue;
        if (out && n < cap) {
            int model = 0;
            while (model + 1 < (int)sc->model_face_off.size() && face >= sc->model_face_off[model + 1]) ++model;
            out[n * 3 + 0] = model;                              // entries of model.silhouette carry the raw ids
            out[n * 3 + 1] = sc->edge_raw[(size_t)face * 3 + k];
            out[n * 3 + 2] = sc->edge_raw[(size_t)face * 3 + (k + 1) % 3];
        }
        ++n;
    }
    return n;
}

// samples per output pixel and axis (MR_FRAME_SUPERSAMPLE2/4), 1 without
inline int ss_factor(const mr_frame_desc *fr)
{
    return (fr->flags & MR_FRAME_SUPERSAMPLE4) ? 4 : (fr->flags & MR_FRAME_SUPERSAMPLE2) ? 2 : 1;
}
inline int ss_shift(int s) { return s == 4 ? 2 : s == 2 ? 1 : 0; }

// a device that owns only part of the frame: a band of its rows or a stripe of its tile rows (a rank of a multi-GPU split)
inline bool is_partial(const mr_frame_desc *fr) { return fr->row_begin != 0 || fr->row_end != fr->height || fr->stripe_count > 1; }

// what a frame descriptor must satisfy, and what a scene with extra lights (mr_scene_set_extra_lights) refuses
int validate_frame(const mr_scene *sc, const mr_frame_desc *fr)
{
    if (!fr) return fail(MR_E_INVALID, "frame descriptor is NULL");
    if (!frame_size_ok(fr->height, fr->width)) return fail(MR_E_INVALID, "resolution out of range");
    if (fr->system != 1 && fr->system != -1) return fail(MR_E_INVALID, "system must be +1 (RH) or -1 (LH)");
    if (fr->row_begin < 0 || fr->row_end > fr->height || fr->row_begin >= fr->row_end)
        return fail(MR_E_INVALID, "row band must satisfy 0 <= row_begin < row_end <= height");
    if (fr->light_type < 0 || fr->light_type > 2) return fail(MR_E_INVALID, "unknown light type");
    if (fr->stripe_count > 1) {
        if (fr->stripe_index < 0 || fr->stripe_index >= fr->stripe_count)
            return fail(MR_E_INVALID, "stripe_index must satisfy 0 <= stripe_index < stripe_count");
        if (fr->row_begin != 0 || fr->row_end != fr->height)
            return fail(MR_E_INVALID, "a striped frame spans all rows: row_begin / row_end must be 0 / height");
    } else if (fr->stripe_count < 0) {
        return fail(MR_E_INVALID, "stripe_count must not be negative");
    }
    if ((fr->flags & MR_FRAME_SUPERSAMPLE2) && (fr->flags & MR_FRAME_SUPERSAMPLE4))
        return fail(MR_E_INVALID, "MR_FRAME_SUPERSAMPLE2 and MR_FRAME_SUPERSAMPLE4 are exclusive");
    const int s = ss_factor(fr);
    if (s > 1) {
        if (fr->width % s || fr->height % s) return fail(MR_E_INVALID, "supersampling: the sample grid's width and height must be multiples of s");
        if (fr->row_begin % s || fr->row_end % s) return fail(MR_E_INVALID, "supersampling: row_begin / row_end must be multiples of s");
        if (fr->stripe_count > 1) return fail(MR_E_INVALID, "supersampling is not available on striped frames");
    }
    const struct { bool on; const char *name; } passes[] = { { sc->ao.on, "ambient occlusion" }, { sc->dof.on, "depth of field" }, { sc->motion.on, "motion blur" },
                                                         { sc->taa.on, "temporal anti-aliasing" }, { sc->bloom.on, "bloom" }, { sc->shafts.on, "light shafts" }, { sc->tone.on, "tone mapping" },
                                                         { sc->layers.on, "data layers" } };
    for (const auto &pass : passes)
        if (pass.on && is_partial(fr))
            return fail(MR_E_INVALID, std::string(pass.name) + " takes whole frames (no row band, no stripes): its taps cross the bands");
    // (host order is the only ordering between the frames that write the history and those that read it)
    if (sc->taa.on && sc->taa.pending)
        return fail(MR_E_INVALID, "temporal anti-aliasing: an earlier frame of the scene has not been waited for (mr_render_wait): its history is not there yet");
    if (sc->tone.on && sc->tone.params.adaptive() && sc->tone.pending)
        return fail(MR_E_INVALID, "tone mapping: an earlier frame of the adaptive scene has not been waited for (mr_render_wait): its exposure is not there yet");
    if (sc->n_extra_lights > 0) {
        if (fr->flags & MR_FRAME_FACE_STATUS)
            return fail(MR_E_INVALID, "MR_FRAME_FACE_STATUS is not available with extra lights: the per-face status reads the one stencil buffer");
        if (fr->stripe_count > 1)
            return fail(MR_E_INVALID, "striped frames are not available with extra lights");
    }
    return MR_OK;
}

// a light as the kernels read it, from the fields of mr_frame_desc (its light_* ...) or of mr_light_desc
mr::LightRec light_rec(int32_t type, const double *pos, const double *dir, const double *color, const double *ambient, double specular_strength,
                       double att_constant, double att_linear, double att_quadratic, double spot_edge0, double spot_edge1)
{
    mr::LightRec l;
    std::memset(&l, 0, sizeof l);
    for (int j = 0; j < 3; ++j) { l.pos[j] = pos[j]; l.dir[j] = dir[j]; l.color[j] = color[j]; l.ambient[j] = ambient[j]; }
    l.specular_strength = specular_strength;
    l.att_constant = att_constant; l.att_linear = att_linear; l.att_quadratic = att_quadratic;
    l.spot_edge0 = spot_edge0; l.spot_edge1 = spot_edge1;
    l.type = type;
    return l;
}

// all the lights of a frame with several: the frame's own (FrameConst::light), then the scene's extra ones
void make_lights(const mr_scene *sc, const mr::FrameConst &fc, mr::FrameLights &fl)
{
    std::memset(&fl, 0, sizeof fl);
    fl.n = 1 + sc->n_extra_lights;
    fl.l[0] = fc.light;
    for (int k = 0; k < sc->n_extra_lights; ++k) fl.l[1 + k] = sc->extra_lights[k];
}

// Cluster culling (kernels_geometry.h, cluster_culled): the frame's CC_* bits, and the camera's centre of projection
// for the back-face cone.  Not when the caller wants per-face status or the fragment counters: those see faces one by
// one.  The cone needs the camera's centre of projection E and the sign convention of obj/triangular.py:47-48 in world
// space: with e the null vector of MVP's (x, y, w) columns, e = ew (E, 1), the screen-space area of a face whose corners
// are all in front of the camera has the sign of  det(viewport xy) * ew * n . (E - a)  for its world normal
// n = (b - a) x (c - a)  (Cauchy-Binet on the 3x4 by 4x3 product; checked against the per-face test on random cameras
// and triangles, tests/test_host_api.py).
// Measured on MI355X (round 3, A/B on one box): on a whole frame the test in front of every wavefront's first load
// costs more than the 40 % of c4's face wavefronts it ends are worth -- the face half is not what the launch waits
// for -- quoted regime c4 +2.5 %, c5 +0.8 %; on one rank's rows of a split frame, where most clusters go, set-up -3 us
// (c5, a rank of eight).  So: on for partial frames, off for whole ones; MR_CLUSTER_CULL=0 / 1 / box / count (`env`)
// force it off / on / boxes only / on and counted.
int cluster_cull_mode(const mr_frame_desc *fr, const char *env, double cull_eye[3])
{
    int mode = is_partial(fr) ? mr::CC_BOX | mr::CC_CONE : 0;
    if (env && !strcmp(env, "0")) mode = 0;
    if (env && (!strcmp(env, "1") || !strcmp(env, "count"))) mode = mr::CC_BOX | mr::CC_CONE;
    if (env && !strcmp(env, "box")) mode = mr::CC_BOX;
    if (fr->flags & (MR_FRAME_FACE_STATUS | MR_FRAME_COUNTERS)) mode = 0;
    if (mode & mr::CC_CONE) {
        const double *m = fr->mvp, *vp = fr->viewport;
        auto P = [&](int r, int c) { return m[r * 4 + (c == 2 ? 3 : c)]; };       // columns x, y, w
        double e[4];
        for (int i = 0; i < 4; ++i) {
            int r[3], k = 0;
            for (int j = 0; j < 4; ++j) if (j != i) r[k++] = j;
            const double det = P(r[0], 0) * (P(r[1], 1) * P(r[2], 2) - P(r[1], 2) * P(r[2], 1))
                             - P(r[0], 1) * (P(r[1], 0) * P(r[2], 2) - P(r[1], 2) * P(r[2], 0))
                             + P(r[0], 2) * (P(r[1], 0) * P(r[2], 1) - P(r[1], 1) * P(r[2], 0));
            e[i] = (i & 1) ? -det : det;
        }
        const double det_v = vp[0] * vp[5] - vp[1] * vp[4];
        const double big = std::max(std::max(fabs(e[0]), fabs(e[1])), std::max(fabs(e[2]), fabs(e[3])));
        const bool ok = std::isfinite(big) && big > 0 && fabs(e[3]) > 1e-9 * big && std::isfinite(det_v) && det_v != 0 &&
                        vp[8] == 0 && vp[9] == 0;          // (an orthographic camera has no centre: the boxes only)
        if (ok) {
            for (int j = 0; j < 3; ++j) cull_eye[j] = e[j] / e[3];
            if (det_v * e[3] < 0) mode |= mr::CC_NEGATIVE;
        } else {
            mode &= ~mr::CC_CONE;
        }
    }
    if (env && !strcmp(env, "count") && mode) mode |= mr::CC_COUNT;
    return mode;
}

// The frame's constants as the kernels read them (rast_types.h, FrameConst).
mr::FrameConst make_const(const mr_scene *sc, const mr_frame_desc *fr, const Env &env)
{
    mr::FrameConst fc;
    std::memset(&fc, 0, sizeof fc);
    fc.width = fr->width; fc.height = fr->height; fc.system = fr->system;
    fc.backface_culling = fr->backface_culling; fc.flags = fr->flags;
    // output rows count from the top, the reference's buffers from the bottom (obj/core.py:640 flips)
    fc.band_y0 = fr->height - fr->row_end;
    fc.band_y1 = fr->height - fr->row_begin;
    fc.tiles_x = (fr->width + mr::TILE_W - 1) / mr::TILE_W;
    if (fr->stripe_count > 1) {
        // interleaved tile rows: this device owns frame tile rows stripe_index, stripe_index + N, ...
        const int rows = (fr->height + mr::TILE_H - 1) / mr::TILE_H;
        fc.tile_y0 = fr->stripe_index;
        fc.tile_step = fr->stripe_count;
        fc.tiles_y = rows > fr->stripe_index ? (rows - 1 - fr->stripe_index) / fr->stripe_count + 1 : 0;
        fc.out_tile_rows = (rows + fr->stripe_count - 1) / fr->stripe_count;
    } else {
        fc.tile_y0 = fc.band_y0 / mr::TILE_H;
        fc.tile_step = 1;
        fc.tiles_y = (fc.band_y1 - 1) / mr::TILE_H + 1 - fc.tile_y0;
        fc.out_tile_rows = 0;
    }
    fc.n_vertices = (int32_t)(sc->verts.size() / 4);
    fc.n_faces = (int32_t)(sc->faces.size() / 12);
    fc.n_edges = (int32_t)sc->edges.size();
    fc.n_materials = (int32_t)sc->materials.size();
    std::memcpy(fc.mvp, fr->mvp, sizeof fc.mvp);
    std::memcpy(fc.viewport, fr->viewport, sizeof fc.viewport);
    std::memcpy(fc.debug_mvp, fr->debug_mvp, sizeof fc.debug_mvp);
    std::memcpy(fc.planes, fr->frustum_planes, sizeof fc.planes);
    fc.two_nf = 2 * fr->z_near * fr->z_far;          // obj/core.py:228, evaluated left to right
    fc.f_plus_n = fr->z_far + fr->z_near;
    fc.f_minus_n = fr->z_far - fr->z_near;
    for (int j = 0; j < 3; ++j) {
        fc.camera_pos[j] = fr->camera_pos[j];
        fc.background[j] = fr->background[j];
    }
    fc.light = light_rec(fr->light_type, fr->light_pos, fr->light_dir, fr->light_color, fr->light_ambient, fr->specular_strength,
                         fr->att_constant, fr->att_linear, fr->att_quadratic, fr->spot_edge0, fr->spot_edge1);
    fc.background_u8 = (uint32_t)fr->background_u8;
    std::memcpy(fc.sky_tri, fr->sky_tri, sizeof fc.sky_tri);
    std::memcpy(fc.sky_rays, fr->sky_rays, sizeof fc.sky_rays);
    fc.sky_size = sc->sky_size;
    fc.has_no_depth = sc->has_no_depth ? 1 : 0;     // (found at commit: a scan of the face flags here was 0.2 ms of host time per frame of a million faces)
    fc.same_clip = memcmp(fr->mvp, fr->debug_mvp, sizeof(fr->mvp)) == 0 ? 1 : 0;
    fc.edge_compact = sc->edge_compact ? 1 : 0;
    fc.pos32 = sc->pos32 ? 1 : 0;
    fc.cluster_cull = cluster_cull_mode(fr, env.cluster_cull, fc.cull_eye);
    const int s = ss_factor(fr);
    fc.ss_mode = s > 1 ? ss_shift(s) | (env.resolve_separate ? mr::SS_SEPARATE : 0) : 0;
    return fc;
}

// bytes of the uint8 output of a frame: the band's rows, or the striped layout's blocks (a supersampled frame: its
// output pixels, s x s samples each)
size_t out_bytes(const mr_frame_desc *fr)
{
    if (fr->stripe_count > 1) {
        const int rows = (fr->height + mr::TILE_H - 1) / mr::TILE_H;
        return (size_t)((rows + fr->stripe_count - 1) / fr->stripe_count) * mr::TILE_H * fr->width * 3;
    }
    const int s = ss_factor(fr);
    return (size_t)((fr->row_end - fr->row_begin) / s) * (fr->width / s) * 3;
}

// k_bin_work: enough wavefronts for every one to be resident at once (five per SIMD): an item is three dependent trips to
// memory and a returning atomic, so the kernel lasts as many of those chains as a wavefront has items (c4: 512
// workgroups 12.7 us, 1 280 11.5; c5: 25.0 -> 19.0; quoted regime c4 -1.5 %)
constexpr unsigned WORK_BLOCKS = 1280;
constexpr unsigned COUNT_BLOCKS = 512;      // at most this many workgroups of k_bin_work count leftover survivors
constexpr unsigned SPLIT_MAX_BIG = 64;      // tiles of a whole frame shared out at most (a small grid: HEAVY0_MAX)

// What enqueue_frame decided about this frame, once, before its first step.
//   partial      this device owns only part of the frame
//   deferred     the overlay is left to finish_overlay
//   overlay      this call draws (whole frame) or exports (partial frame) the overlay
//   taps_asked   the CALLER asked for the z / stencil / winner / float-frame taps
//   keep         MR_FRAME_KEEP_BUFFERS, asked for or implied;  shadows: MR_FRAME_SHADOWS
//   timing       MR_FRAME_NO_TIMING records no marks; MR_FRAME_LIGHT_TIMING not all_marks: those around the frame and the tile kernel
//   ml, ss       several lights / supersampled: the instantiations of k_setup and k_tile
//   ordered      k_tile takes the heaviest tiles first;  split: it shares heavy tiles out, from split_cost / split_quads, at most split_max
//   full         the general kernels k_setup_full / k_tile_full; else the frame-only ones k_setup / k_tile (tile_body, kernels_tile.h)
//   serial       the scene's frame serial with this frame
//   edge_spread  EDGE_DENSE, or lanes per edge as a shift;  face_blocks, count_blocks: workgroups of k_setup's face half, of k_bin_work's counting
//   order_bytes  d_hist: the tile order in front, the tiles' class bytes behind
//   ao           the scene has ambient obscurance on: k_ao behind the tile kernel, with ao_params, the scene's description now
//   dof          the scene has depth of field on: k_dof behind them, with dof_params, likewise
//   motion       the scene has motion blur on: k_velocity and k_mblur behind them, with motion_params, likewise
//   taa          the scene has temporal anti-aliasing on: k_velocity and k_taa behind k_ao, in front of k_dof, with taa_params and
//                taa_vel (the velocity's scalars), likewise
//   bloom        the scene has bloom on: its 2 L launches behind k_mblur, in front of the overlay, with bloom_params, likewise
//   shafts       the scene has light shafts on: their three launches behind k_mblur, in front of the bloom, with shafts_params, likewise
//   tone         the scene has tone mapping on: its launches behind the bloom, in front of the overlay, with tone_params, likewise
//   layers       the scene has data layers on: k_layers right behind the tile kernel, in front of every pass above, with layers_params,
//                likewise; it rewrites nothing, so it is no part of post()
//   post()       a pass rewrites the float frame behind the tile kernel: the bytes are the full resolve of the result
struct FramePlan {
    Env env;
    bool partial, deferred, overlay, taps_asked, keep, shadows, timing, all_marks, ml, ss, ordered, split, full, ao, dof, motion, taa, bloom, shafts, tone, layers;
    mr::LayersParams layers_params;
    mr::AoParams ao_params;
    mr::DofParams dof_params;
    mr::MotionParams motion_params, taa_vel;
    mr::TaaParams taa_params;
    mr::BloomParams bloom_params;
    mr::ShaftsParams shafts_params;
    mr::ToneParams tone_params;
    bool post() const { return ao || dof || motion || taa || bloom || shafts || tone; }
    int n_lights, n_tiles;
    uint64_t serial;
    unsigned split_cost, split_quads, split_max, edge_spread, face_blocks, count_blocks;
    size_t order_bytes;
};

// The overlay of this frame: what it refuses, the lists of cameras left by mr_scene_set_overlay_cameras (built now -- or,
// for a whole frame of a caller that finishes it with finish_overlay, after the frame's kernels have been launched) and
// the slot's copy of them.  A device that owns only part of the frame (a rank of a multi-GPU split) cannot replay the
// overlay: its lines test z at pixels other devices own.  It appends the state of the touched pixels it owns to its rows
// instead (k_overlay_export), and the overlay is replayed on the assembled frame (mr_overlay_apply).
int plan_overlay(mr_scene *sc, FrameSlot *fs, const mr_frame_desc *fr, const mr::FrameConst &fc, bool may_defer, FramePlan &p)
{
    p.deferred = may_defer && sc->ov_pending.set && !p.partial &&
                 sc->ov_pending.width == fc.width && sc->ov_pending.height == fc.height;
    if (!p.deferred) realize_overlay(sc);
    p.overlay = sc->ov_points > 0 && !p.deferred;
    if (p.partial && fc.ss_mode)
        return fail(MR_E_INVALID, "the overlay of a supersampled frame is drawn on whole frames only");
    if (p.partial && fr->stripe_count <= 1 && (fr->height % (fr->row_end - fr->row_begin) || fr->row_begin % (fr->row_end - fr->row_begin)))
        return fail(MR_E_INVALID, "overlay on a row band: the bands of the split must be equal");
    if (p.overlay && (sc->ov_width != fc.width || sc->ov_height != fc.height))
        return fail(MR_E_INVALID, "overlay lists were built for a frame of another size");
    return p.overlay ? sync_slot_overlay(sc, fs->ov, fs->stream, p.partial || (fc.ss_mode != 0 && !p.post())) : MR_OK;
}

// Decides what kind of frame this is: fills the plan and the frame's constants.
int plan_frame(mr_scene *sc, FrameSlot *fs, const mr_frame_desc *fr, bool may_defer_overlay, mr::FrameConst &fc, FramePlan &p)
{
    using namespace mr;
    p.env = read_env();
    fc = make_const(sc, fr, p.env);
    p.partial = is_partial(fr);
    if (fc.flags & MR_FRAME_FACE_STATUS) fc.flags |= MR_FRAME_KEEP_BUFFERS;
    // (a supersampled frame resolved by k_resolve_full needs every tile's float colour)
    if (fc.ss_mode & SS_SEPARATE) fc.flags |= MR_FRAME_KEEP_FLOAT;
    // (a post pass reads the whole z-buffer -- the motion blur the winner map as well -- and rewrites the whole float frame,
    // in place or into the second one: every tile writes its taps, as for a caller who asked for them)
    p.ao = sc->ao.on; p.dof = sc->dof.on; p.motion = sc->motion.on; p.taa = sc->taa.on; p.bloom = sc->bloom.on; p.shafts = sc->shafts.on; p.tone = sc->tone.on;
    if (p.motion && sc->motion.params.n_models != (int32_t)sc->model_face_off.size())
        return fail(MR_E_INVALID, "motion blur: the scene's models changed since mr_scene_set_motion_blur: hand the classes over again");
    if (p.motion && sc->mfaces.on && sc->mfaces.deforming.size() != sc->model_face_off.size())
        return fail(MR_E_INVALID, "per-face velocity: the scene's models changed since mr_scene_set_motion_faces: hand the flags over again");
    if (p.taa && sc->taa.vel.n_models != (int32_t)sc->model_face_off.size())
        return fail(MR_E_INVALID, "temporal anti-aliasing: the scene's models changed since mr_scene_set_temporal_aa: hand the classes over again");
    if (p.taa && p.motion && !same_velocity_tables(sc->taa.vel, sc->taa.tables, sc->motion.params, sc->motion.tables))
        return fail(MR_E_INVALID, "temporal anti-aliasing: its velocity tables are not the motion blur's: one k_velocity serves both, hand both descriptions the same matrices");
    p.ao_params = sc->ao.params; p.dof_params = sc->dof.params; p.motion_params = sc->motion.params;
    p.taa_params = sc->taa.params; p.taa_vel = sc->taa.vel;
    p.bloom_params = sc->bloom.params;
    p.shafts_params = sc->shafts.params;
    p.tone_params = sc->tone.params;
    p.layers = sc->layers.on; p.layers_params = sc->layers.params;
    if (p.layers && p.layers_params.n_models != (int32_t)sc->model_face_off.size())
        return fail(MR_E_INVALID, "data layers: the scene's models changed since mr_scene_set_layers: hand the description over again");
    if (p.layers) fc.flags |= MR_FRAME_KEEP_BUFFERS;        // (the winner map, as for k_velocity)
    if (p.post()) fc.flags |= MR_FRAME_KEEP_BUFFERS | MR_FRAME_KEEP_FLOAT;
    // (The overlay needs z and colour too, but only at the pixels its lines touch: then only the tiles that hold such a
    // pixel write them, TileArgs::tap_mask.)
    p.taps_asked = (fc.flags & (MR_FRAME_KEEP_BUFFERS | MR_FRAME_KEEP_FLOAT)) != 0;
    p.deferred = p.overlay = false;
    if (fc.flags & MR_FRAME_OVERLAY) {
        if (int rc = plan_overlay(sc, fs, fr, fc, may_defer_overlay, p)) return rc;
        fc.flags |= MR_FRAME_KEEP_BUFFERS | MR_FRAME_KEEP_FLOAT;
    }
    p.keep = (fc.flags & MR_FRAME_KEEP_BUFFERS) != 0; p.shadows = (fc.flags & MR_FRAME_SHADOWS) != 0;
    p.timing = !(fc.flags & MR_FRAME_NO_TIMING);
    p.all_marks = p.timing && !(fc.flags & MR_FRAME_LIGHT_TIMING);
    p.n_lights = 1 + sc->n_extra_lights; p.ml = p.n_lights > 1;
    p.ss = fc.ss_mode != 0;
    p.n_tiles = fc.tiles_x * fc.tiles_y;
    p.serial = sc->frame_serial + 1;
    // The order k_tile takes the tiles in.  Heaviest-first order shortens the critical path of a frame that has the
    // device to itself.  When the scene is being rendered from several streams at once (frames in flight), the next
    // frame's work fills the tail anyway and bunching the heavy tiles at the front only makes them compete: measured on
    // MI355X with three streams, row-major is 4 % (c4) to 28 % (c2) faster per frame, and 10 % slower for a lone frame.
    // So: ordered when no other stream took one of the scene's last frames.  MR_TILE_ORDER=rowmajor | heaviest forces
    // either (for the ablation in DESIGN.md).
    bool alone = true;
    for (auto &s : sc->slots)
        if (s.get() != fs && s->have_frame && p.serial - s->last_serial <= 8) alone = false;
    p.ordered = p.env.tile_order == 2 || (p.env.tile_order == 0 && alone);
    // which tiles are shared out over HEAVY_SPLIT workgroups next frame: on a device whose tiles are all resident
    // at once (a rank of a multi-GPU split; there the launch lasts as long as the slowest tile, see HEAVY_SPLIT) every
    // tile with a quad walk worth sharing; on a whole frame the handful that outlast everything else -- which still lead
    // the order (k_tile<true> and its class rule), but are shared out only with MR_TILE_SPLIT=1 (split_max = 0 otherwise,
    // see below).  MR_TILE_SPLIT=0 | 1 forces the split off / on for every grid.
    const bool small_grid = p.n_tiles <= 2048;
    p.split_cost = small_grid ? 350u : p.env.split_cost;
    p.split_quads = small_grid ? 32u : p.env.split_quads;
    // (Whole frames were shared out too while the strip walk took a heavy tile's quads one after the other, 46 us for the
    // 111 of c4's heaviest.  With the span walk a lone c4 frame's k_tile lasts 62.9 us with its heavy tiles shared out
    // and 60.6 us with none (split_max = 0), c3's 73.2 and 70.1, and a rank of eight still gains: 55.8 us against 57.4 for the
    // slowest rank's rows -- profiles/quad_spans_ab.txt.)
    p.split_max = small_grid ? (unsigned)HEAVY0_MAX : p.env.tile_split > 0 ? std::min<unsigned>(SPLIT_MAX_BIG, (unsigned)HEAVY0_MAX) : 0u;
    p.split = !p.ml && (p.env.tile_split < 0 ? (small_grid || p.ordered) : p.env.tile_split != 0);
    // The frame-only kernels count nothing and know no face that writes no z: a frame whose counters or per-face status
    // somebody reads, and every frame of a scene with a depth_test == False model, takes the general ones.
    p.full = sc->force_full || sc->has_no_depth || (fc.flags & (MR_FRAME_COUNTERS | MR_FRAME_FACE_STATUS)) != 0;
    // small meshes: one edge per 2 / 4 lanes, so that a wavefront rarely finds more silhouette edges than one round
    // of its quad set-up takes (kernels_geometry.h, edge_block)
    const int spread_env = p.env.edge_spread;                                                         // -1: dense
    const bool dense = spread_env == -1 || (spread_env == -2 && fc.n_edges > (1 << 17));
    p.edge_spread = dense ? EDGE_DENSE : spread_env >= 0 ? (unsigned)std::min(spread_env, 4) : fc.n_edges <= (1 << 15) ? 2u : 1u;
    p.face_blocks = fc.n_faces > 0 ? blocks_for(fc.n_faces, SETUP_BLOCK) : 0u;
    p.count_blocks = fc.n_faces > 0 ? std::min(COUNT_BLOCKS, blocks_for((long long)fc.n_faces * WAVE, 256)) : 0u;
    // tile order: ORDER_HEAD + n_tiles words (written by k_bin_work), then the tiles' class bytes (k_tile, for the next frame)
    p.order_bytes = (((size_t)ORDER_HEAD + (size_t)std::max(p.n_tiles, 1)) * sizeof(uint32_t) + 15) & ~(size_t)15;
    return MR_OK;
}

// Grows the slot's buffers to what this frame needs, at the capacities the scene has learnt.
int grow_slot(mr_scene *sc, FrameSlot *fs, const mr::FrameConst &fc, const FramePlan &p)
{
    using namespace mr;
    const size_t npx = (size_t)fc.width * fc.height, nF = (size_t)std::max(fc.n_faces, 1), nV = (size_t)std::max(fc.n_vertices, 1), nT = (size_t)std::max(p.n_tiles, 1);
    if (sc->quad_cap == 0) sc->quad_cap = (uint32_t)std::min<size_t>((size_t)std::max(fc.n_edges, 1) * p.n_lights, 1u << 17);
    fs->quad_cap = sc->quad_cap; fs->work_cap = sc->work_cap;
    for (int c = 0; c < BIN_CLASSES; ++c) fs->bin_cap[c] = sc->bin_cap[c];
    // (the vertex records only with MR_VERTEX_PATH=mfma, the taps only when kept: nothing is asked for otherwise)
    const size_t mfma_v = p.env.vertex_mfma ? nV : 0, kept = p.keep ? npx : 0, kept_f = (fc.flags & MR_FRAME_KEEP_FLOAT) ? npx : 0;
    const struct { DevBuf &buf; size_t bytes; } sized[] = {
        { fs->d_vout, mfma_v * sizeof(VertexOut) }, { fs->d_vclip, mfma_v * sizeof(VertexClip) },
        { fs->d_count_list, nF * sizeof(uint32_t) }, { fs->d_tris, nF * sizeof(TriRec) }, { fs->d_clips, nF * sizeof(TriClip) },
        { fs->d_status, nF }, { fs->d_quads, (size_t)fs->quad_cap * sizeof(QuadRec) }, { fs->d_sil, (size_t)fs->quad_cap * 2 * sizeof(int32_t) },
        { fs->d_bin_count, (size_t)(BIN_CLASSES * p.n_tiles + 1) * 4 }, { fs->d_work, (size_t)fs->work_cap * sizeof(uint2) },
        { fs->d_tile_stats, nT * TILE_REC * 4 }, { fs->d_z, kept * sizeof(double) }, { fs->d_winner, kept * sizeof(int32_t) },
        { fs->d_stencil, kept * sizeof(int32_t) }, { fs->d_frame, kept_f * 3 * sizeof(float) },
        { fs->d_frame_b, p.dof || p.motion || p.taa ? kept_f * 3 * sizeof(float) : 0 },
        // (one pyramid per slot: frames in flight keep their own)
        { fs->d_bloom, p.bloom ? bloom_pyramid(fc.width, fc.height, p.bloom_params.levels).floats * sizeof(float) : 0 },
        // (S and R per slot: two frames in flight under two cameras keep their own light position)
        { fs->d_shafts, p.shafts ? 2 * shafts_level(fc.width, fc.height, p.shafts_params.levels).device_floats() * sizeof(float) : 0 },
        // (likewise: every slot its histogram, its exposure cell and its slab)
        { fs->d_tone, p.tone ? tone_slot_bytes(tone_grid(fc.width, fc.height, p.env)) : 0 } };
    for (const auto &b : sized) HIP_TRY(b.buf.ensure(b.bytes));
    if (p.taa)
        if (int rc = grow_history(sc, fc.width, fc.height)) return rc;
    for (int k = 1; k < p.n_lights; ++k) HIP_TRY(fs->d_stencil_x[k - 1].ensure(kept * sizeof(int32_t)));
    if (int rc = ensure_cleared(fs->d_counters, 2 * sizeof(Counters) + sizeof(Sticky), fs->stream)) return rc;
    for (int c = 0; c < BIN_CLASSES; ++c) {
        const size_t bytes = nT * fs->bin_cap[c] * 4;
        if (bytes > ((size_t)48 << 30))
            return fail(MR_E_OVERFLOW, "more primitives in one 16x16 tile than the tile lists are allowed to grow to (48 GB per class)");
        HIP_TRY(fs->d_items[c].ensure(bytes));
    }
    HIP_TRY(fs->d_quad_bound.ensure(nT * fs->bin_cap[2] * sizeof(float)));      // one float beside every entry of the quad lists

    if (!fs->events_ok) {
        for (auto &set : fs->ev_ring) for (auto &e : set) HIP_TRY(hipEventCreate(&e));
        HIP_TRY(hipHostMalloc((void **)&fs->h_counters, sizeof(Counters) + sizeof(Sticky), hipHostMallocDefault));
        fs->h_sticky = reinterpret_cast<Sticky *>(fs->h_counters + 1);
        fs->events_ok = true;
    }
    return MR_OK;
}

// The state the tile lists keep from frame to frame, behind the frame's first mark.  The list cursors are left zeroed
// by k_tile and the frame counters are cleared by the previous frame's k_tile, so a steady-state frame issues no
// memset; only a new tile grid needs one.
int grow_tile_state(FrameSlot *fs, const FramePlan &p)
{
    using namespace mr;
    HIP_TRY(fs->d_hist.ensure(p.order_bytes + (size_t)std::max(p.n_tiles, 1) + 16));     // class bytes: 16-byte aligned, padded
    // split tiles: HEAVY0_MAX arrival counters (zero between frames), then the parts' stencil counts, then their counts of staged quads
    constexpr size_t arrive_bytes = (size_t)HEAVY0_MAX * 4;
    if (int rc = ensure_cleared(fs->d_split, arrive_bytes + arrive_bytes * HEAVY_SPLIT * TILE_PX + arrive_bytes * HEAVY_SPLIT, fs->stream, arrive_bytes)) return rc;
    if (fs->bins_zeroed_for != BIN_CLASSES * p.n_tiles + 1) {
        HIP_TRY(hipMemsetAsync(fs->d_bin_count.p, 0, fs->d_bin_count.cap, fs->stream));
        HIP_TRY(hipMemsetAsync(fs->d_hist.p, 0, fs->d_hist.cap, fs->stream));       // no history for a new tile grid
        fs->bins_zeroed_for = BIN_CLASSES * p.n_tiles + 1;
    }
    return MR_OK;
}

mr::BinArgs bin_args(const FrameSlot *fs)
{
    mr::BinArgs ba;
    ba.tris = fs->d_tris.as<mr::TriRec>(); ba.quads = fs->d_quads.as<mr::QuadRec>();
    ba.ctr = fs->ctr(fs->frames_enqueued); ba.quad_cap = fs->quad_cap;
    ba.bin_count = fs->d_bin_count.as<uint32_t>();
    for (int c = 0; c < mr::BIN_CLASSES; ++c) { ba.items[c] = fs->d_items[c].as<uint32_t>(); ba.cap[c] = fs->bin_cap[c]; }
    ba.work = fs->d_work.as<uint2>(); ba.work_cap = fs->work_cap;
    ba.quad_bound = fs->d_quad_bound.as<float>();
    return ba;
}

// ---- 1. set-up: faces and (with shadows) edges, one launch; with MR_VERTEX_PATH=mfma the vertex kernel in front of it
int launch_setup(mr_scene *sc, FrameSlot *fs, const mr::FrameConst &fc, const FramePlan &p, const mr::FrameLights &lights)
{
    using namespace mr;
    hipStream_t stream = fs->stream;
    SetupKernArgs ska;
    ska.fc = fc; ska.bins = bin_args(fs); ska.face_blocks = p.face_blocks;
    SetupArgs &sa = ska.sa;
    sa.faces = sc->d_faces.as<int32_t>(); sa.face_flags = sc->d_face_flags.as<uint8_t>();
    sa.verts = sc->d_verts.as<double>(); sa.uv = sc->d_uv.as<float>(); sa.normals = sc->d_normals.as<float>();
    sa.vout = fs->d_vout.as<VertexOut>(); sa.vclip = fs->d_vclip.as<VertexClip>();
    sa.face_pos = sc->d_face_pos.p; sa.clusters = sc->d_clusters.as<ClusterRec>();
    sa.tris = fs->d_tris.as<TriRec>(); sa.clips = fs->d_clips.as<TriClip>();
    sa.status = fs->d_status.as<uint8_t>(); sa.count_list = fs->d_count_list.as<uint32_t>(); sa.ctr = ska.bins.ctr;
    sa.edges = sc->edge_compact ? reinterpret_cast<const EdgeRec *>(sc->d_edges32.p) : sc->d_edges.as<EdgeRec>();
    sa.edge_inc = sc->d_edge_inc.as<uint32_t>(); sa.face_n = sc->d_face_n.as<double>();
    sa.tile_class = reinterpret_cast<uint8_t *>(fs->d_hist.p) + p.order_bytes; sa.order = fs->d_hist.as<uint32_t>();
    sa.sil_edges = fs->d_sil.as<int32_t>(); sa.quads = fs->d_quads.as<QuadRec>(); sa.quad_cap = fs->quad_cap;

    if (p.env.vertex_mfma && fc.n_vertices > 0)
        hipLaunchKernelGGL(k_vertex_mfma, dim3(blocks_for(fc.n_vertices, 64)), dim3(256), 0, stream, fc,
                           sc->d_verts.as<double>(), fs->d_vout.as<VertexOut>(), fs->d_vclip.as<VertexClip>());
    if (p.all_marks) HIP_TRY(hipEventRecord(fs->ev[1], stream));

    const bool edges = p.shadows && fc.n_edges > 0;
    ska.sil = SilArgs{};
    if (edges) sc->sil.choose_path(p.env.sil_cache, p.n_lights, fs->id, stream, fs->quad_cap, sc->frame_serial, fc.light, ska.sil);
    constexpr unsigned QS_PER_BLOCK = SETUP_BLOCK / QS_LANES;
    const unsigned edge_blocks = !edges ? 0u
                               : ska.sil.mode == SIL_CACHED ? (ska.sil.count + QS_PER_BLOCK - 1) / QS_PER_BLOCK     // quad workgroups
                               : p.edge_spread == EDGE_DENSE ? blocks_for(fc.n_edges, 2 * SETUP_BLOCK) : blocks_for((long long)fc.n_edges << p.edge_spread, SETUP_BLOCK);
    ska.edge_spread = ska.sil.mode == SIL_CACHED ? EDGE_CACHED : p.edge_spread;
    if (p.ml) ska.lights = lights; else ska.lights.n = 1;      // (only the ML instantiations read them)
    // k_setup<PRE_XFORM, ML> / k_setup_full<PRE_XFORM, ML>, by [full][!ML][!PRE_XFORM]
    static void (*const kernel[2][2][2])(const SetupKernArgs) = {
        { { k_setup<true, true>, k_setup<false, true> }, { k_setup<true, false>, k_setup<false, false> } },
        { { k_setup_full<true, true>, k_setup_full<false, true> }, { k_setup_full<true, false>, k_setup_full<false, false> } } };
    hipLaunchKernelGGL(kernel[p.full][!p.ml][!p.env.vertex_mfma], dim3(1 + p.face_blocks + edge_blocks), dim3(SETUP_BLOCK), 0, stream, ska);
    return ska.sil.mode == SIL_CAPTURE ? sc->sil.capture_launched(&sa.ctr->n_quads, stream) : MR_OK;
}

// ---- 2. tile lists of the large primitives + leftover survivor counts (one wavefront per face,
// grid-stride: a mesh of large faces lists most of them)
void launch_bin_work(FrameSlot *fs, const mr::FrameConst &fc, const FramePlan &p)
{
    using namespace mr;
    hipLaunchKernelGGL(k_bin_work, dim3(p.count_blocks + WORK_BLOCKS), dim3(256), 0, fs->stream, fc, bin_args(fs), fs->d_count_list.as<uint32_t>(),
                       fs->d_tris.as<TriRec>(), fs->d_clips.as<TriClip>(), fs->d_status.as<uint8_t>(), fs->ctr(fs->frames_enqueued), p.count_blocks,
                       p.env.big_tri_reject ? 1u : 0u);
}

// ---- 3. tiles: coverage, z, stencil, shading, finalise
int launch_tile(mr_scene *sc, FrameSlot *fs, const mr::FrameConst &fc, const FramePlan &p, const mr::FrameLights &lights, uint8_t *d_out)
{
    using namespace mr;
    TileKernArgs tka;
    tka.fc = fc;
    TileArgs &ta = tka.ta;
    ta.clips = fs->d_clips.as<TriClip>(); ta.quads = fs->d_quads.as<QuadRec>();
    ta.bin_count = fs->d_bin_count.as<uint32_t>();
    for (int c = 0; c < BIN_CLASSES; ++c) { ta.items[c] = fs->d_items[c].as<uint32_t>(); ta.cap[c] = fs->bin_cap[c]; }
    ta.tap_mask = (p.overlay && !p.taps_asked) ? fs->ov.list<uint8_t>(3) : nullptr;
    ta.zbuf = p.keep ? fs->d_z.as<double>() : nullptr;
    ta.winner = p.keep ? fs->d_winner.as<int32_t>() : nullptr;
    ta.stencil = p.keep ? fs->d_stencil.as<int32_t>() : nullptr;
    ta.tile_stats = fs->d_tile_stats.as<uint32_t>();
    // (the counters are double-buffered: this frame's, and the next frame's, which this kernel clears)
    ta.ctr = fs->ctr(fs->frames_enqueued); ta.next_ctr = fs->ctr(fs->frames_enqueued + 1); ta.sticky = fs->sticky();
    ta.order = p.ordered ? fs->d_hist.as<uint32_t>() : nullptr;
    ta.tile_class = reinterpret_cast<uint8_t *>(fs->d_hist.p) + p.order_bytes;
    ta.split_arrive = fs->d_split.as<uint32_t>(); ta.split_sten = fs->d_split.as<int32_t>() + HEAVY0_MAX;
    ta.split_cost = p.split_cost; ta.split_quads = p.split_quads; ta.split_max = p.split_max;
    ta.quad_walk = (uint32_t)p.env.quad_walk;
    ta.quad_bound = fs->d_quad_bound.as<float>(); ta.quad_cull = (uint32_t)p.env.quad_tile_cull;
    ta.pair_log = (uint32_t)fc.n_faces <= PAIR_LOG_MAX_FACE ? (uint32_t)p.env.pair_log : 0u;   // (a log entry holds 24 bits of the face)
    ShadeArgs &sh = tka.sh;
    sh.tris = fs->d_tris.as<TriRec>(); sh.face_pos = sc->d_face_pos.p; sh.face_attr = sc->d_face_attr.as<FaceAttr>();
    sh.materials = sc->d_materials.as<Material>();
    sh.sky = sc->sky_size > 0 ? sc->d_sky.as<uint8_t>() : nullptr;
    sh.gamma_lut = sc->d_gamma.as<float>(); sh.out = d_out;
    sh.frame = (fc.flags & MR_FRAME_KEEP_FLOAT) ? fs->d_frame.as<float>() : nullptr;
    tka.ml.lights.n = 1;
    if (p.ml) tka.ml.lights = lights;
    for (int k = 1; p.ml && k < MAX_LIGHTS; ++k) tka.ml.stencil[k - 1] = p.keep && k < p.n_lights ? fs->d_stencil_x[k - 1].as<int32_t>() : nullptr;
    if (p.n_tiles <= 0) {     // nothing to draw on this device (a stripe beyond the frame): still hand the counters on
        HIP_TRY(hipMemsetAsync(ta.next_ctr, 0, sizeof(Counters), fs->stream));
        return MR_OK;
    }
    // k_tile<SPLIT, SS, ML> / k_tile_full<SPLIT, SS, ML> and the workgroups it takes beyond one per tile, by [full] and
    // (ML ? 0 : SPLIT ? 2 : 4) + !SS; a frame with several lights never splits
    static const struct { void (*kernel)(const TileKernArgs); int front; } choice[2][6] = {
        { { k_tile<false, true, true>, 0 },            { k_tile<false, false, true>, 0 },
          { k_tile<true, true, false>, SPLIT_FRONT },  { k_tile<true, false, false>, SPLIT_FRONT },
          { k_tile<false, true, false>, 0 },           { k_tile<false, false, false>, 0 } },
        { { k_tile_full<false, true, true>, 0 },           { k_tile_full<false, false, true>, 0 },
          { k_tile_full<true, true, false>, SPLIT_FRONT }, { k_tile_full<true, false, false>, SPLIT_FRONT },
          { k_tile_full<false, true, false>, 0 },          { k_tile_full<false, false, false>, 0 } } };
    const auto &c = choice[p.full][(p.ml ? 0 : p.split ? 2 : 4) + !p.ss];
    hipLaunchKernelGGL(c.kernel, dim3((unsigned)(p.n_tiles + c.front)), dim3(TILE_PX), 0, fs->stream, tka);
    return MR_OK;
}

// The bytes of a frame that ran k_ao or k_dof: the tree's finalise of the whole float frame, after the overlay (the
// accumulation's resolve with scale 1: block mean, min(., 1), the gamma step, rows flipped).
void launch_post_resolve(mr_scene *sc, FrameSlot *fs, const mr_frame_desc &fr, int ss_mode, uint8_t *d_out)
{
    mr_accum::launch_resolve(fs->stream, fs->d_frame.as<float>(), fr.width, fr.height, ss_mode & mr::SS_SHIFT_MASK, 1.0f,
                             sc->d_gamma.as<float>(), d_out);
}

// A pass has written the other float frame: that one is the slot's float frame from here on.  The overlay, the resolve,
// mr_read_frame_f32 and k_accum_add read d_frame; work enqueued on the stream before this point keeps the pointers it was
// given; the two ping-pong when several of k_taa, k_dof and k_mblur run.
inline void swap_float_frames(FrameSlot *fs) { std::swap(fs->d_frame, fs->d_frame_b); }

// ---- 4. behind the tile kernel: the per-face verdicts, the ambient obscurance, the temporal anti-aliasing, the depth of field, the motion blur, the light shafts, the bloom, the tone mapping, the overlay (exported
// by a device that owns part of the frame, else drawn: after the lit pass' per-face verdicts, as in obj/core.py:624-638)
// and the resolve of a supersampled, darkened or blurred frame
int launch_after_tile(mr_scene *sc, FrameSlot *fs, const mr_frame_desc *fr, const mr::FrameConst &fc, const FramePlan &p, uint8_t *d_out)
{
    using namespace mr;
    hipStream_t stream = fs->stream;
    if ((fc.flags & MR_FRAME_FACE_STATUS) && fc.n_faces > 0)
        hipLaunchKernelGGL(k_face_status, dim3(blocks_for(fc.n_faces, 256)), dim3(256), 0, stream, fc, fs->d_tris.as<TriRec>(),
                           fs->d_clips.as<TriClip>(), fs->d_z.as<double>(), fs->d_stencil.as<int32_t>(), fs->d_status.as<uint8_t>());
    if (p.ao && p.n_tiles > 0)
        if (int rc = launch_ao(sc, stream, fs->d_z.as<double>(), fs->d_frame.as<float>(), fc.width, fc.height, p.ao_params, p.env.ao_shape)) return rc;
    if (p.taa && p.n_tiles > 0) {
        if (int rc = launch_taa(sc, stream, fs->motion, fs->motion_faces, fs->d_z.as<double>(), fs->d_winner.as<int32_t>(), fs->d_frame.as<float>(),
                                fs->d_frame_b.as<float>(), fc.width, fc.height, p.taa_params, p.taa_vel, p.env.taa_shape))
            return rc;
        swap_float_frames(fs);
    }
    if (p.dof && p.n_tiles > 0) {
        if (int rc = launch_dof(sc, stream, fs->d_z.as<double>(), fs->d_frame.as<float>(), fs->d_frame_b.as<float>(), fc.width, fc.height, p.dof_params,
                                p.env.dof_shape))
            return rc;
        swap_float_frames(fs);
    }
    if (p.motion && p.n_tiles > 0) {
        if (int rc = launch_motion(sc, stream, fs->motion, fs->motion_faces, fs->d_z.as<double>(), fs->d_winner.as<int32_t>(), fs->d_frame.as<float>(),
                                   fs->d_frame_b.as<float>(), fc.width, fc.height, p.motion_params, p.env.mblur_shape,
                                   p.taa))
            return rc;
        swap_float_frames(fs);
    }
    // (the lens and the blur key on the z of the surface behind a ray and would treat the rays as paint on it: the shafts
    // are added behind them; the bloom comes after, so a bright shaft may glow)
    if (p.shafts && p.n_tiles > 0)
        if (int rc = launch_light_shafts(sc, stream, fs->d_frame.as<float>(), fs->d_z.as<double>(), fs->d_shafts.as<float>(), fc.width, fc.height, p.shafts_params))
            return rc;
    // (the glow forms in the lens, behind the blur; k_taa's history was written in front of it and never holds glow; the
    // overlay's lines are drawn over it and do not glow)
    if (p.bloom && p.n_tiles > 0)
        if (int rc = launch_bloom(sc, stream, fs->d_frame.as<float>(), fs->d_bloom.as<float>(), fc.width, fc.height, p.bloom_params, p.env.bloom_shape))
            return rc;
    // (the exposure is metered from everything that adds light, the glow and the rays included; the overlay's lines are
    // drawn over the result and keep their colours)
    if (p.tone && p.n_tiles > 0)
        if (int rc = launch_tone_map(sc, stream, fs->d_frame.as<float>(), fs->d_tone.as<uint32_t>(), fc.width, fc.height, p.tone_params, p.env)) return rc;
    if (p.overlay && p.partial) {
        const int world = fr->stripe_count > 1 ? fr->stripe_count : fr->height / (fr->row_end - fr->row_begin);
        const int rank = fr->stripe_count > 1 ? fr->stripe_index : fr->row_begin / (fr->row_end - fr->row_begin);
        const int n_slots = (int)sc->ov_touched.size();
        OverlayState *state = reinterpret_cast<OverlayState *>(d_out + ((out_bytes(fr) + 15) & ~(size_t)15));
        hipLaunchKernelGGL(k_overlay_export, dim3(blocks_for(n_slots, 256)), dim3(256), 0, stream, fs->ov.list<int32_t>(5), n_slots,
                           fs->d_z.as<double>(), fs->d_frame.as<float>(), fc.width, fc.height, world, fr->stripe_count > 1 ? 1 : 0, rank, state);
    } else if (p.overlay) {
        launch_overlay(sc, fs->ov, fs->d_z.as<double>(), fs->d_frame.as<float>(), fc.ss_mode || p.post() ? nullptr : d_out, fc.width, fc.height, fc.system, stream);
    }
    if (p.deferred) return MR_OK;                                    // (finish_overlay resolves)
    if (p.post()) launch_post_resolve(sc, fs, *fr, fc.ss_mode, d_out);
    else launch_resolve(sc, fs->ov, fs->d_frame.as<float>(), *fr, fc.ss_mode, p.overlay, d_out, stream);
    return MR_OK;
}

// ---- 5. what the slot and the scene remember of the frame
void record_frame(mr_scene *sc, FrameSlot *fs, const mr_frame_desc *fr, const mr::FrameConst &fc, const FramePlan &p)
{
    sc->frame_serial = fs->last_serial = p.serial;
    fs->last_ordered = p.ordered;
    fs->last_full = p.full; fs->last_split = p.split;
    fs->overlay_deferred = p.deferred;
    fs->last_ss_mode = fc.ss_mode;
    fs->last_post = p.post();
    fs->last_motion = (p.motion || p.taa) && p.n_tiles > 0;
    if (p.taa && p.n_tiles > 0) taa_enqueued(sc, fs, fc.width, fc.height);
    fs->last_tone = p.tone && p.n_tiles > 0 ? (p.tone_params.fixed ? 2 : 1) : 0;
    fs->last_tone_exposure = p.tone_params.exposure;
    if (fs->last_tone && p.tone_params.adaptive()) tone_enqueued(sc, fs);
    fs->last_layers = p.layers && p.n_tiles > 0 ? p.layers_params.mask : 0;
    fs->last_frame = *fr; fs->last_frame.flags = fc.flags;
    fs->last_n_tiles = p.n_tiles;
    fs->last_n_lights = p.n_lights;
    fs->have_frame = true;
    fs->stats_reduced = false;
    fs->last_copied = false;
    fs->frames_enqueued += 1;
    sc->last = fs;
}

// Enqueues one frame on the slot's stream, with no host synchronisation; d_out receives the uint8 rows.  The event
// marks (FrameSlot) are recorded here, between the steps, but for mark 1 inside launch_setup.
int enqueue_frame(mr_scene *sc, FrameSlot *fs, const mr_frame_desc *fr, uint8_t *d_out, bool may_defer_overlay = false)
{
    int rc = commit(sc);
    if (rc) return rc;
    if ((rc = apply_poses(sc))) return rc;
    hipStream_t stream = fs->stream;
    mr::FrameConst fc;
    FramePlan p;
    if ((rc = plan_frame(sc, fs, fr, may_defer_overlay, fc, p))) return rc;
    if ((rc = grow_slot(sc, fs, fc, p))) return rc;
    fs->ev = fs->ev_ring[fs->frames_enqueued % EVENT_RING];
    fs->ev_marks[fs->frames_enqueued % EVENT_RING] = p.timing ? (p.all_marks ? 2 : 1) : 0;
    if (p.timing) HIP_TRY(hipEventRecord(fs->ev[0], stream));
    if ((rc = grow_tile_state(fs, p))) return rc;
    // several lights (mr_scene_set_extra_lights): the multi-light instantiations of k_setup and k_tile read them all
    mr::FrameLights lights;
    if (p.ml) make_lights(sc, fc, lights);
    if ((rc = launch_setup(sc, fs, fc, p, lights))) return rc;
    if (p.all_marks) HIP_TRY(hipEventRecord(fs->ev[2], stream));
    launch_bin_work(fs, fc, p);
    if (p.timing) HIP_TRY(hipEventRecord(fs->ev[3], stream));
    if ((rc = launch_tile(sc, fs, fc, p, lights, d_out))) return rc;
    if (p.timing) HIP_TRY(hipEventRecord(fs->ev[4], stream));
    // the data layers: from the winner map alone, in front of every pass that rewrites the float frame
    if (p.layers && p.n_tiles > 0)
        if ((rc = launch_layers(sc, stream, fs->layers, fs->d_winner.as<int32_t>(), fc.width, fc.height, p.layers_params))) return rc;
    if ((rc = launch_after_tile(sc, fs, fr, fc, p, d_out))) return rc;
    HIP_TRY(hipGetLastError());
    record_frame(sc, fs, fr, fc, p);
    return MR_OK;
}

// Second half of a frame whose overlay enqueue_frame left for later (may_defer_overlay): the device is busy with the
// frame's three kernels, the host builds the lines' lists meanwhile, then the upload and the overlay kernel follow on the
// frame's stream (and, on a supersampled frame, the resolve that has to wait for it).
int finish_overlay(mr_scene *sc, FrameSlot *fs, uint8_t *d_out)
{
    if (!fs->overlay_deferred) return MR_OK;
    fs->overlay_deferred = false;
    realize_overlay(sc);
    const mr_frame_desc &fr = fs->last_frame;
    const int ss_mode = fs->last_ss_mode;
    const bool draw = sc->ov_points != 0;
    if (draw) {
        if (sc->ov_width != fr.width || sc->ov_height != fr.height) return fail(MR_E_INVALID, "overlay lists were built for a frame of another size");
        if (int rc = sync_slot_overlay(sc, fs->ov, fs->stream, ss_mode != 0 && !fs->last_post)) return rc;
        launch_overlay(sc, fs->ov, fs->d_z.as<double>(), fs->d_frame.as<float>(), ss_mode || fs->last_post ? nullptr : d_out, fr.width, fr.height, fr.system, fs->stream);
    }
    if (fs->last_post) launch_post_resolve(sc, fs, fr, ss_mode, d_out);
    else launch_resolve(sc, fs->ov, fs->d_frame.as<float>(), fr, ss_mode, draw, d_out, fs->stream);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

// The fragment / pixel counts of a frame are left as per-tile partials by the tile kernel; they
// are summed and fetched only when somebody asks (mr_render, mr_get_stats).
int fetch_counters(FrameSlot *fs, bool reduce)
{
    using namespace mr;
    Counters *ctr = fs->ctr(fs->frames_enqueued - 1);
    // mr_render without a stats pointer only needs the overflow flags: no reduction launch
    if (reduce && !fs->stats_reduced && fs->last_n_tiles > 0) {
        hipLaunchKernelGGL(k_reduce_tile_stats, dim3(256), dim3(256), 0, fs->stream, fs->d_tile_stats.as<uint32_t>(),
                           fs->last_n_tiles, ctr, fs->last_full ? 1 : 0);
        fs->stats_reduced = true;
    }
    HIP_TRY(hipMemcpyAsync(fs->h_counters, ctr, sizeof(Counters), hipMemcpyDeviceToHost, fs->stream));
    HIP_TRY(hipMemcpyAsync(fs->h_sticky, fs->sticky(), sizeof(Sticky), hipMemcpyDeviceToHost, fs->stream));
    return MR_OK;
}

// After the stream has drained: turn counters + events into mr_stats; grow work lists on overflow.
int collect(mr_scene *sc, FrameSlot *fs, bool with_copy)
{
    const mr::Counters &c = *fs->h_counters;
    mr_stats &s = sc->stats;
    if (fs->last_frame.flags & MR_FRAME_COUNTERS) {
        s.frag_tri = (int64_t)c.frag_tri; s.frag_quad = (int64_t)c.frag_quad;
        s.covered_px = (int64_t)c.covered_px; s.lit_px = (int64_t)c.lit_px;
        s.stencil_updates = (int64_t)c.stencil_updates;
    } else {                                  // not counted: the frame was rendered without MR_FRAME_COUNTERS
        s.frag_tri = s.frag_quad = s.covered_px = s.lit_px = s.stencil_updates = -1;
    }
    s.n_faces = (int64_t)(sc->faces.size() / 12); s.n_faces_setup = c.n_valid_tris;
    s.n_quads = c.n_quads; s.n_quads_drawn = c.n_quads_drawn;
    s.tri_bin_entries = c.tri_bin_total; s.quad_bin_entries = c.bin_total - c.tri_bin_total;
    sc->n_silhouette = (int)c.n_quads;
    float ms = 0;
    const bool timed = !(fs->last_frame.flags & MR_FRAME_NO_TIMING);
    auto span = [&](int a, int b) { ms = 0; if (timed) (void)hipEventElapsedTime(&ms, fs->ev[a], fs->ev[b]); return ms; };
    const bool light = (fs->last_frame.flags & MR_FRAME_LIGHT_TIMING) != 0;
    s.gpu_ms_setup = light ? 0.f : span(0, 2); s.gpu_ms_binning = light ? span(0, 3) : span(2, 3);
    s.gpu_ms_tile = span(3, 4);
    s.gpu_ms_copy = with_copy && timed ? span(4, 5) : 0.f;
    s.gpu_ms_total = span(0, with_copy ? 5 : 4);
    // the verdicts of the last frame and of every frame of this slot since the host last looked (Sticky)
    mr::Sticky &st = *fs->h_sticky;
    const uint32_t overflow = c.overflow | st.overflow;
    uint32_t longest_stretch = 0;             // the work list is WORK_SHARDS stretches: the fullest one decides what it needs
    for (const auto &w : c.work) longest_stretch = std::max(longest_stretch, w.n);
    const uint32_t n_work = std::max(longest_stretch * (uint32_t)mr::WORK_SHARDS, st.n_work), n_quads = std::max(c.n_quads, st.n_quads);
    const uint32_t n_quads_drawn = std::max(c.n_quads_drawn, st.n_quads_drawn);
    bool grown = false;
    if (overflow) {
        for (int cls = 0; cls < mr::BIN_CLASSES; ++cls)
            if (overflow & (1u << cls)) {
                const uint32_t longest = std::max(c.max_list[cls], st.max_list[cls]);
                uint32_t want = std::max(longest + longest / 2, fs->bin_cap[cls] * 2);
                uint32_t cap = 64;
                while (cap < want) cap <<= 1;
                sc->bin_cap[cls] = std::max(sc->bin_cap[cls], cap);
            }
        if (overflow & 8u) sc->work_cap = std::max(sc->work_cap, n_work + n_work / 2 + 1024);
        if (overflow & 16u) sc->quad_cap = std::max(sc->quad_cap, std::max(n_quads_drawn + n_quads_drawn / 2 + 64, fs->quad_cap * 2));
        grown = true;
    }
    if (n_quads > fs->quad_cap) { sc->quad_cap = std::max(sc->quad_cap, n_quads + n_quads / 2 + 64); grown = true; }
    if (grown) {
        // acted on: the device's record and the last frame's block start clean (stream order puts this in front of
        // the slot's next frame, whose tile kernel would fold that block into the record again)
        (void)hipMemsetAsync(fs->ctr(fs->frames_enqueued - 1), 0, sizeof(mr::Counters), fs->stream);
        (void)hipMemsetAsync(fs->sticky(), 0, sizeof(mr::Sticky), fs->stream);
        st = mr::Sticky{};
    }
    return grown ? MR_E_OVERFLOW : MR_OK;
}

// What mr_render and mr_render_async do on the slot's stream: the frame, the host's share of its overlay (beside the
// device's kernels), the counters (summed only if somebody reads them: `reduce`), the copy to the caller's rows, mark 5.
int render_and_copy(mr_scene *sc, FrameSlot *fs, const mr_frame_desc *fr, uint8_t *out_rgb, bool reduce)
{
    const size_t band_bytes = out_bytes(fr);
    HIP_TRY(fs->d_out.ensure(band_bytes));
    int rc;
    if ((rc = enqueue_frame(sc, fs, fr, fs->d_out.as<uint8_t>(), true))) return rc;
    if ((rc = finish_overlay(sc, fs, fs->d_out.as<uint8_t>()))) return rc;
    if ((rc = fetch_counters(fs, reduce))) return rc;
    HIP_TRY(hipMemcpyAsync(out_rgb, fs->d_out.p, band_bytes, hipMemcpyDeviceToHost, fs->stream));
    if (!(fr->flags & MR_FRAME_NO_TIMING)) { HIP_TRY(hipEventRecord(fs->ev[5], fs->stream)); fs->last_copied = true; }
    return MR_OK;
}

}  // namespace
