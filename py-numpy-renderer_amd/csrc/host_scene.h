// host_scene.h -- the static scene: what the caller's models become on the host (concatenated arrays, the unique-edge
// table, the cluster records), their device copies, and commit(), which brings the device up to date.
#pragma once

namespace {

struct FrameSlot;      // host_frame.h

struct EdgeKey {
    uint64_t key;      // (lo << 32) | hi of the two global vertex indices
    uint32_t inc;      // face * 4 + corner
};

// What the next pose pass (host_pose.h) has to redo, as bits of mr_scene::pose_dirty: vertices and what is built from
// them; the whole normals' part; k_skin_normals alone (new bones); k_morph_normals alone (new weights)
enum PoseDirty : uint8_t { POSE_GEOM = 1, POSE_NORMALS = 2, POSE_SKIN_N = 4, POSE_MORPH_N = 8 };

// Timing marks of one part of the pose pass: events on the library's stream, created when first recorded, round SPANS
// kernels.  Span k lies between marks k * STRIDE and k * STRIDE + 1: consecutive marks, each the end of one span and the
// start of the next, with STRIDE 1; a pair of its own per kernel with STRIDE 2.
template <int SPANS, int STRIDE>
struct PassMarks {
    hipEvent_t ev[(SPANS - 1) * STRIDE + 2] = {};
    bool seen = false;                        // a pass has come this way: until then there is nothing to read
    bool ran[SPANS] = {};                     // the last pass launched span k's kernel
    void none_ran() { for (bool &r : ran) r = false; }
    int mark(int i)
    {
        if (!ev[i]) HIP_TRY(hipEventCreate(&ev[i]));
        HIP_TRY(hipEventRecord(ev[i], g_stream));
        return MR_OK;
    }
    int read(float *out_ms, const char *none_yet) const
    {
        if (!seen) return fail(MR_E_INVALID, none_yet);
        for (int k = 0; k < SPANS; ++k) {
            out_ms[k] = 0.f;                  // (a kernel the last pass did not launch: not the empty span between two marks)
            if (ran[k]) HIP_TRY(hipEventElapsedTime(&out_ms[k], ev[k * STRIDE], ev[k * STRIDE + 1]));
        }
        return MR_OK;
    }
    void release() { for (hipEvent_t &e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; } }
};

}  // namespace

struct mr_scene {
    // ---- host staging of the static scene (concatenated over models, indices made global)
    std::vector<double> verts;
    std::vector<float> uv, normals;
    std::vector<int32_t> faces;
    std::vector<uint8_t> face_flags;
    std::vector<mr::Material> materials;
    std::vector<mr::Texture> textures;       // device pointers
    std::vector<void *> texture_allocs;
    std::vector<int32_t> model_face_off;      // first face of every model
    std::vector<int32_t> edge_ids;            // per face corner: raw vertex identity for silhouette edges (made unique per model)
    std::vector<int32_t> edge_raw;            // the same as the caller passed it (for mr_read_silhouette)
    std::vector<mr::EdgeRec> edges;           // unique undirected edges, scrambled order
    std::vector<uint32_t> edge_inc;           // incidences beyond an edge's first two
    bool dirty = true;
    // a model's place in the arrays above and its pose (mr_scene_set_model_pose; host_pose.h)
    struct ModelPose {
        int32_t vert_off = 0, n_verts = 0;
        bool verts_f32 = false;               // as the caller passed it: a posed model's faces lose FF_VERTS_F32
        bool posed = false;
        bool on_device = false;               // d_verts holds posed vertices in this model's range
        double m[16] = {};
        // the normal matrix (mr_scene_set_model_pose_normals): the model's vertex normals (an OBJ file counts its vn
        // apart from its v) and its materials' object-space normal maps follow the pose
        int32_t normal_off = 0, n_normals = 0, mat_off = 0, n_mats = 0;
        bool has_g = false;
        bool normals_on_device = false;       // d_normals holds transformed normals in this model's range
        bool maps_on_device = false;          // this model's materials point at re-baked copies of their maps
        double g[9] = {};
        // the skin (mr_scene_set_model_skin): joints and weights per vertex, the owner of every normal (empty: the
        // normals stay), kept on the host and uploaded once per skin; and the bones (mr_scene_set_model_bones), which
        // make the model move: "has bones" is to the pass what "posed" is
        std::vector<int32_t> joints, owners;
        std::vector<double> weights, bones;
        int32_t n_bones = 0;                  // > 0: the model has a skin
        bool has_bones = false;
        int32_t table_off = 0, owner_off = 0; // where the model's rows start in d_skin_joints / d_skin_weights, d_skin_owners
        // the morph (mr_scene_set_model_morph): the per-vertex contribution lists of its targets (host_morph.h), for the
        // vertices and, where the caller passed some, for the normals, built on the host once per morph and uploaded with
        // every other model's; and the weights (mr_scene_set_model_morph_weights), which make the model move
        mr_morph::Lists morph_v, morph_n;
        int32_t n_targets = 0;                // > 0: the model has a morph
        bool has_weights = false;
        std::vector<double> morph_w;
        int32_t slice0_v = 0, slice0_n = 0;   // where the model's slices start in d_morph_slices
        bool verts_m_morphed = false;         // d_verts_m differs from d_verts0 in this model's range
        bool normals_m_morphed = false;       // ... d_normals_m from d_normals0
        // the flag of mr_scene_set_model_auto_normals and the per-normal face lists (host_autonormals.h), built when the
        // flag is first on, dropped by commit() and built again by the next pass that needs them
        bool auto_on = false;
        mr_autonormals::Lists auto_lists;
        int32_t auto_slice0 = 0;              // where the model's slices start in d_auto_slices
        bool moved() const { return posed || has_bones || has_weights; }                   // d_verts differs from d_verts0
        bool auto_normals() const { return auto_on && n_normals > 0 && moved(); }          // d_normals is rebuilt from d_verts: none of the other three writes it
        bool skin_normals() const { return has_bones && !owners.empty() && n_normals > 0 && !auto_normals(); }  // ... d_normals from d_normals0 by the skin
        bool morph_normals() const { return has_weights && morph_n.n > 0 && n_normals > 0 && !auto_normals(); } // ... or by the morph
    };
    std::vector<ModelPose> poses;             // one per model
    bool skin_tables_dirty = false;           // a skin was set or removed: the device tables are rebuilt by the next pass
    int32_t skin_bones = 0, skin_written = 0, skin_normals_written = 0;     // mr_debug_skin
    bool morph_tables_dirty = false;          // a morph was set or removed: the device lists are rebuilt by the next pass that needs them
    int32_t morph_targets = 0, morph_written = 0, morph_normals_written = 0, morph_entries = 0;   // mr_debug_morph
    bool auto_tables_dirty = false;           // a model's lists were built, or the scene was committed: the device lists (of every model that holds some) are rebuilt by the next pass that needs them
    int32_t auto_models = 0, auto_written = 0, auto_entries = 0, auto_kept_waves = 0;   // mr_debug_auto_normals (the kept count is summed from d_auto_kept when asked for)
    uint8_t pose_dirty = 0;                   // PoseDirty bits: what the setters and commit() left for apply_poses()
    int32_t commits = 0, pose_passes = 0, pose_written = 0;      // mr_debug_pose

    // ---- device copies of the static scene
    DevBuf d_verts, d_uv, d_normals, d_faces, d_face_flags, d_materials, d_textures, d_edges, d_edge_inc, d_face_n;
    DevBuf d_edges32;                        // the compact edge table, when the scene allows it
    bool edge_compact = false;
    DevBuf d_face_pos, d_face_attr;          // static per face (rast_types.h, FacePosT / FaceAttr), built by commit()
    DevBuf d_clusters;                       // static per 64 faces (rast_types.h, ClusterRec), built by commit()
    int32_t n_clusters = 0;
    // the pose pass: the vertices as the caller passed them (d_verts holds what the kernels read) and the pass's two tables
    DevBuf d_verts0, d_pose_rows, d_pose_blocks;
    bool verts0_valid = false;
    PassMarks<MR_N_POSE_TIMES, 1> marks_pose;             // six marks round the vertex kernels and the four rebuilds of the last pass over faces
    // the same for normal matrices: the normals as the caller passed them, the tables of k_pose_normals and
    // k_pose_texels, and the re-baked copies of object-space normal maps, one after the other
    DevBuf d_normals0, d_normal_rows, d_normal_blocks, d_texel_rows, d_texel_blocks, d_rebaked;
    bool normals0_valid = false;
    PassMarks<MR_N_POSE_NORMALS_TIMES, 1> marks_normals;  // three marks round the two kernels of the last pass that launched one of them
    // the skin: joints (int4), weights (double4) and normal owners of the skinned models, one after the other; the bone
    // table of the last pass (its host copy lives until the pass has waited for the stream) and the two kernels' tables
    DevBuf d_skin_joints, d_skin_weights, d_skin_owners, d_bones, d_skin_rows, d_skin_blocks, d_skin_n_rows, d_skin_n_blocks;
    std::vector<double> bone_table;
    PassMarks<MR_N_SKIN_TIMES, 2> marks_skin;             // k_skin_vertices, k_skin_normals
    // the morphs: the sliced contribution lists of every model that has a morph, one after the other (the slice table,
    // then four planes: target, delta x / y / z); the weight table of the last pass and the two kernels' tables; and the
    // copies of d_verts0 / d_normals0 in which the morphed models' ranges hold the morphed arrays: what the skin and pose
    // kernels take as their pristine source while they exist
    DevBuf d_morph_slices, d_morph_target, d_morph_dx, d_morph_dy, d_morph_dz, d_morph_weights;
    DevBuf d_morph_rows, d_morph_blocks, d_morph_n_rows, d_morph_n_blocks, d_verts_m, d_normals_m;
    bool verts_m_valid = false, normals_m_valid = false;
    std::vector<double> morph_weight_table;
    PassMarks<MR_N_MORPH_TIMES, 2> marks_morph;           // k_morph_vertices, k_morph_normals
    // rebuilt normals: the sliced face lists of every model whose flag is on, one after the other (the slice table and
    // one plane of faces), the kernel's two tables and its per-wavefront counts of normals that kept their value
    DevBuf d_auto_slices, d_auto_faces, d_auto_rows, d_auto_blocks, d_auto_kept;
    PassMarks<1, 2> marks_auto;                           // k_auto_normals
    bool pos32 = false;                     // d_face_pos holds FacePos32 (every model's vertices are float32)
    bool has_no_depth = false;               // some model has depth_test == False (what a frame asks once per scene, not once per frame)
    bool force_full = false;                 // mr_debug_force_full: every frame takes the general kernels (FramePlan::full)
    DevBuf d_sky;                            // cubemap texels, uint8 (6, S, S, 3)
    DevBuf d_gamma;                          // GAMMA_LUT_SIZE float32 thresholds of the finalise step function
    int32_t sky_size = 0;

    // ---- debug-frustum overlay: the lines' points as built on the host (five targets and a depth per point, segment by
    // segment); every frame slot keeps its own device copy (FrameSlot::ov), brought up to date when a frame of that
    // slot draws the overlay
    int32_t ov_height = 0, ov_width = 0;     // the frame the lists were built for
    int32_t ov_points = 0, ov_segments = 0;
    uint64_t ov_serial = 0;                  // bumped whenever the lists change
    std::vector<int32_t> ov_target;          // (5, n_points) pixel row * width + col of every target
    std::vector<double> ov_z;
    std::vector<int32_t> ov_seg;             // first point, number of points per segment (| OVERLAY_SEG_GLOBAL: mark_global_segments)
    std::vector<uint8_t> ov_tile_mask;       // the 16x16 tiles that hold a target
    // mr_scene_set_overlay_cameras only leaves its arguments here; the lists are built when first needed (realize_overlay)
    // -- for mr_render / mr_render_async AFTER the frame's three kernels have been launched, so that the host walks the
    // lines while the device renders (the lists' only early use, the tile kernel's tap mask, is given up for that frame)
    struct OvPending {
        bool set = false;
        double corners[32], planes[24], mvp[16], viewport[16], near_ = 0, far_ = 0;
        int32_t inside = 0, height = 0, width = 0;
    } ov_pending;
    // the same targets as slots of the list of touched pixels, for a frame assembled from several devices (built
    // when first asked for: build_overlay_slots)
    std::vector<int32_t> ov_slot_of, ov_touched;
    uint64_t ov_slots_serial = 0;            // the ov_serial the slot lists were built for
    mr_host::OverlaySlotWork ov_slot_work;
    mr_host::OverlayCountWork ov_count_work;

    // ---- lanes of mr_render_async: a stream of the library's own each, and what is in flight on it
    struct Lane { hipStream_t stream = nullptr; bool busy = false; } lanes[MR_ASYNC_LANES];

    // ---- the accumulation (host_accum.h): the weighted sum of the sub-frames added so far, on their sample grid.  It is
    // the scene's, not a slot's: frames rendered in between leave it alone, and so does mr_scene_clear
    struct Accum {
        DevBuf d_acc;                         // float32 (height, width, 3), rows bottom-up; kept from one accumulation to the next
        int32_t width = 0, height = 0, ss_flags = 0;      // fixed by the first add
        int32_t count = 0, rerendered = 0;    // sub-frames added; sub-frames rendered again after an overflow
        Marks<4> marks;                       // round the last k_accum_add and the last k_accum_resolve
        bool add_marked = false, resolve_marked = false;
    } accum;

    // ---- the passes behind a frame's tile kernel (host_pass.h, PassRecord): ambient obscurance (host_ao.h) and depth of
    // field (host_dof.h), marked round their one kernel ...
    struct Ao : PassRecord<2> { mr::AoParams params = {}; } ao;
    struct Dof : PassRecord<2> { mr::DofParams params = {}; } dof;
    // ... bloom (host_bloom.h), marked in front of its down chain, behind it, behind the up chain and behind the composite
    struct Bloom : PassRecord<4> { mr::BloomParams params = {}; int32_t last_levels = 0; } bloom;      // (the levels of the last frame enqueued)
    // ... light shafts (host_shafts.h), marked in front of the source, behind it, behind the march and behind the composite
    struct Shafts : PassRecord<4> { mr::ShaftsParams params = {}; int32_t last_levels = 0; } shafts;   // (likewise)

    // ... tone mapping (host_tonemap.h), marked in front of k_lum_hist, behind it, behind k_exposure and behind k_tone_apply.
    // The previous exposure is the scene's, not a slot's, and only an adaptive scene has one: two cells, `cur` the one the
    // last frame whose mr_render or mr_render_wait returned MR_OK left (valid), the other the one a frame in flight is
    // writing (pending, on pending_slot) -- the hand-over rule of the temporal anti-aliasing's history
    struct Tone : PassRecord<4> {
        mr::ToneParams params = {};
        DevBuf d_state;
        int cur = 0;
        bool valid = false;
        bool pending = false;
        const FrameSlot *pending_slot = nullptr;
        uint64_t epoch = 0, pending_epoch = 0;    // + 1 whenever the exposure is forgotten: a frame issued before that hands nothing over
        int32_t adopted = 0, last_grid = 0;       // exposures handed over; the workgroups of the last k_lum_hist (mr_debug_tone_map)
    } tone;

    // ... the data layers (host_layers.h), marked round k_layers: the description every frame takes a copy of, and the
    // models' first faces on the device, uploaded once per commit
    struct Layers : PassRecord<2> {
        mr::LayersParams params = {};
        DevBuf d_face_off;
        int32_t table_commits = -1, last_mask = 0;    // the commit the table was uploaded for; the mask of the last frame enqueued
    } layers;

    // ... and motion blur (host_motion.h), marked in front of k_velocity, behind it, behind k_velocity_faces in a frame that
    // ran the per-face pass, and behind k_mblur; the tables are the class matrices, the background's, the models' first
    // faces and their classes as one block (motion_params)
    struct Motion : PassRecord<4> {
        mr::MotionParams params = {};
        std::vector<double> tables;
        int blur_from = 1;                    // the mark k_mblur's span starts at: 2 in a frame that ran the per-face pass; set with the marks
        bool vel_skipped = false;             // the last frame's U was the temporal anti-aliasing's: no k_velocity of its own
    } motion;

    // ---- temporal anti-aliasing (host_taa.h), marked in front of its k_velocity, behind it (and behind the per-face pass
    // where that ran) and behind k_taa.  `tables` is the velocity's block, laid out as the motion blur's.  The history is
    // the scene's, not a slot's: two float frames on the sample grid, `cur` the one the last frame whose mr_render or
    // mr_render_wait returned MR_OK left (valid), the other the one a frame in flight is writing (pending, on pending_slot)
    struct Taa : PassRecord<3> {
        mr::TaaParams params = {};
        mr::MotionParams vel = {};
        std::vector<double> tables;
        DevBuf d_hist[2];
        int cur = 0;
        bool valid = false;
        int32_t hist_rows = 0, hist_cols = 0;
        bool pending = false;
        const FrameSlot *pending_slot = nullptr;
        int32_t pending_rows = 0, pending_cols = 0;
        uint64_t epoch = 0, pending_epoch = 0;    // + 1 whenever the history is forgotten: a frame issued before that adopts nothing
        int32_t velocities = 0, adopted = 0;      // k_velocity launches in front of k_taa; histories adopted (mr_debug_taa)
    } taa;

    // ---- the velocity of models that bend (host_motion_faces.h): the description every frame with motion blur reads, the
    // snapshot of the vertices as the previous pass left them and the serial of the states d_verts has held
    struct MotionFaces {
        bool on = false;
        double s_now[12] = {}, s_prev[12] = {};
        std::vector<int32_t> deforming;       // per model: its samples take the per-face velocity
        int64_t prev_serial = -1;             // the vertex serial of the previous frame, as its caller saw it
        int32_t ran = 0, skipped = 0, records = 0, snapshots = 0;      // mr_debug_motion_faces
        Marks<3> marks;                       // in front of k_face_homography, between the two kernels, behind k_velocity_faces
        bool marked = false;
    } mfaces;
    bool track_verts = false;                 // mr_scene_track_vertices
    int64_t vert_serial = 0;                  // + 1 for every commit that uploads vertices and every pass that rewrites them
    DevBuf d_verts_prev;                      // d_verts as it was before the last such pass, while tracking is on
    bool snap_valid = false;
    int64_t snap_serial = -1, snap_verts = 0; // the serial of the state d_verts_prev holds; its vertices

    // ---- frame slots, one per stream that has rendered this scene
    std::vector<std::unique_ptr<FrameSlot>> slots;
    FrameSlot *last = nullptr;               // slot of the most recently enqueued frame
    uint64_t frame_serial = 0;               // frames enqueued on any stream
    mr_stats stats = {};
    int n_silhouette = 0;
    SilCache sil;
    // lights 1.. of the frames to come (mr_scene_set_extra_lights); light 0 is the frame descriptor's
    int n_extra_lights = 0;
    mr::LightRec extra_lights[mr::MAX_LIGHTS - 1] = {};
    // Capacities of the per-frame work lists, shared by all slots: what one frame learnt (a tile with
    // a longer list, more silhouette edges) holds for the frames rendered on other streams too.
    uint32_t bin_cap[mr::BIN_CLASSES] = { 512u, 128u, 256u };   // entries per tile and class
    uint32_t work_cap = 1u << 18, quad_cap = 0;
    void reset_caps() { bin_cap[0] = 512u; bin_cap[1] = 128u; bin_cap[2] = 256u; work_cap = 1u << 18; quad_cap = 0; }
};

namespace {

// Unique undirected edges with their incident (face, corner) pairs in face order: what the
// reference's per-model set of Edge objects (obj/triangular.py:286-302) reduces to.  An edge is
// identified by the RAW vertex ids of its corners (mr_model_desc.edge_ids), as in the reference.
// The table is stored in a scrambled order (sorted by a hash of the edge): silhouettes run along
// consecutive vertex indices, and a wavefront of k_setup that found dozens of silhouette edges
// among its 64 would set their quads up four at a time while the rest of the device idles.
void build_edge_table(mr_scene *sc)
{
    const size_t nf = sc->faces.size() / 12;
    std::vector<EdgeKey> keys;
    keys.reserve(nf * 3);
    for (size_t f = 0; f < nf; ++f) {
        const int32_t *id = &sc->edge_ids[f * 3];
        for (int k = 0; k < 3; ++k) {
            uint32_t a = (uint32_t)id[k], b = (uint32_t)id[(k + 1) % 3];
            uint32_t lo = std::min(a, b), hi = std::max(a, b);
            keys.push_back({ ((uint64_t)lo << 32) | hi, (uint32_t)(f * 4 + k) });
        }
    }
    auto scramble = [](uint64_t k) {                   // splitmix64 finaliser: a bijection
        k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull; k ^= k >> 27; k *= 0x94d049bb133111ebull; k ^= k >> 31;
        return k;
    };
    for (EdgeKey &e : keys) e.key = scramble(e.key);
    std::sort(keys.begin(), keys.end(), [](const EdgeKey &x, const EdgeKey &y) {
        return x.key != y.key ? x.key < y.key : x.inc < y.inc;
    });
    sc->edges.clear();
    sc->edge_inc.clear();
    for (size_t i = 0; i < keys.size();) {
        size_t j = i;
        while (j < keys.size() && keys[j].key == keys[i].key) ++j;
        mr::EdgeRec r;
        std::memset(&r, 0, sizeof r);
        r.inc[0] = keys[i].inc;
        r.inc[1] = j - i > 1 ? keys[i + 1].inc : 0xffffffffu;
        r.extra_off = (uint32_t)sc->edge_inc.size();
        r.extra_cnt = j - i > 2 ? (uint32_t)(j - i - 2) : 0u;
        for (size_t k = i + 2; k < j; ++k) sc->edge_inc.push_back(keys[k].inc);
        sc->edges.push_back(r);
        i = j;
    }
}

// Finalise is uint8(frame ** 0.8 * 255) in float32 (obj/core.py:640): a monotone step function
// of the colour with 255 steps.  GAMMA_LUT[k] is the smallest float32 in [0, 1] whose step is
// >= k, found by bisection over the bit patterns against the host's own powf, so that k_shade
// can place a colour with one approximate exp2/log2 and two table compares and still return
// exactly what powf would (k_shade's gamma_u8).
std::vector<float> gamma_thresholds()
{
    auto step = [](float x) { return (int)(uint8_t)(powf(x, 0.8f) * 255.0f); };
    std::vector<float> lut(mr::GAMMA_LUT_SIZE);
    lut[0] = 0.0f;
    for (int k = 1; k < 256; ++k) {
        uint32_t lo = 0, hi = 0x3f800000u;      // step(0) = 0 < k <= 255 = step(1)
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            float x;
            memcpy(&x, &mid, 4);
            if (step(x) >= k) hi = mid; else lo = mid;
        }
        memcpy(&lut[k], &hi, 4);
    }
    lut[256] = INFINITY;
    return lut;
}

// The static cluster records (rast_types.h, ClusterRec): bounding box and normal cone of every 64 consecutive faces.
std::vector<mr::ClusterRec> build_clusters(const mr_scene *sc)
{
    const size_t nf = sc->faces.size() / 12, nc = (nf + mr::CLUSTER_FACES - 1) / mr::CLUSTER_FACES;
    std::vector<mr::ClusterRec> out(nc);
    auto down = [](double x) { float f = (float)x; return (double)f > x ? std::nextafter(f, -INFINITY) : f; };
    auto up = [](double x) { float f = (float)x; return (double)f < x ? std::nextafter(f, INFINITY) : f; };
    for (size_t c = 0; c < nc; ++c) {
        mr::ClusterRec r;
        std::memset(&r, 0, sizeof r);
        double lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY }, sum[3] = { 0, 0, 0 };
        bool boxed = true, coned = true;
        const size_t f0 = c * mr::CLUSTER_FACES, f1 = std::min(nf, f0 + mr::CLUSTER_FACES);
        std::vector<std::array<double, 3>> normals;
        normals.reserve(f1 - f0);
        for (size_t f = f0; f < f1; ++f) {
            const double *v[3];
            for (int k = 0; k < 3; ++k) {
                v[k] = &sc->verts[(size_t)sc->faces[f * 12 + k * 4] * 4];
                if (!(v[k][3] == 1.0)) boxed = false;                     // (a homogeneous coordinate other than 1: no box)
                for (int j = 0; j < 3; ++j) { lo[j] = std::min(lo[j], v[k][j]); hi[j] = std::max(hi[j], v[k][j]); if (!std::isfinite(v[k][j])) boxed = false; }
            }
            const double a[3] = { v[1][0] - v[0][0], v[1][1] - v[0][1], v[1][2] - v[0][2] };
            const double b[3] = { v[2][0] - v[0][0], v[2][1] - v[0][1], v[2][2] - v[0][2] };
            double n[3] = { a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0] };
            const double l = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            if (!(l > 0) || !std::isfinite(l)) { coned = false; continue; }
            for (int j = 0; j < 3; ++j) { n[j] /= l; sum[j] += n[j]; }
            normals.push_back({ n[0], n[1], n[2] });
        }
        if (boxed) {
            for (int j = 0; j < 3; ++j) { r.lo[j] = down(lo[j]); r.hi[j] = up(hi[j]); }
        } else {
            for (int j = 0; j < 3; ++j) { r.lo[j] = NAN; r.hi[j] = NAN; }      // never culled: every comparison fails
        }
        r.cos_half = -2.f; r.sin_half = 1.f;
        const double sl = std::sqrt(sum[0] * sum[0] + sum[1] * sum[1] + sum[2] * sum[2]);
        if (coned && sl > 1e-6 * (double)(f1 - f0)) {
            double least = 1.0;
            for (const auto &n : normals) least = std::min(least, (n[0] * sum[0] + n[1] * sum[1] + n[2] * sum[2]) / sl);
            least -= 1e-6;
            if (least > 0.05) {                                             // a cone wider than ~87 degrees never culls anything
                for (int j = 0; j < 3; ++j) r.axis[j] = (float)(sum[j] / sl);
                // the axis as stored (float32) is not the axis the dots were taken with: 1e-6 covers it
                r.cos_half = (float)(least - 1e-6);
                r.sin_half = (float)std::min(1.0, std::sqrt(std::max(0.0, 1.0 - (double)r.cos_half * (double)r.cos_half)) + 1e-6);
            }
        }
        out[c] = r;
    }
    return out;
}

// the thresholds on the device, uploaded once per scene (commit; mr_debug_post on a scene that never committed)
int ensure_gamma(mr_scene *sc)
{
    if (sc->d_gamma.p) return MR_OK;
    const std::vector<float> lut = gamma_thresholds();
    HIP_TRY(sc->d_gamma.ensure(lut.size() * sizeof(float)));
    HIP_TRY(hipMemcpy(sc->d_gamma.p, lut.data(), lut.size() * sizeof(float), hipMemcpyHostToDevice));
    return MR_OK;
}

int commit(mr_scene *sc)
{
    if (!sc->dirty) return MR_OK;
    HIP_TRY(hipDeviceSynchronize());          // no frame may still be reading the old arrays
    sc->sil.drop();                           // the silhouette belongs to the geometry that is about to be replaced
    if (int rc = ensure_gamma(sc)) return rc;
    build_edge_table(sc);
    for (mr::Material &m : sc->materials) {
        const mr::Texture none = { nullptr, 0, 0 };
        auto header = [&](int32_t id) { return id >= 0 && id < (int32_t)sc->textures.size() ? sc->textures[id] : none; };
        m.map_kd = header(m.tex_kd); m.map_norm = header(m.tex_norm); m.map_ks = header(m.tex_ks);
    }
    int rc = MR_OK;
    auto up = [&](DevBuf &buf, const auto &v) { if (!rc) rc = upload(buf, v, g_stream); };
    up(sc->d_verts, sc->verts); up(sc->d_uv, sc->uv); up(sc->d_normals, sc->normals); up(sc->d_faces, sc->faces);
    up(sc->d_face_flags, sc->face_flags); up(sc->d_materials, sc->materials); up(sc->d_textures, sc->textures);
    up(sc->d_edges, sc->edges); up(sc->d_edge_inc, sc->edge_inc);
    if (rc) return rc;
    // static per scene: the faces' unit normals (light-facing test), copied into the edge records
    const int nf = (int)(sc->faces.size() / 12), ne = (int)sc->edges.size();
    HIP_TRY(sc->d_face_n.ensure(std::max<size_t>((size_t)nf * 4 * sizeof(double), 16)));
    if (nf > 0)
        hipLaunchKernelGGL(mr::k_face_normals, dim3((nf + 255) / 256), dim3(256), 0, g_stream, nf, sc->d_faces.as<int32_t>(),
                           sc->d_face_flags.as<uint8_t>(), sc->d_verts.as<double>(), sc->d_face_n.as<double>());
    if (ne > 0)
        hipLaunchKernelGGL(mr::k_edge_normals, dim3((ne + 255) / 256), dim3(256), 0, g_stream, ne, sc->d_edges.as<mr::EdgeRec>(),
                           sc->d_face_n.as<double>());
    // the static face records: float32 corners when every model's vertices are float32
    sc->pos32 = true;
    sc->has_no_depth = false;
    for (uint8_t ff : sc->face_flags) {
        if (!(ff & mr::FF_VERTS_F32)) sc->pos32 = false;
        if (ff & mr::FF_NO_DEPTH) sc->has_no_depth = true;
    }
    HIP_TRY(sc->d_face_pos.ensure(std::max<size_t>((size_t)nf * (sc->pos32 ? sizeof(mr::FacePos32) : sizeof(mr::FacePos64)), 16)));
    HIP_TRY(sc->d_face_attr.ensure(std::max<size_t>((size_t)nf * sizeof(mr::FaceAttr), 16)));
    {
        const std::vector<mr::ClusterRec> clusters = build_clusters(sc);
        sc->n_clusters = (int32_t)clusters.size();
        HIP_TRY(sc->d_clusters.ensure(std::max<size_t>(clusters.size() * sizeof(mr::ClusterRec), 64)));
        if (!clusters.empty())
            HIP_TRY(hipMemcpyAsync(sc->d_clusters.p, clusters.data(), clusters.size() * sizeof(mr::ClusterRec), hipMemcpyHostToDevice, g_stream));
        HIP_TRY(hipStreamSynchronize(g_stream));            // (the vector goes out of scope)
    }
    auto face_static = [&](auto kernel, auto *face_pos) {
        hipLaunchKernelGGL(kernel, dim3((nf + 255) / 256), dim3(256), 0, g_stream, nf, sc->d_faces.as<int32_t>(), sc->d_face_flags.as<uint8_t>(),
                           sc->d_verts.as<double>(), sc->d_uv.as<float>(), sc->d_normals.as<float>(), face_pos, sc->d_face_attr.as<mr::FaceAttr>());
    };
    if (nf > 0 && sc->pos32) face_static(mr::k_face_static<float>, sc->d_face_pos.as<mr::FacePos32>());
    else if (nf > 0) face_static(mr::k_face_static<double>, sc->d_face_pos.as<mr::FacePos64>());
    // compact edge records when every model's vertices are float32 and no edge has more than two faces
    sc->edge_compact = ne > 0 && sc->edge_inc.empty() && sc->pos32;
    if (sc->edge_compact) {
        HIP_TRY(sc->d_edges32.ensure((size_t)ne * sizeof(mr::EdgeRec32)));
        hipLaunchKernelGGL(mr::k_edge_compact, dim3((ne + 255) / 256), dim3(256), 0, g_stream, ne, sc->d_edges.as<mr::EdgeRec>(),
                           sc->d_edges32.as<mr::EdgeRec32>());
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g_stream));
    sc->dirty = false;
    // d_verts holds the vertices as they were passed: the poses are applied next (apply_poses)
    sc->commits += 1;
    sc->vert_serial += 1;                     // (another state of d_verts: host_motion_faces.h)
    sc->verts0_valid = false;
    sc->normals0_valid = false;               // (and the normals and the materials' map headers)
    sc->verts_m_valid = sc->normals_m_valid = false;
    for (mr_scene::ModelPose &mp : sc->poses) {
        mp.on_device = mp.normals_on_device = mp.maps_on_device = false;
        mp.verts_m_morphed = mp.normals_m_morphed = false;
        mp.auto_lists.clear();                // (the face lists belong to the committed faces)
        if (mp.auto_on) sc->auto_tables_dirty = true;
        if (mp.moved()) sc->pose_dirty |= POSE_GEOM;
        if (mp.has_g || mp.skin_normals() || mp.morph_normals()) sc->pose_dirty |= POSE_NORMALS;
    }
    return MR_OK;
}

}  // namespace
