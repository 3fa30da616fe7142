// host_pose.h -- the pose pass: what the setters of a model's morph, skin, pose, normal matrix and auto-normals flag leave
// to be done is done on the device, in front of the frame.  d_verts / d_normals are what a frame's kernels read, d_verts0 /
// d_normals0 the arrays as the caller passed them.  A model "moves" while it has weights on its morph, bones on its skin
// or a pose; its vertices are morph -> skin -> pose of the pristine ones (k_morph_vertices into d_verts, or into the held
// copy d_verts_m where a skin or a pose follows; k_skin_vertices applies the pose behind it itself), its normals come
// from k_morph_normals (d_normals_m likewise), k_skin_normals or k_pose_normals -- or, flagged, from k_auto_normals
// alone; k_pose_texels re-bakes object-space normal maps into d_rebaked.  A model back at rest gets its ranges back.
// What a commit builds from positions is rebuilt where it lives; the silhouette cache goes with the geometry.
//
// apply_poses() runs where commit() runs, right after it: plan_pass() fills a PosePlan, run_pass() is the steps in order,
// each switched by the plan -- refuse float32 face records; wait for the device (frames in flight read the records about
// to be rewritten); while vertex tracking is on, the snapshot of d_verts (host_motion_faces.h); morph tables and weights;
// apply_morph_normals; apply_pose_normals; skin tables and bones; apply_skin_normals; move_vertices (restores, mark 0, morph, pose, skin); apply_auto_normals; rebuild_static; wait for
// the stream (the host side of every table, PassTables, lives until then) -- and the dirty bits are cleared, here alone.
//
// The dirty bits (PoseDirty, host_scene.h) and who sets them; mr_scene_clear clears them:
//     set_model_pose           GEOM; NORMALS when the pose goes and takes a normal matrix with it
//     set_model_pose_normals   NORMALS
//     set_model_skin, _morph   GEOM if the model moved; NORMALS if its normals followed the skin / the morph
//     set_model_bones          GEOM; NORMALS if its normals start or stop following the skin, else SKIN_N if they follow
//     set_model_morph_weights  GEOM; NORMALS if its normals start or stop following the morph, else, if they follow,
//                              MORPH_N and what takes the result: SKIN_N (the skin), else NORMALS (a normal matrix)
//     set_model_auto_normals   NORMALS if the model moves and has normals
//     moved_changed            (every setter that can start or stop a model) NORMALS for a flagged model with normals
//     commit()                 GEOM for a model that moves; NORMALS for one with a normal matrix or following normals
#pragma once

namespace {

int snapshot_vertices(mr_scene *sc);                 // host_motion_faces.h

// A model that moves (a pose, or bones on its skin) has float64 vertices -- the products of float64 matrices: when
// "moves" changes for a model passed as float32, its faces lose FF_VERTS_F32 or get it back, and the scene is left
// for commit() to rebuild
void moved_changed(mr_scene *sc, int32_t model, bool was)
{
    const mr_scene::ModelPose &mp = sc->poses[model];
    const bool now = mp.moved();
    // a model whose normals are rebuilt from its mesh (mr_scene_set_model_auto_normals) starts or stops doing so with
    // "moves": the whole normals' part, as for a model that starts or stops following a skin
    if (was != now && mp.auto_on && mp.n_normals > 0) sc->pose_dirty |= POSE_NORMALS;
    if (was == now || !mp.verts_f32) return;
    const size_t f0 = (size_t)sc->model_face_off[model];
    const size_t f1 = (size_t)model + 1 < sc->model_face_off.size() ? (size_t)sc->model_face_off[model + 1] : sc->face_flags.size();
    for (size_t f = f0; f < f1; ++f)
        sc->face_flags[f] = (uint8_t)(now ? sc->face_flags[f] & ~mr::FF_VERTS_F32 : sc->face_flags[f] | mr::FF_VERTS_F32);
    sc->dirty = true;
}

// mr_scene_set_model_pose behind its argument checks: the matrix is kept
void set_model_pose(mr_scene *sc, int32_t model, const double *m16)
{
    mr_scene::ModelPose &mp = sc->poses[model];
    if (!m16 && !mp.posed) return;
    if (m16 && mp.posed && !std::memcmp(mp.m, m16, sizeof mp.m)) return;
    const bool was = mp.moved();
    mp.posed = m16 != nullptr;
    if (m16) std::memcpy(mp.m, m16, sizeof mp.m);
    if (!mp.posed && mp.has_g) {                     // the normal matrix goes with the pose
        mp.has_g = false;
        sc->pose_dirty |= POSE_NORMALS;
    }
    moved_changed(sc, model, was);
    sc->pose_dirty |= POSE_GEOM;
}

// mr_scene_set_model_pose_normals behind its argument checks
void set_model_pose_normals(mr_scene *sc, int32_t model, const double *g9)
{
    mr_scene::ModelPose &mp = sc->poses[model];
    if (!g9 && !mp.has_g) return;
    if (g9 && mp.has_g && !std::memcmp(mp.g, g9, sizeof mp.g)) return;
    mp.has_g = g9 != nullptr;
    if (g9) std::memcpy(mp.g, g9, sizeof mp.g);
    sc->pose_dirty |= POSE_NORMALS;
}

// mr_scene_set_model_skin behind its argument checks: the tables are copied; a skin alone moves nothing
void set_model_skin(mr_scene *sc, int32_t model, const int32_t *joints, const double *weights, int32_t n_bones, const int32_t *owners)
{
    mr_scene::ModelPose &mp = sc->poses[model];
    if (!joints && mp.n_bones == 0) return;
    const bool was = mp.moved(), was_n = mp.skin_normals();
    const size_t n = (size_t)mp.n_verts * 4;
    mp.has_bones = false;                            // a new skin starts in the rest position; no skin, no bones
    mp.bones.clear();
    mp.joints.assign(joints ? joints : nullptr, joints ? joints + n : nullptr);
    mp.weights.assign(joints ? weights : nullptr, joints ? weights + n : nullptr);
    mp.owners.assign(joints && owners ? owners : nullptr, joints && owners ? owners + mp.n_normals : nullptr);
    mp.n_bones = joints ? n_bones : 0;
    sc->skin_tables_dirty = true;
    if (was) sc->pose_dirty |= POSE_GEOM;
    if (was_n) sc->pose_dirty |= POSE_NORMALS;
    moved_changed(sc, model, was);
}

// mr_scene_set_model_bones behind its argument checks
void set_model_bones(mr_scene *sc, int32_t model, const double *bones16)
{
    mr_scene::ModelPose &mp = sc->poses[model];
    const size_t n = (size_t)mp.n_bones * 16;
    if (!bones16 && !mp.has_bones) return;
    if (bones16 && mp.has_bones && !std::memcmp(mp.bones.data(), bones16, n * sizeof(double))) return;
    const bool was = mp.moved(), was_n = mp.skin_normals();
    mp.has_bones = bones16 != nullptr;
    mp.bones.assign(bones16 ? bones16 : nullptr, bones16 ? bones16 + n : nullptr);
    moved_changed(sc, model, was);
    sc->pose_dirty |= POSE_GEOM;
    // normals that follow the skin: new bones bring k_skin_normals alone, a model that starts or stops following
    // the whole normals' part (its normals come from another kernel, or from the pristine copy, then)
    if (was_n != mp.skin_normals()) sc->pose_dirty |= POSE_NORMALS;
    else if (was_n) sc->pose_dirty |= POSE_SKIN_N;
}

// mr_scene_set_model_morph behind its argument checks (the tables are checked: mr_morph::check_tables): the per-vertex
// lists are built and kept; a morph alone moves nothing
int set_model_morph(mr_scene *sc, int32_t model, int32_t n_targets, const int32_t *first, const int32_t *index, const double *delta,
                    const int32_t *nfirst, const int32_t *nindex, const double *ndelta)
{
    mr_scene::ModelPose &mp = sc->poses[model];
    if (!first && mp.n_targets == 0) return MR_OK;
    mr_morph::Lists v, n;
    if (first && !mr_morph::build_lists(mp.n_verts, n_targets, first, index, delta, v))
        return fail(MR_E_INVALID, "the morph's padded lists do not fit 32-bit offsets");
    if (first && nfirst && !mr_morph::build_lists(mp.n_normals, n_targets, nfirst, nindex, ndelta, n))
        return fail(MR_E_INVALID, "the morph's padded lists do not fit 32-bit offsets");
    const bool was = mp.moved(), was_n = mp.morph_normals();
    mp.has_weights = false;                          // a new morph starts in the rest shape; no morph, no weights
    mp.morph_w.clear();
    mp.morph_v = std::move(v); mp.morph_n = std::move(n);
    mp.n_targets = first ? n_targets : 0;
    sc->morph_tables_dirty = true;
    if (was) sc->pose_dirty |= POSE_GEOM;
    if (was_n) sc->pose_dirty |= POSE_NORMALS;
    moved_changed(sc, model, was);
    return MR_OK;
}

// mr_scene_set_model_morph_weights behind its argument checks
void set_model_morph_weights(mr_scene *sc, int32_t model, const double *w)
{
    mr_scene::ModelPose &mp = sc->poses[model];
    const size_t n = (size_t)mp.n_targets;
    if (!w && !mp.has_weights) return;
    if (w && mp.has_weights && !std::memcmp(mp.morph_w.data(), w, n * sizeof(double))) return;
    const bool was = mp.moved(), was_n = mp.morph_normals();
    mp.has_weights = w != nullptr;
    mp.morph_w.assign(w ? w : nullptr, w ? w + n : nullptr);
    moved_changed(sc, model, was);
    sc->pose_dirty |= POSE_GEOM;
    // normals that follow the morph: new weights bring k_morph_normals and whatever takes its result (the skin's
    // normals, or the normal matrix), a model that starts or stops following the whole normals' part
    if (was_n != mp.morph_normals()) sc->pose_dirty |= POSE_NORMALS;
    else if (was_n) sc->pose_dirty |= POSE_MORPH_N | (mp.skin_normals() ? POSE_SKIN_N : mp.has_g ? POSE_NORMALS : 0);
}

// the per-normal face lists of one model, from the faces the scene holds
bool build_auto_lists(mr_scene *sc, size_t model)
{
    mr_scene::ModelPose &mp = sc->poses[model];
    const int32_t f0 = sc->model_face_off[model];
    const int32_t f1 = model + 1 < sc->model_face_off.size() ? sc->model_face_off[model + 1] : (int32_t)(sc->faces.size() / 12);
    return mr_autonormals::build_lists(mp.n_normals, mp.normal_off, sc->faces.data(), f0, f1, mp.auto_lists);
}

// mr_scene_set_model_auto_normals behind its argument checks: the lists are built when the flag is first on; the flag
// alone launches nothing, and changes nothing for a model that is at rest or has no normals
int set_model_auto_normals(mr_scene *sc, int32_t model, bool on)
{
    mr_scene::ModelPose &mp = sc->poses[model];
    if (mp.auto_on == on) return MR_OK;
    if (on && mp.n_normals > 0 && mp.auto_lists.n == 0) {
        if (!build_auto_lists(sc, (size_t)model)) return fail(MR_E_INVALID, "the model's padded face lists do not fit 32-bit offsets");
        sc->auto_tables_dirty = true;
    }
    mp.auto_on = on;
    // the other normals' paths (normal targets, the skin, the normal matrix) go or come back: the whole normals' part
    if (mp.n_normals > 0 && mp.moved()) sc->pose_dirty |= POSE_NORMALS;
    return MR_OK;
}

// What one pass does, asked of the scene once (plan_pass) and passed to the steps by const reference.
struct PosePlan {
    bool geom = false, restore = false;     // POSE_GEOM is set; a model at rest still has moved vertices in d_verts
    bool normals = false, skin_normals = false, morph_normals = false, auto_n = false;   // the four normals' steps have work
    bool bones = false, weights = false;    // some model has bones / weights
    int32_t pose_rows = 0;                  // models for k_pose_vertices
    int64_t written = 0, skinned = 0, morphed = 0;      // vertices written (moved and restored); by k_skin_vertices; by k_morph_vertices
    bool vertices() const { return pose_rows || skinned || morphed || restore; }      // else: normals alone
    bool nothing() const { return !vertices() && !normals && !skin_normals && !morph_normals && !auto_n; }
    bool morph_tables() const { return weights && (morphed || morph_normals); }
    bool bone_table() const { return bones && (skinned || skin_normals); }
};

PosePlan plan_pass(const mr_scene *sc)
{
    PosePlan p;
    const uint8_t dirty = sc->pose_dirty;
    p.geom = dirty & POSE_GEOM;
    for (const mr_scene::ModelPose &mp : sc->poses) {
        p.normals = p.normals || ((dirty & POSE_NORMALS) && (mp.has_g || mp.normals_on_device || mp.maps_on_device));
        p.skin_normals = p.skin_normals || ((dirty & (POSE_NORMALS | POSE_SKIN_N)) && mp.skin_normals());
        p.morph_normals = p.morph_normals || ((dirty & (POSE_NORMALS | POSE_MORPH_N)) && (mp.morph_normals() || mp.normals_m_morphed));
        p.bones = p.bones || mp.has_bones;
        p.weights = p.weights || mp.has_weights;
        p.auto_n = p.auto_n || ((dirty & (POSE_GEOM | POSE_NORMALS)) && mp.auto_normals());
        if (!p.geom) continue;
        if (!mp.moved()) {                                            // (its own vertices back: restore_vertices)
            if (mp.on_device) { p.restore = true; p.written += mp.n_verts; }
            continue;
        }
        p.written += mp.n_verts;
        if (mp.has_weights) p.morphed += mp.n_verts;                  // (a morph alone: k_morph_vertices writes d_verts)
        if (mp.has_bones) p.skinned += mp.n_verts;
        else if (mp.posed) p.pose_rows += 1;
    }
    return p;
}

// The host side of a pass's tables, a pair per kernel (a row per model, its row per workgroup): kept until the pass has waited for the stream
struct PassTables {
    std::vector<mr::PoseRow> pose;
    std::vector<mr::Vec3Row> normal, texel;
    std::vector<mr::SkinRow> skin;
    std::vector<mr::SkinNormalRow> skin_n;
    std::vector<mr::MorphRow> morph, morph_n;
    std::vector<mr::AutoRow> auto_n;
    std::vector<int32_t> pose_blocks, normal_blocks, texel_blocks, skin_blocks, skin_n_blocks, morph_blocks, morph_n_blocks, auto_blocks;
    std::vector<int32_t> bone0, weight0;     // per model: where its bones / weights start in the pass's tables
};

// A zeroed row for the range [first, first + count) and the entries of the workgroups that cover it; the caller fills
// in the rest at once (the reference holds until the next row)
template <class Row>
Row &add_row(std::vector<Row> &rows, std::vector<int32_t> &blocks, int64_t first, int64_t count)
{
    Row r;
    std::memset(&r, 0, sizeof r);
    r.first = (decltype(r.first))first; r.count = (decltype(r.count))count; r.block0 = (int32_t)blocks.size();
    blocks.insert(blocks.end(), (size_t)blocks_for(count, mr::POSE_BLOCK), (int32_t)rows.size());
    rows.push_back(r);
    return rows.back();
}

// the arrays as the caller passed them, on the device when a pass first needs them
template <class T>
int ensure_pristine(DevBuf &buf, const std::vector<T> &host, bool &valid)
{
    if (valid) return MR_OK;
    if (int rc = upload(buf, host, g_stream)) return rc;
    valid = true;
    return MR_OK;
}
int ensure_pristine_normals(mr_scene *sc) { return ensure_pristine(sc->d_normals0, sc->normals, sc->normals0_valid); }
int ensure_pristine_verts(mr_scene *sc) { return ensure_pristine(sc->d_verts0, sc->verts, sc->verts0_valid); }

// a model's range of dst, given back from the pristine copy
constexpr size_t VERT_BYTES = 4 * sizeof(double), NORMAL_BYTES = 3 * sizeof(float);
int restore_range(DevBuf &dst, const DevBuf &src, int32_t first, int32_t count, size_t bytes_per_element)
{
    const size_t off = (size_t)first * bytes_per_element, bytes = (size_t)count * bytes_per_element;
    HIP_TRY(hipMemcpyAsync(dst.as<char>() + off, src.as<char>() + off, bytes, hipMemcpyDeviceToDevice, g_stream));
    return MR_OK;
}

// d_verts_m / d_normals_m: a copy of the pristine array, made when a morph first leaves its result for the kernels behind it
int ensure_held_copy(DevBuf &held, const DevBuf &pristine, size_t bytes, bool &valid)
{
    if (valid) return MR_OK;
    HIP_TRY(held.ensure(std::max<size_t>(bytes, 16)));
    HIP_TRY(hipMemcpyAsync(held.p, pristine.p, bytes, hipMemcpyDeviceToDevice, g_stream));
    valid = true;
    return MR_OK;
}

// what the kernels behind a morph start from
const double4 *verts_source(const mr_scene *sc) { return (sc->verts_m_valid ? sc->d_verts_m : sc->d_verts0).as<double4>(); }
const float *normals_source(const mr_scene *sc) { return (sc->normals_m_valid ? sc->d_normals_m : sc->d_normals0).as<float>(); }

// a material's object-space normal map, if it has one
inline bool object_space_map(const mr_scene *sc, const mr::Material &m)
{
    return m.tex_norm >= 0 && m.tex_norm < (int32_t)sc->textures.size() && !m.norm_tangent;
}

// The rows of k_pose_normals and k_pose_texels: a row of vertex normals for every model that has a matrix, one of texels
// for every (model, object-space normal map) pair, its re-baked copy in d_rebaked; that model's materials -- the host's
// records -- point at the copy.  mat_row lists (material, the texel row of its map's copy), in model order.
int build_normal_rows(mr_scene *sc, PassTables &t, std::vector<std::pair<int32_t, size_t>> &mat_row)
{
    std::vector<size_t> toff;                            // of every texel row: its copy's first float in d_rebaked
    size_t rebaked = 0;
    for (const mr_scene::ModelPose &mp : sc->poses) {
        if (!mp.has_g) continue;
        if (mp.n_normals > 0 && !mp.skin_normals() && !mp.auto_normals())      // (normals that follow a skin: k_skin_normals applies G as well; rebuilt normals: G has no part in them)
            std::memcpy(add_row(t.normal, t.normal_blocks, mp.normal_off, mp.n_normals).g, mp.g, sizeof mp.g);
        const size_t own = mat_row.size();               // two materials of one model with one map share its copy
        for (int32_t k = mp.mat_off; k < mp.mat_off + mp.n_mats; ++k) {
            const mr::Material &m = sc->materials[k];
            if (!object_space_map(sc, m)) continue;
            size_t row = t.texel.size();
            for (size_t j = own; j < mat_row.size(); ++j)
                if (sc->materials[mat_row[j].first].tex_norm == m.tex_norm) row = mat_row[j].second;
            if (row == t.texel.size()) {
                const mr::Texture &tex = sc->textures[m.tex_norm];
                mr::Vec3Row &r = add_row(t.texel, t.texel_blocks, 0, (int64_t)tex.h * tex.w);
                r.src = tex.rgb;
                std::memcpy(r.g, mp.g, sizeof r.g);
                toff.push_back(rebaked);
                rebaked += (size_t)r.count * 3;
            }
            mat_row.push_back({ k, row });
        }
    }
    HIP_TRY(sc->d_rebaked.ensure(std::max<size_t>(rebaked * sizeof(float), 16)));
    for (size_t k = 0; k < t.texel.size(); ++k) t.texel[k].dst = sc->d_rebaked.as<float>() + toff[k];
    for (const auto &[k, row] : mat_row) sc->materials[k].map_norm.rgb = t.texel[row].dst;      // (h and w stay)
    return MR_OK;
}

// The normals' part of the pass, in front of the vertices' (k_face_static copies d_normals into the face records): runs
// when a normal matrix was set, changed or removed, for every model that has one.  Vertex normals go from the pristine
// d_normals0 (d_normals_m while a morph holds normals there) into d_normals; the re-baked maps' materials go to the
// device.  A model whose matrix is gone gets its normals and its materials' headers back.
int apply_pose_normals(mr_scene *sc, PassTables &t)
{
    std::vector<std::pair<int32_t, size_t>> mat_row;
    if (int rc = build_normal_rows(sc, t, mat_row)) return rc;
    if (!t.normal.empty())
        if (int rc = ensure_pristine_normals(sc)) return rc;
    auto upload_materials = [&](const mr_scene::ModelPose &mp) -> int {
        HIP_TRY(hipMemcpyAsync(sc->d_materials.as<mr::Material>() + mp.mat_off, sc->materials.data() + mp.mat_off,
                               (size_t)mp.n_mats * sizeof(mr::Material), hipMemcpyHostToDevice, g_stream));
        return MR_OK;
    };
    size_t next = 0;
    for (mr_scene::ModelPose &mp : sc->poses) {
        if (mp.has_g) {
            const size_t first = next;
            while (next < mat_row.size() && mat_row[next].first < mp.mat_off + mp.n_mats) ++next;
            if (next > first)
                if (int rc = upload_materials(mp)) return rc;
            mp.maps_on_device = next > first;
            mp.normals_on_device = mp.n_normals > 0;
            continue;
        }
        if (mp.skin_normals() || mp.morph_normals() || mp.auto_normals()) mp.normals_on_device = true;    // (apply_skin_normals / apply_morph_normals / apply_auto_normals write them)
        else if (mp.normals_on_device) {                 // a model whose matrix is gone gets its own normals back
            if (int rc = restore_range(sc->d_normals, sc->d_normals0, mp.normal_off, mp.n_normals, NORMAL_BYTES)) return rc;
            mp.normals_on_device = false;
        }
        if (mp.maps_on_device) {                         // ... and its materials the maps as they were added
            for (int32_t k = mp.mat_off; k < mp.mat_off + mp.n_mats; ++k)
                if (object_space_map(sc, sc->materials[k])) sc->materials[k].map_norm = sc->textures[sc->materials[k].tex_norm];
            if (int rc = upload_materials(mp)) return rc;
            mp.maps_on_device = false;
        }
    }
    if (t.normal.empty() && t.texel.empty()) return MR_OK;
    auto &marks = sc->marks_normals;
    if (int rc = marks.mark(0)) return rc;
    if (!t.normal.empty()) {
        if (int rc = upload(sc->d_normal_rows, t.normal, g_stream)) return rc;
        if (int rc = upload(sc->d_normal_blocks, t.normal_blocks, g_stream)) return rc;
        hipLaunchKernelGGL(mr::k_pose_normals, dim3((unsigned)t.normal_blocks.size()), dim3(mr::POSE_BLOCK), 0, g_stream,
                           sc->d_normal_rows.as<mr::Vec3Row>(), sc->d_normal_blocks.as<int32_t>(), normals_source(sc), sc->d_normals.as<float>());
    }
    if (int rc = marks.mark(1)) return rc;
    if (!t.texel.empty()) {
        if (int rc = upload(sc->d_texel_rows, t.texel, g_stream)) return rc;
        if (int rc = upload(sc->d_texel_blocks, t.texel_blocks, g_stream)) return rc;
        hipLaunchKernelGGL(mr::k_pose_texels, dim3((unsigned)t.texel_blocks.size()), dim3(mr::POSE_BLOCK), 0, g_stream,
                           sc->d_texel_rows.as<mr::Vec3Row>(), sc->d_texel_blocks.as<int32_t>());
    }
    if (int rc = marks.mark(2)) return rc;
    marks.seen = true; marks.ran[0] = !t.normal.empty(); marks.ran[1] = !t.texel.empty();
    return MR_OK;
}

// The skin tables on the device: joints, weights and normal owners of every model that has a skin, one after the
// other.  Rebuilt when a skin was set or removed, not when bones change.
int upload_skin_tables(mr_scene *sc)
{
    if (!sc->skin_tables_dirty) return MR_OK;
    std::vector<int32_t> joints, owners;
    std::vector<double> weights;
    for (mr_scene::ModelPose &mp : sc->poses) {
        if (mp.n_bones == 0) continue;
        mp.table_off = (int32_t)(joints.size() / 4); mp.owner_off = (int32_t)owners.size();
        joints.insert(joints.end(), mp.joints.begin(), mp.joints.end());
        weights.insert(weights.end(), mp.weights.begin(), mp.weights.end());
        owners.insert(owners.end(), mp.owners.begin(), mp.owners.end());
    }
    if (int rc = upload(sc->d_skin_joints, joints, g_stream)) return rc;
    if (int rc = upload(sc->d_skin_weights, weights, g_stream)) return rc;
    if (int rc = upload(sc->d_skin_owners, owners, g_stream)) return rc;
    HIP_TRY(hipStreamSynchronize(g_stream));         // (the vectors go out of scope)
    sc->skin_tables_dirty = false;
    return MR_OK;
}

// The bone table of a pass: the bones of every model that has some, back to back, in one asynchronous upload;
// first[k] is where model k's start.  sc->bone_table lives until the pass has waited for the stream.
int upload_bones(mr_scene *sc, std::vector<int32_t> &first)
{
    sc->bone_table.clear();
    first.assign(sc->poses.size(), 0);
    for (size_t k = 0; k < sc->poses.size(); ++k) {
        const mr_scene::ModelPose &mp = sc->poses[k];
        if (!mp.has_bones) continue;
        first[k] = (int32_t)(sc->bone_table.size() / 16);
        sc->bone_table.insert(sc->bone_table.end(), mp.bones.begin(), mp.bones.end());
    }
    sc->skin_bones = (int32_t)(sc->bone_table.size() / 16);
    return upload(sc->d_bones, sc->bone_table, g_stream);
}

// The normals of the models whose normals follow their skin (k_skin_normals), after apply_pose_normals where that ran:
// from the pristine d_normals0 (d_normals_m while a morph holds normals there) into d_normals.  The bone table is on its
// way (upload_bones).
int apply_skin_normals(mr_scene *sc, PassTables &t)
{
    int64_t written = 0;
    for (size_t k = 0; k < sc->poses.size(); ++k) {
        mr_scene::ModelPose &mp = sc->poses[k];
        if (!mp.skin_normals()) continue;
        mr::SkinNormalRow &r = add_row(t.skin_n, t.skin_n_blocks, mp.normal_off, mp.n_normals);
        r.owner_off = mp.owner_off; r.table_off = mp.table_off; r.bone0 = t.bone0[k];
        r.has_g = mp.has_g ? 1 : 0;
        if (mp.has_g) std::memcpy(r.g, mp.g, sizeof r.g);
        mp.normals_on_device = true;
        written += mp.n_normals;
    }
    sc->skin_normals_written = (int32_t)written;
    if (t.skin_n.empty()) return MR_OK;
    if (int rc = ensure_pristine_normals(sc)) return rc;
    if (int rc = upload(sc->d_skin_n_rows, t.skin_n, g_stream)) return rc;
    if (int rc = upload(sc->d_skin_n_blocks, t.skin_n_blocks, g_stream)) return rc;
    if (int rc = sc->marks_skin.mark(2)) return rc;
    hipLaunchKernelGGL(mr::k_skin_normals, dim3((unsigned)t.skin_n_blocks.size()), dim3(mr::POSE_BLOCK), 0, g_stream,
                       sc->d_skin_n_rows.as<mr::SkinNormalRow>(), sc->d_skin_n_blocks.as<int32_t>(), normals_source(sc),
                       sc->d_skin_owners.as<int32_t>(), sc->d_skin_joints.as<int4>(), sc->d_skin_weights.as<double4>(),
                       sc->d_bones.as<double4>(), sc->d_normals.as<float>());
    if (int rc = sc->marks_skin.mark(3)) return rc;
    sc->marks_skin.ran[1] = true;
    return MR_OK;
}

// The morph lists on the device: the slices of every model that has a morph, its vertices' and then its normals', one
// after the other in the four planes.  Rebuilt when a morph was set or removed, not when weights change.
int upload_morph_tables(mr_scene *sc)
{
    if (!sc->morph_tables_dirty) return MR_OK;
    std::vector<int32_t> slices, target;
    std::vector<double> dx, dy, dz;
    auto append = [&](const mr_morph::Lists &l, int32_t &slice0) {
        const int64_t base = (int64_t)target.size();
        if (base + l.entries() > INT32_MAX) return false;
        slice0 = (int32_t)slices.size();
        for (int32_t f : l.slice_first) slices.push_back((int32_t)base + f);
        target.insert(target.end(), l.target.begin(), l.target.end());
        dx.insert(dx.end(), l.dx.begin(), l.dx.end());
        dy.insert(dy.end(), l.dy.begin(), l.dy.end());
        dz.insert(dz.end(), l.dz.begin(), l.dz.end());
        return true;
    };
    for (mr_scene::ModelPose &mp : sc->poses) {
        if (mp.n_targets == 0) continue;
        if (!append(mp.morph_v, mp.slice0_v) || (mp.morph_n.n > 0 && !append(mp.morph_n, mp.slice0_n)))
            return fail(MR_E_INVALID, "the scene's morph lists do not fit 32-bit offsets");
    }
    if (int rc = upload(sc->d_morph_slices, slices, g_stream)) return rc;
    if (int rc = upload(sc->d_morph_target, target, g_stream)) return rc;
    if (int rc = upload(sc->d_morph_dx, dx, g_stream)) return rc;
    if (int rc = upload(sc->d_morph_dy, dy, g_stream)) return rc;
    if (int rc = upload(sc->d_morph_dz, dz, g_stream)) return rc;
    HIP_TRY(hipStreamSynchronize(g_stream));         // (the vectors go out of scope)
    sc->morph_entries = (int32_t)target.size();
    sc->morph_tables_dirty = false;
    return MR_OK;
}

// The weight table of a pass: the weights of every model that has some, back to back, in one asynchronous upload;
// weight0[k] is where model k's start.  sc->morph_weight_table lives until the pass has waited for the stream.
int upload_morph_weights(mr_scene *sc, std::vector<int32_t> &weight0)
{
    sc->morph_weight_table.clear();
    weight0.assign(sc->poses.size(), 0);
    for (size_t k = 0; k < sc->poses.size(); ++k) {
        const mr_scene::ModelPose &mp = sc->poses[k];
        if (!mp.has_weights) continue;
        weight0[k] = (int32_t)sc->morph_weight_table.size();
        sc->morph_weight_table.insert(sc->morph_weight_table.end(), mp.morph_w.begin(), mp.morph_w.end());
    }
    sc->morph_targets = (int32_t)sc->morph_weight_table.size();
    return upload(sc->d_morph_weights, sc->morph_weight_table, g_stream);
}

// The normals of the models whose normals follow their morph (k_morph_normals), in front of apply_pose_normals and
// apply_skin_normals, which take the result: from the pristine d_normals0 into d_normals_m, or straight into d_normals
// for a model that has neither a normal matrix nor a skin its normals follow.  A model that stopped following gets its
// range of d_normals_m back.  The weight table is on its way (upload_morph_weights).
int apply_morph_normals(mr_scene *sc, PassTables &t)
{
    int64_t written = 0;
    for (size_t k = 0; k < sc->poses.size(); ++k) {
        mr_scene::ModelPose &mp = sc->poses[k];
        if (!mp.morph_normals()) {
            if (mp.normals_m_morphed && sc->normals_m_valid)
                if (int rc = restore_range(sc->d_normals_m, sc->d_normals0, mp.normal_off, mp.n_normals, NORMAL_BYTES)) return rc;
            mp.normals_m_morphed = false;
            continue;
        }
        const bool direct = !mp.has_g && !mp.skin_normals();
        mr::MorphRow &r = add_row(t.morph_n, t.morph_n_blocks, mp.normal_off, mp.n_normals);
        r.slice0 = mp.slice0_n; r.weight0 = t.weight0[k]; r.n_targets = mp.n_targets; r.direct = direct ? 1 : 0;
        if (direct) mp.normals_on_device = true;
        else mp.normals_m_morphed = true;
        written += mp.n_normals;
    }
    sc->morph_normals_written = (int32_t)written;
    if (t.morph_n.empty()) return MR_OK;
    if (int rc = ensure_pristine_normals(sc)) return rc;
    if (int rc = ensure_held_copy(sc->d_normals_m, sc->d_normals0, sc->normals.size() * sizeof(float), sc->normals_m_valid)) return rc;
    if (int rc = upload(sc->d_morph_n_rows, t.morph_n, g_stream)) return rc;
    if (int rc = upload(sc->d_morph_n_blocks, t.morph_n_blocks, g_stream)) return rc;
    if (int rc = sc->marks_morph.mark(2)) return rc;
    hipLaunchKernelGGL(mr::k_morph_normals, dim3((unsigned)t.morph_n_blocks.size()), dim3(mr::POSE_BLOCK), 0,
                       g_stream, sc->d_morph_n_rows.as<mr::MorphRow>(), sc->d_morph_n_blocks.as<int32_t>(), sc->d_morph_slices.as<int32_t>(),
                       sc->d_morph_target.as<int32_t>(), sc->d_morph_dx.as<double>(), sc->d_morph_dy.as<double>(), sc->d_morph_dz.as<double>(),
                       sc->d_morph_weights.as<double>(), sc->d_normals0.as<float>(), sc->d_normals_m.as<float>(), sc->d_normals.as<float>());
    if (int rc = sc->marks_morph.mark(3)) return rc;
    sc->marks_morph.ran[1] = true;
    return MR_OK;
}

// The face lists on the device: the slices of every model that holds lists -- its flag is on, or was on since the last
// commit: a model whose flag comes back finds its slices where it left them -- one after the other.  Rebuilt when a
// model's lists were built or the scene was committed (which drops the host lists: they are built again here), not per pass.
int upload_auto_tables(mr_scene *sc)
{
    if (!sc->auto_tables_dirty) return MR_OK;
    std::vector<int32_t> slices, faces;
    for (size_t k = 0; k < sc->poses.size(); ++k) {
        mr_scene::ModelPose &mp = sc->poses[k];
        if (mp.n_normals == 0 || (!mp.auto_on && mp.auto_lists.n == 0)) continue;
        if (mp.auto_lists.n == 0 && !build_auto_lists(sc, k))
            return fail(MR_E_INVALID, "the model's padded face lists do not fit 32-bit offsets");
        const int64_t base = (int64_t)faces.size();
        if (base + mp.auto_lists.entries() > INT32_MAX) return fail(MR_E_INVALID, "the scene's face lists do not fit 32-bit offsets");
        mp.auto_slice0 = (int32_t)slices.size();
        for (int32_t f : mp.auto_lists.slice_first) slices.push_back((int32_t)base + f);
        faces.insert(faces.end(), mp.auto_lists.face.begin(), mp.auto_lists.face.end());
    }
    if (int rc = upload(sc->d_auto_slices, slices, g_stream)) return rc;
    if (int rc = upload(sc->d_auto_faces, faces, g_stream)) return rc;
    HIP_TRY(hipStreamSynchronize(g_stream));         // (the vectors go out of scope)
    sc->auto_entries = (int32_t)faces.size();
    sc->auto_tables_dirty = false;
    return MR_OK;
}

// The normals of the models that rebuild them from their mesh (k_auto_normals), after the vertex kernels -- d_verts holds the
// moved vertices (already, where only a flag was turned on) -- and in front of k_face_static: from d_verts, and the pristine
// d_normals0 for the values that stay, into d_normals.  Every such model is rebuilt whenever geometry or the normals' part is.
int apply_auto_normals(mr_scene *sc, PassTables &t)
{
    if (int rc = upload_auto_tables(sc)) return rc;
    int64_t written = 0;
    for (mr_scene::ModelPose &mp : sc->poses) {
        if (!mp.auto_normals()) continue;
        add_row(t.auto_n, t.auto_blocks, mp.normal_off, mp.n_normals).slice0 = mp.auto_slice0;
        mp.normals_on_device = true;
        written += mp.n_normals;
    }
    if (t.auto_n.empty()) return MR_OK;
    if (int rc = ensure_pristine_normals(sc)) return rc;
    const size_t waves = t.auto_blocks.size() * (mr::POSE_BLOCK / mr::WAVE);
    HIP_TRY(sc->d_auto_kept.ensure(waves * sizeof(int32_t)));
    HIP_TRY(hipMemsetAsync(sc->d_auto_kept.p, 0, waves * sizeof(int32_t), g_stream));    // (a wavefront past the range's end writes nothing)
    if (int rc = upload(sc->d_auto_rows, t.auto_n, g_stream)) return rc;
    if (int rc = upload(sc->d_auto_blocks, t.auto_blocks, g_stream)) return rc;
    if (int rc = sc->marks_auto.mark(0)) return rc;
    hipLaunchKernelGGL(mr::k_auto_normals, dim3((unsigned)t.auto_blocks.size()), dim3(mr::POSE_BLOCK), 0, g_stream,
                       sc->d_auto_rows.as<mr::AutoRow>(), sc->d_auto_blocks.as<int32_t>(), sc->d_auto_slices.as<int32_t>(),
                       sc->d_auto_faces.as<int32_t>(), sc->d_faces.as<int32_t>(), sc->d_verts.as<double4>(),
                       sc->d_normals0.as<float>(), sc->d_normals.as<float>(), sc->d_auto_kept.as<int32_t>());
    if (int rc = sc->marks_auto.mark(1)) return rc;
    sc->marks_auto.seen = sc->marks_auto.ran[0] = true;
    sc->auto_models = (int32_t)t.auto_n.size();
    sc->auto_written = (int32_t)written;
    sc->auto_kept_waves = (int32_t)waves;
    return MR_OK;
}

// a model that stopped moving gets its own vertices back; behind mark 0, one whose weights are gone its range of d_verts_m
int restore_vertices(mr_scene *sc)
{
    if (int rc = ensure_pristine_verts(sc)) return rc;
    for (mr_scene::ModelPose &mp : sc->poses) {
        if (mp.moved() || !mp.on_device) continue;
        if (int rc = restore_range(sc->d_verts, sc->d_verts0, mp.vert_off, mp.n_verts, VERT_BYTES)) return rc;
        mp.on_device = false;
    }
    if (int rc = sc->marks_pose.mark(0)) return rc;
    for (mr_scene::ModelPose &mp : sc->poses) {
        if (mp.has_weights || !mp.verts_m_morphed) continue;
        if (sc->verts_m_valid)
            if (int rc = restore_range(sc->d_verts_m, sc->d_verts0, mp.vert_off, mp.n_verts, VERT_BYTES)) return rc;
        mp.verts_m_morphed = false;
    }
    return MR_OK;
}

// the morphed models first: one row each (vertex range, slices, weights), into d_verts where nothing follows, else d_verts_m
int morph_vertices(mr_scene *sc, const PosePlan &p, PassTables &t)
{
    if (int rc = ensure_held_copy(sc->d_verts_m, sc->d_verts0, sc->verts.size() * sizeof(double), sc->verts_m_valid)) return rc;
    for (size_t k = 0; k < sc->poses.size(); ++k) {
        mr_scene::ModelPose &mp = sc->poses[k];
        if (!mp.has_weights) continue;
        const bool direct = !mp.posed && !mp.has_bones;
        mr::MorphRow &r = add_row(t.morph, t.morph_blocks, mp.vert_off, mp.n_verts);
        r.slice0 = mp.slice0_v; r.weight0 = t.weight0[k]; r.n_targets = mp.n_targets; r.direct = direct ? 1 : 0;
        if (!direct) mp.verts_m_morphed = true;
    }
    if (int rc = upload(sc->d_morph_rows, t.morph, g_stream)) return rc;
    if (int rc = upload(sc->d_morph_blocks, t.morph_blocks, g_stream)) return rc;
    if (int rc = sc->marks_morph.mark(0)) return rc;
    hipLaunchKernelGGL(mr::k_morph_vertices, dim3((unsigned)t.morph_blocks.size()),
                       dim3(mr::POSE_BLOCK), 0, g_stream, sc->d_morph_rows.as<mr::MorphRow>(), sc->d_morph_blocks.as<int32_t>(),
                       sc->d_morph_slices.as<int32_t>(), sc->d_morph_target.as<int32_t>(), sc->d_morph_dx.as<double>(),
                       sc->d_morph_dy.as<double>(), sc->d_morph_dz.as<double>(), sc->d_morph_weights.as<double>(),
                       sc->d_verts0.as<double4>(), sc->d_verts_m.as<double4>(), sc->d_verts.as<double4>());
    if (int rc = sc->marks_morph.mark(1)) return rc;
    sc->marks_morph.ran[0] = true;
    sc->morph_written = (int32_t)p.morphed;
    return MR_OK;
}

// the posed models that have no bones: one row each (vertex range, the pose)
int pose_vertices(mr_scene *sc, PassTables &t)
{
    for (const mr_scene::ModelPose &mp : sc->poses)
        if (mp.posed && !mp.has_bones) std::memcpy(add_row(t.pose, t.pose_blocks, mp.vert_off, mp.n_verts).m, mp.m, sizeof mp.m);
    if (int rc = upload(sc->d_pose_rows, t.pose, g_stream)) return rc;
    if (int rc = upload(sc->d_pose_blocks, t.pose_blocks, g_stream)) return rc;
    hipLaunchKernelGGL(mr::k_pose_vertices, dim3((unsigned)t.pose_blocks.size()), dim3(mr::POSE_BLOCK), 0, g_stream,
                       sc->d_pose_rows.as<mr::PoseRow>(), sc->d_pose_blocks.as<int32_t>(), verts_source(sc), sc->d_verts.as<double4>());
    return MR_OK;
}

// the skinned models: one row each (vertex range, joint / weight offset, first bone, the pose that follows)
int skin_vertices(mr_scene *sc, const PosePlan &p, PassTables &t)
{
    bool staged = true;                              // the bones of every model of the pass fit the kernel's LDS table
    for (size_t k = 0; k < sc->poses.size(); ++k) {
        const mr_scene::ModelPose &mp = sc->poses[k];
        if (!mp.has_bones) continue;
        mr::SkinRow &r = add_row(t.skin, t.skin_blocks, mp.vert_off, mp.n_verts);
        r.table_off = mp.table_off; r.bone0 = t.bone0[k]; r.n_bones = mp.n_bones;
        r.has_pose = mp.posed ? 1 : 0;
        if (mp.posed) std::memcpy(r.m, mp.m, sizeof r.m);
        staged = staged && mp.n_bones <= mr::SKIN_LDS_BONES;
    }
    if (int rc = upload(sc->d_skin_rows, t.skin, g_stream)) return rc;
    if (int rc = upload(sc->d_skin_blocks, t.skin_blocks, g_stream)) return rc;
    if (int rc = sc->marks_skin.mark(0)) return rc;
    hipLaunchKernelGGL(staged ? mr::k_skin_vertices<true> : mr::k_skin_vertices<false>, dim3((unsigned)t.skin_blocks.size()), dim3(mr::POSE_BLOCK), 0, g_stream,
                       sc->d_skin_rows.as<mr::SkinRow>(), sc->d_skin_blocks.as<int32_t>(), verts_source(sc),
                       sc->d_skin_joints.as<int4>(), sc->d_skin_weights.as<double4>(), sc->d_bones.as<double4>(),
                       sc->d_verts.as<double4>());
    if (int rc = sc->marks_skin.mark(1)) return rc;
    sc->marks_skin.ran[0] = true;
    sc->skin_written = (int32_t)p.skinned;
    return MR_OK;
}

// The vertices' part: d_verts of every model that moves or stopped moving, from the pristine copy.
int move_vertices(mr_scene *sc, const PosePlan &p, PassTables &t)
{
    int rc = restore_vertices(sc);
    if (rc) return rc;
    if (p.morphed && (rc = morph_vertices(sc, p, t))) return rc;
    if (p.pose_rows && (rc = pose_vertices(sc, t))) return rc;
    if (p.skinned && (rc = skin_vertices(sc, p, t))) return rc;
    for (mr_scene::ModelPose &mp : sc->poses)
        if (mp.moved()) mp.on_device = true;
    return MR_OK;
}

// Where no vertex moved the face records take the new normals (k_face_static); else all that a commit builds from positions
// is built again, marks 1-5 of mr_debug_pose_times round the four kernels, and the silhouette cache goes with the geometry.
int rebuild_static(mr_scene *sc, const PosePlan &p)
{
    const int nf = (int)(sc->faces.size() / 12), ne = (int)sc->edges.size();
    auto face_static = [&] {
        hipLaunchKernelGGL(mr::k_face_static<double>, dim3((nf + 255) / 256), dim3(256), 0, g_stream, nf, sc->d_faces.as<int32_t>(),
                           sc->d_face_flags.as<uint8_t>(), sc->d_verts.as<double>(), sc->d_uv.as<float>(), sc->d_normals.as<float>(),
                           sc->d_face_pos.as<mr::FacePos64>(), sc->d_face_attr.as<mr::FaceAttr>());
    };
    auto &marks = sc->marks_pose;
    if (!p.vertices()) {
        if (nf > 0) face_static();
        return MR_OK;
    }
    if (int rc = marks.mark(1)) return rc;
    if (nf > 0) {
        hipLaunchKernelGGL(mr::k_face_normals, dim3((nf + 255) / 256), dim3(256), 0, g_stream, nf, sc->d_faces.as<int32_t>(),
                           sc->d_face_flags.as<uint8_t>(), sc->d_verts.as<double>(), sc->d_face_n.as<double>());
        if (int rc = marks.mark(2)) return rc;
        if (ne > 0)
            hipLaunchKernelGGL(mr::k_edge_normals, dim3((ne + 255) / 256), dim3(256), 0, g_stream, ne, sc->d_edges.as<mr::EdgeRec>(),
                               sc->d_face_n.as<double>());
        if (int rc = marks.mark(3)) return rc;
        face_static();
        if (int rc = marks.mark(4)) return rc;
        const int nc = (nf + mr::CLUSTER_FACES - 1) / mr::CLUSTER_FACES;
        hipLaunchKernelGGL(mr::k_clusters, dim3((nc + 3) / 4), dim3(256), 0, g_stream, nf, sc->d_faces.as<int32_t>(),
                           sc->d_verts.as<double>(), sc->d_clusters.as<mr::ClusterRec>());
        if (int rc = marks.mark(5)) return rc;
    }
    marks.seen = nf > 0;                             // (a scene without faces: two marks, no span to read)
    for (bool &ran : marks.ran) ran = marks.seen;
    sc->sil.drop();
    return MR_OK;
}

int run_pass(mr_scene *sc, const PosePlan &p)
{
    if (sc->pos32) return fail(MR_E_INVALID, "pose pass on a scene of float32 face records");   // (set_model_pose leaves such a scene dirty)
    HIP_TRY(hipDeviceSynchronize());                 // no frame may still be reading the records about to be rewritten
    if (p.vertices())                                // (while tracking is on: d_verts as it stands, for the next frame's per-face velocity)
        if (int rc = snapshot_vertices(sc)) return rc;
    sc->marks_morph.none_ran(); sc->marks_skin.none_ran();
    sc->morph_written = sc->morph_normals_written = sc->morph_targets = sc->skin_written = sc->skin_normals_written = 0;
    PassTables t;
    int rc = MR_OK;
    if (p.morph_tables()) {
        sc->marks_morph.seen = true;
        if ((rc = upload_morph_tables(sc)) || (rc = upload_morph_weights(sc, t.weight0))) return rc;
    }
    if (p.morph_normals && (rc = apply_morph_normals(sc, t))) return rc;
    if (p.normals && (rc = apply_pose_normals(sc, t))) return rc;
    if (p.bone_table()) {
        sc->marks_skin.seen = true;
        if ((rc = upload_skin_tables(sc)) || (rc = upload_bones(sc, t.bone0))) return rc;
    }
    if (p.skin_normals && (rc = apply_skin_normals(sc, t))) return rc;
    if (p.vertices() && (rc = move_vertices(sc, p, t))) return rc;
    if (p.auto_n && (rc = apply_auto_normals(sc, t))) return rc;      // the vertices are in place: the normals rebuilt from them
    if ((rc = rebuild_static(sc, p))) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g_stream));         // (the tables go out of scope)
    sc->pose_passes += 1;
    if (p.vertices()) sc->vert_serial += 1;          // (another state of d_verts)
    sc->pose_written = (int32_t)p.written;           // (0 where no vertex moved)
    return MR_OK;
}

// Runs where commit() runs, right after it.
int apply_poses(mr_scene *sc)
{
    if (!sc->pose_dirty) return MR_OK;
    sc->marks_auto.ran[0] = false;                   // (also a pass that finds nothing to launch rebuilt no normals)
    sc->auto_models = sc->auto_written = sc->auto_kept_waves = 0;
    const PosePlan p = plan_pass(sc);
    if (!p.nothing())                                // (nothing: a commit has just uploaded the pristine vertices)
        if (int rc = run_pass(sc, p)) return rc;
    sc->pose_dirty = 0;
    return MR_OK;
}

}  // namespace
