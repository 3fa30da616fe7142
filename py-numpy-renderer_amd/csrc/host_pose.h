// host_pose.h -- the pose pass: a model's pose (mr_scene_set_model_pose) applied on the device, in front of the frame.
//
// A pose changes vertex positions, so what a commit builds from positions is rebuilt where it lives:
// the posed vertices (k_pose_vertices, from the pristine copy d_verts0 into d_verts, which is what every kernel reads),
// the face normals and their copies in the edge records, the static face records and the cluster records (k_clusters:
// commit() keeps the host builder, so a scene without poses is what it always was).  Topology, attributes, materials,
// tile histories and list capacities stay; the silhouette cache goes, it belongs to the geometry.
// A model that also has a normal matrix (mr_scene_set_model_pose_normals) gets its vertex normals and its object-space
// normal maps transformed in the same pass (apply_pose_normals), in front of the kernels above.
// A model that has a skin and bones (mr_scene_set_model_skin, mr_scene_set_model_bones) is to the pass what a posed one
// is: its vertices come from k_skin_vertices instead of k_pose_vertices (the pose, if any, applied after the skin), its
// normals, where they follow the skin, from k_skin_normals (apply_skin_normals); everything after that is the same code.
// A model that has a morph and weights (mr_scene_set_model_morph, mr_scene_set_model_morph_weights) comes first in the
// pass: k_morph_vertices writes its morphed vertices -- straight into d_verts when neither skin nor pose follows, else into
// d_verts_m, the copy of d_verts0 that k_skin_vertices and k_pose_vertices then take as their pristine source -- and
// k_morph_normals does the same for its normals with d_normals_m (apply_morph_normals).  The kernels that follow are
// the same code with another source pointer.
// A model whose flag is on (mr_scene_set_model_auto_normals) and that moves gets its vertex normals from k_auto_normals
// (apply_auto_normals), after the vertex kernels and in front of k_face_static; k_morph_normals, k_skin_normals and
// k_pose_normals leave it out of their rows (k_pose_texels does not: its object-space maps are re-baked as ever).
// The pass is synchronous: it waits for the device before it starts (frames in flight on other streams read the static
// records: the rule of commit() and mr_scene_add_model) and for its own kernels before it returns.
#pragma once

namespace {

// A model that moves (a pose, or bones on its skin) has float64 vertices -- the products of float64 matrices: when
// "moves" changes for a model passed as float32, its faces lose FF_VERTS_F32 or get it back, and the scene is left
// for commit() to rebuild
void moved_changed(mr_scene *sc, int32_t model, bool was)
{
    const mr_scene::ModelPose &mp = sc->poses[model];
    const bool now = mp.moved();
    // a model whose normals are rebuilt from its mesh (mr_scene_set_model_auto_normals) starts or stops doing so with
    // "moves": the whole normals' part, as for a model that starts or stops following a skin
    if (was != now && mp.auto_on && mp.n_normals > 0) sc->pose_dirty = sc->pose_g_dirty = true;
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
        sc->pose_g_dirty = true;
    }
    moved_changed(sc, model, was);
    sc->pose_dirty = sc->pose_geom_dirty = true;
}

// mr_scene_set_model_pose_normals behind its argument checks
void set_model_pose_normals(mr_scene *sc, int32_t model, const double *g9)
{
    mr_scene::ModelPose &mp = sc->poses[model];
    if (!g9 && !mp.has_g) return;
    if (g9 && mp.has_g && !std::memcmp(mp.g, g9, sizeof mp.g)) return;
    mp.has_g = g9 != nullptr;
    if (g9) std::memcpy(mp.g, g9, sizeof mp.g);
    sc->pose_dirty = sc->pose_g_dirty = true;
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
    if (was) sc->pose_dirty = sc->pose_geom_dirty = true;
    if (was_n) sc->pose_dirty = sc->pose_g_dirty = true;
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
    sc->pose_dirty = sc->pose_geom_dirty = true;
    // normals that follow the skin: new bones bring k_skin_normals alone, a model that starts or stops following
    // the whole normals' part (its normals come from another kernel, or from the pristine copy, then)
    if (was_n != mp.skin_normals()) sc->pose_g_dirty = true;
    else if (was_n) sc->skin_n_dirty = true;
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
    if (was) sc->pose_dirty = sc->pose_geom_dirty = true;
    if (was_n) sc->pose_dirty = sc->pose_g_dirty = true;
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
    sc->pose_dirty = sc->pose_geom_dirty = true;
    // normals that follow the morph: new weights bring k_morph_normals and whatever takes its result (the skin's
    // normals, or the normal matrix), a model that starts or stops following the whole normals' part
    if (was_n != mp.morph_normals()) sc->pose_g_dirty = true;
    else if (was_n) {
        sc->morph_n_dirty = true;
        if (mp.skin_normals()) sc->skin_n_dirty = true;
        else if (mp.has_g) sc->pose_g_dirty = true;
    }
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
    if (mp.n_normals > 0 && mp.moved()) sc->pose_dirty = sc->pose_g_dirty = true;
    return MR_OK;
}

// a material's object-space normal map, if it has one
inline bool object_space_map(const mr_scene *sc, const mr::Material &m)
{
    return m.tex_norm >= 0 && m.tex_norm < (int32_t)sc->textures.size() && !m.norm_tangent;
}

// The normals' part of the pass, in front of the vertices' (k_face_static copies d_normals into the face records): runs
// when a normal matrix was set, changed or removed, for every model that has one.  Vertex normals go from the pristine
// d_normals0 into d_normals; every (model, object-space normal map) pair gets a re-baked copy of the map in d_rebaked,
// and that model's materials -- the host's records, then their range on the device -- point at the copy.  A model whose
// matrix is gone gets its normals and its materials' headers back.  The caller has waited for the device.
struct NormalTables {                                    // (the caller keeps them until it has waited for the stream)
    std::vector<mr::Vec3Row> nrows, trows;
    std::vector<int32_t> nblocks, tblocks;
};

int apply_pose_normals(mr_scene *sc, NormalTables &tables)
{
    auto &[nrows, trows, nblocks, tblocks] = tables;
    std::vector<size_t> toff;                            // of every texel row: its copy's first float in d_rebaked
    std::vector<std::pair<int32_t, size_t>> mat_row;     // (material, the texel row of its map's copy)
    size_t rebaked = 0;
    for (const mr_scene::ModelPose &mp : sc->poses) {
        if (!mp.has_g) continue;
        mr::Vec3Row r;
        std::memset(&r, 0, sizeof r);
        std::memcpy(r.g, mp.g, sizeof r.g);
        if (mp.n_normals > 0 && !mp.skin_normals() && !mp.auto_normals()) {    // (normals that follow a skin: k_skin_normals applies G as well; rebuilt normals: G has no part in them)
            r.first = mp.normal_off; r.count = mp.n_normals; r.block0 = (int32_t)nblocks.size();
            nblocks.insert(nblocks.end(), (size_t)blocks_for(mp.n_normals, mr::POSE_BLOCK), (int32_t)nrows.size());
            nrows.push_back(r);
        }
        const size_t own = mat_row.size();               // two materials of one model with one map share its copy
        for (int32_t k = mp.mat_off; k < mp.mat_off + mp.n_mats; ++k) {
            const mr::Material &m = sc->materials[k];
            if (!object_space_map(sc, m)) continue;
            size_t row = trows.size();
            for (size_t j = own; j < mat_row.size(); ++j)
                if (sc->materials[mat_row[j].first].tex_norm == m.tex_norm) row = mat_row[j].second;
            if (row == trows.size()) {
                const mr::Texture &t = sc->textures[m.tex_norm];
                r.first = 0; r.src = t.rgb; r.count = (int64_t)t.h * t.w; r.block0 = (int32_t)tblocks.size();
                tblocks.insert(tblocks.end(), (size_t)blocks_for(r.count, mr::POSE_BLOCK), (int32_t)row);
                trows.push_back(r);
                toff.push_back(rebaked);
                rebaked += (size_t)r.count * 3;
            }
            mat_row.push_back({ k, row });
        }
    }
    HIP_TRY(sc->d_rebaked.ensure(std::max<size_t>(rebaked * sizeof(float), 16)));
    for (size_t k = 0; k < trows.size(); ++k) trows[k].dst = sc->d_rebaked.as<float>() + toff[k];
    for (const auto &[k, row] : mat_row) sc->materials[k].map_norm.rgb = trows[row].dst;      // (h and w stay)
    if (!nrows.empty() && !sc->normals0_valid) {
        if (int rc = upload(sc->d_normals0, sc->normals, g_stream)) return rc;
        sc->normals0_valid = true;
    }
    auto upload_materials = [&](const mr_scene::ModelPose &mp) -> int {
        HIP_TRY(hipMemcpyAsync(sc->d_materials.as<mr::Material>() + mp.mat_off, sc->materials.data() + mp.mat_off,
                               (size_t)mp.n_mats * sizeof(mr::Material), hipMemcpyHostToDevice, g_stream));
        return MR_OK;
    };
    size_t next = 0;                                     // (mat_row lists the models' materials in model order)
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
            const size_t off = (size_t)mp.normal_off * 3 * sizeof(float), bytes = (size_t)mp.n_normals * 3 * sizeof(float);
            HIP_TRY(hipMemcpyAsync(static_cast<char *>(sc->d_normals.p) + off, static_cast<const char *>(sc->d_normals0.p) + off, bytes,
                                   hipMemcpyDeviceToDevice, g_stream));
            mp.normals_on_device = false;
        }
        if (mp.maps_on_device) {                         // ... and its materials the maps as they were added
            for (int32_t k = mp.mat_off; k < mp.mat_off + mp.n_mats; ++k)
                if (object_space_map(sc, sc->materials[k])) sc->materials[k].map_norm = sc->textures[sc->materials[k].tex_norm];
            if (int rc = upload_materials(mp)) return rc;
            mp.maps_on_device = false;
        }
    }
    if (nrows.empty() && trows.empty()) return MR_OK;
    // three marks round the two kernels (mr_debug_pose_normals_times)
    for (hipEvent_t &e : sc->pose_n_ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventRecord(sc->pose_n_ev[0], g_stream));
    if (!nrows.empty()) {
        if (int rc = upload(sc->d_normal_rows, nrows, g_stream)) return rc;
        if (int rc = upload(sc->d_normal_blocks, nblocks, g_stream)) return rc;
        hipLaunchKernelGGL(mr::k_pose_normals, dim3((unsigned)nblocks.size()), dim3(mr::POSE_BLOCK), 0, g_stream,
                           sc->d_normal_rows.as<mr::Vec3Row>(), sc->d_normal_blocks.as<int32_t>(),
                           (sc->normals_m_valid ? sc->d_normals_m : sc->d_normals0).as<float>(), sc->d_normals.as<float>());
    }
    HIP_TRY(hipEventRecord(sc->pose_n_ev[1], g_stream));
    if (!trows.empty()) {
        if (int rc = upload(sc->d_texel_rows, trows, g_stream)) return rc;
        if (int rc = upload(sc->d_texel_blocks, tblocks, g_stream)) return rc;
        hipLaunchKernelGGL(mr::k_pose_texels, dim3((unsigned)tblocks.size()), dim3(mr::POSE_BLOCK), 0, g_stream,
                           sc->d_texel_rows.as<mr::Vec3Row>(), sc->d_texel_blocks.as<int32_t>());
    }
    HIP_TRY(hipEventRecord(sc->pose_n_ev[2], g_stream));
    sc->pose_n_marks = 3;
    sc->pose_n_ran[0] = !nrows.empty(); sc->pose_n_ran[1] = !trows.empty();
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

struct SkinTables {                                      // (the caller keeps them until it has waited for the stream)
    std::vector<mr::SkinRow> rows;
    std::vector<mr::SkinNormalRow> nrows;
    std::vector<int32_t> blocks, nblocks, bone0;
};

// The normals of the models whose normals follow their skin (k_skin_normals), after apply_pose_normals where that ran:
// from the pristine d_normals0 (d_normals_m while a morph holds normals there) into d_normals.  The bone table is on its
// way (upload_bones).
int apply_skin_normals(mr_scene *sc, SkinTables &t)
{
    int64_t written = 0;
    for (size_t k = 0; k < sc->poses.size(); ++k) {
        mr_scene::ModelPose &mp = sc->poses[k];
        if (!mp.skin_normals()) continue;
        mr::SkinNormalRow r;
        std::memset(&r, 0, sizeof r);
        r.first = mp.normal_off; r.count = mp.n_normals; r.block0 = (int32_t)t.nblocks.size();
        r.owner_off = mp.owner_off; r.table_off = mp.table_off; r.bone0 = t.bone0[k];
        r.has_g = mp.has_g ? 1 : 0;
        if (mp.has_g) std::memcpy(r.g, mp.g, sizeof r.g);
        t.nblocks.insert(t.nblocks.end(), (size_t)blocks_for(mp.n_normals, mr::POSE_BLOCK), (int32_t)t.nrows.size());
        t.nrows.push_back(r);
        mp.normals_on_device = true;
        written += mp.n_normals;
    }
    sc->skin_normals_written = (int32_t)written;
    if (t.nrows.empty()) return MR_OK;
    if (!sc->normals0_valid) {
        if (int rc = upload(sc->d_normals0, sc->normals, g_stream)) return rc;
        sc->normals0_valid = true;
    }
    if (int rc = upload(sc->d_skin_n_rows, t.nrows, g_stream)) return rc;
    if (int rc = upload(sc->d_skin_n_blocks, t.nblocks, g_stream)) return rc;
    HIP_TRY(hipEventRecord(sc->skin_ev[2], g_stream));
    hipLaunchKernelGGL(mr::k_skin_normals, dim3((unsigned)t.nblocks.size()), dim3(mr::POSE_BLOCK), 0, g_stream,
                       sc->d_skin_n_rows.as<mr::SkinNormalRow>(), sc->d_skin_n_blocks.as<int32_t>(),
                       (sc->normals_m_valid ? sc->d_normals_m : sc->d_normals0).as<float>(),
                       sc->d_skin_owners.as<int32_t>(), sc->d_skin_joints.as<int4>(), sc->d_skin_weights.as<double4>(),
                       sc->d_bones.as<double4>(), sc->d_normals.as<float>());
    HIP_TRY(hipEventRecord(sc->skin_ev[3], g_stream));
    sc->skin_ran[1] = true;
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

struct MorphTables {                                     // (the caller keeps them until it has waited for the stream)
    std::vector<mr::MorphRow> rows, nrows;
    std::vector<int32_t> blocks, nblocks, weight0;
};

// The weight table of a pass: the weights of every model that has some, back to back, in one asynchronous upload;
// weight0[k] is where model k's start.  sc->morph_weight_table lives until the pass has waited for the stream.
int upload_morph_weights(mr_scene *sc, MorphTables &t)
{
    sc->morph_weight_table.clear();
    t.weight0.assign(sc->poses.size(), 0);
    for (size_t k = 0; k < sc->poses.size(); ++k) {
        const mr_scene::ModelPose &mp = sc->poses[k];
        if (!mp.has_weights) continue;
        t.weight0[k] = (int32_t)sc->morph_weight_table.size();
        sc->morph_weight_table.insert(sc->morph_weight_table.end(), mp.morph_w.begin(), mp.morph_w.end());
    }
    sc->morph_targets = (int32_t)sc->morph_weight_table.size();
    return upload(sc->d_morph_weights, sc->morph_weight_table, g_stream);
}

inline mr::MorphRow morph_row(int32_t first, int32_t count, size_t block0, int32_t slice0, int32_t weight0, int32_t n_targets, bool direct)
{
    mr::MorphRow r;
    std::memset(&r, 0, sizeof r);
    r.first = first; r.count = count; r.block0 = (int32_t)block0; r.slice0 = slice0;
    r.weight0 = weight0; r.n_targets = n_targets; r.direct = direct ? 1 : 0;
    return r;
}

// The normals of the models whose normals follow their morph (k_morph_normals), in front of apply_pose_normals and
// apply_skin_normals, which take the result: from the pristine d_normals0 into d_normals_m, or straight into d_normals
// for a model that has neither a normal matrix nor a skin its normals follow.  A model that stopped following gets its
// range of d_normals_m back.  The weight table is on its way (upload_morph_weights).
int apply_morph_normals(mr_scene *sc, MorphTables &t)
{
    int64_t written = 0;
    for (size_t k = 0; k < sc->poses.size(); ++k) {
        mr_scene::ModelPose &mp = sc->poses[k];
        const size_t off = (size_t)mp.normal_off * 3 * sizeof(float), bytes = (size_t)mp.n_normals * 3 * sizeof(float);
        if (!mp.morph_normals()) {
            if (mp.normals_m_morphed && sc->normals_m_valid)
                HIP_TRY(hipMemcpyAsync(static_cast<char *>(sc->d_normals_m.p) + off, static_cast<const char *>(sc->d_normals0.p) + off, bytes,
                                       hipMemcpyDeviceToDevice, g_stream));
            mp.normals_m_morphed = false;
            continue;
        }
        const bool direct = !mp.has_g && !mp.skin_normals();
        t.nrows.push_back(morph_row(mp.normal_off, mp.n_normals, t.nblocks.size(), mp.slice0_n, t.weight0[k], mp.n_targets, direct));
        t.nblocks.insert(t.nblocks.end(), (size_t)blocks_for(mp.n_normals, mr::POSE_BLOCK), (int32_t)t.nrows.size() - 1);
        if (direct) mp.normals_on_device = true;
        else mp.normals_m_morphed = true;
        written += mp.n_normals;
    }
    sc->morph_normals_written = (int32_t)written;
    if (t.nrows.empty()) return MR_OK;
    if (!sc->normals0_valid) {
        if (int rc = upload(sc->d_normals0, sc->normals, g_stream)) return rc;
        sc->normals0_valid = true;
    }
    if (!sc->normals_m_valid) {
        const size_t bytes = sc->normals.size() * sizeof(float);
        HIP_TRY(sc->d_normals_m.ensure(std::max<size_t>(bytes, 16)));
        HIP_TRY(hipMemcpyAsync(sc->d_normals_m.p, sc->d_normals0.p, bytes, hipMemcpyDeviceToDevice, g_stream));
        sc->normals_m_valid = true;
    }
    if (int rc = upload(sc->d_morph_n_rows, t.nrows, g_stream)) return rc;
    if (int rc = upload(sc->d_morph_n_blocks, t.nblocks, g_stream)) return rc;
    HIP_TRY(hipEventRecord(sc->morph_ev[2], g_stream));
    hipLaunchKernelGGL(mr::k_morph_normals, dim3((unsigned)t.nblocks.size()), dim3(mr::POSE_BLOCK), 0,
                       g_stream, sc->d_morph_n_rows.as<mr::MorphRow>(), sc->d_morph_n_blocks.as<int32_t>(), sc->d_morph_slices.as<int32_t>(),
                       sc->d_morph_target.as<int32_t>(), sc->d_morph_dx.as<double>(), sc->d_morph_dy.as<double>(), sc->d_morph_dz.as<double>(),
                       sc->d_morph_weights.as<double>(), sc->d_normals0.as<float>(), sc->d_normals_m.as<float>(), sc->d_normals.as<float>());
    HIP_TRY(hipEventRecord(sc->morph_ev[3], g_stream));
    sc->morph_ran[1] = true;
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

struct AutoTables {                                      // (the caller keeps them until it has waited for the stream)
    std::vector<mr::AutoRow> rows;
    std::vector<int32_t> blocks;
};

// The normals of the models that rebuild them from their mesh (k_auto_normals), after the vertex kernels -- d_verts holds
// the moved vertices -- and in front of k_face_static: from d_verts, and the pristine d_normals0 for the values that
// stay, into d_normals.  Every such model is rebuilt whenever the pass rewrites geometry or the normals' part runs.
int apply_auto_normals(mr_scene *sc, AutoTables &t)
{
    if (int rc = upload_auto_tables(sc)) return rc;
    int64_t written = 0;
    for (mr_scene::ModelPose &mp : sc->poses) {
        if (!mp.auto_normals()) continue;
        mr::AutoRow r;
        std::memset(&r, 0, sizeof r);
        r.first = mp.normal_off; r.count = mp.n_normals; r.block0 = (int32_t)t.blocks.size(); r.slice0 = mp.auto_slice0;
        t.blocks.insert(t.blocks.end(), (size_t)blocks_for(mp.n_normals, mr::POSE_BLOCK), (int32_t)t.rows.size());
        t.rows.push_back(r);
        mp.normals_on_device = true;
        written += mp.n_normals;
    }
    if (t.rows.empty()) return MR_OK;
    if (!sc->normals0_valid) {
        if (int rc = upload(sc->d_normals0, sc->normals, g_stream)) return rc;
        sc->normals0_valid = true;
    }
    for (hipEvent_t &e : sc->auto_ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    const size_t waves = t.blocks.size() * (mr::POSE_BLOCK / mr::WAVE);
    HIP_TRY(sc->d_auto_kept.ensure(waves * sizeof(int32_t)));
    HIP_TRY(hipMemsetAsync(sc->d_auto_kept.p, 0, waves * sizeof(int32_t), g_stream));    // (a wavefront past the range's end writes nothing)
    if (int rc = upload(sc->d_auto_rows, t.rows, g_stream)) return rc;
    if (int rc = upload(sc->d_auto_blocks, t.blocks, g_stream)) return rc;
    HIP_TRY(hipEventRecord(sc->auto_ev[0], g_stream));
    hipLaunchKernelGGL(mr::k_auto_normals, dim3((unsigned)t.blocks.size()), dim3(mr::POSE_BLOCK), 0, g_stream,
                       sc->d_auto_rows.as<mr::AutoRow>(), sc->d_auto_blocks.as<int32_t>(), sc->d_auto_slices.as<int32_t>(),
                       sc->d_auto_faces.as<int32_t>(), sc->d_faces.as<int32_t>(), sc->d_verts.as<double4>(),
                       sc->d_normals0.as<float>(), sc->d_normals.as<float>(), sc->d_auto_kept.as<int32_t>());
    HIP_TRY(hipEventRecord(sc->auto_ev[1], g_stream));
    sc->auto_ran = sc->auto_marks = true;
    sc->auto_models = (int32_t)t.rows.size();
    sc->auto_written = (int32_t)written;
    sc->auto_kept_waves = (int32_t)waves;
    return MR_OK;
}

// Runs where commit() runs, right after it.  What a pass does depends on what changed: a pose brings all of it, a
// normal matrix alone (the pose as it was) the normals' part and k_face_static -- vertices, face and edge normals, the
// cluster records and the silhouette cache stay.
int apply_poses(mr_scene *sc)
{
    if (!sc->pose_dirty) return MR_OK;
    const bool geom = sc->pose_geom_dirty;
    sc->auto_ran = false;                            // (also a pass that finds nothing to launch rebuilt no normals)
    sc->auto_models = sc->auto_written = sc->auto_kept_waves = 0;
    std::vector<mr::PoseRow> rows;
    std::vector<int32_t> block_row;
    SkinTables skin;
    MorphTables morph;
    AutoTables auto_tables;
    bool auto_n = false;
    bool restore = false, normals = false, skin_normals = false, bones = false, morph_normals = false, weights = false;
    int64_t written = 0, skinned = 0, morphed = 0;
    for (const mr_scene::ModelPose &mp : sc->poses) {
        normals = normals || (sc->pose_g_dirty && (mp.has_g || mp.normals_on_device || mp.maps_on_device));
        skin_normals = skin_normals || ((sc->pose_g_dirty || sc->skin_n_dirty) && mp.skin_normals());
        morph_normals = morph_normals || ((sc->pose_g_dirty || sc->morph_n_dirty) && (mp.morph_normals() || mp.normals_m_morphed));
        bones = bones || mp.has_bones;
        weights = weights || mp.has_weights;
        auto_n = auto_n || ((geom || sc->pose_g_dirty) && mp.auto_normals());
        if (!geom) continue;
        if (!mp.moved()) { restore = restore || mp.on_device; continue; }
        if (mp.has_weights) morphed += mp.n_verts;                  // (its row needs the weight table: below)
        if (mp.has_bones) { skinned += mp.n_verts; continue; }      // (its row needs the bone table: below)
        if (!mp.posed) { written += mp.n_verts; continue; }         // (a morph alone: k_morph_vertices writes d_verts)
        mr::PoseRow r;
        std::memset(&r, 0, sizeof r);
        r.first = mp.vert_off; r.count = mp.n_verts; r.block0 = (int32_t)block_row.size();
        std::memcpy(r.m, mp.m, sizeof r.m);
        block_row.insert(block_row.end(), (size_t)blocks_for(mp.n_verts, mr::POSE_BLOCK), (int32_t)rows.size());
        rows.push_back(r);
        written += mp.n_verts;
    }
    written += skinned;
    if (rows.empty() && !skinned && !morphed && !restore && !normals && !skin_normals && !morph_normals && !auto_n) {      // (a commit has just uploaded the pristine vertices)
        sc->pose_dirty = sc->pose_geom_dirty = sc->pose_g_dirty = sc->skin_n_dirty = sc->morph_n_dirty = false;
        return MR_OK;
    }
    if (sc->pos32) return fail(MR_E_INVALID, "pose pass on a scene of float32 face records");   // (set_model_pose leaves such a scene dirty)
    HIP_TRY(hipDeviceSynchronize());                 // no frame may still be reading the records about to be rewritten
    sc->morph_ran[0] = sc->morph_ran[1] = false;
    sc->morph_written = sc->morph_normals_written = sc->morph_targets = 0;
    if (weights && (morphed || morph_normals)) {
        for (hipEvent_t &e : sc->morph_ev)
            if (!e) HIP_TRY(hipEventCreate(&e));
        sc->morph_marks = true;
        if (int rc = upload_morph_tables(sc)) return rc;
        if (int rc = upload_morph_weights(sc, morph)) return rc;
    }
    if (morph_normals)
        if (int rc = apply_morph_normals(sc, morph)) return rc;
    NormalTables normal_tables;
    if (normals)
        if (int rc = apply_pose_normals(sc, normal_tables)) return rc;
    sc->skin_ran[0] = sc->skin_ran[1] = false;
    sc->skin_written = sc->skin_normals_written = 0;
    if (bones && (skinned || skin_normals)) {
        for (hipEvent_t &e : sc->skin_ev)
            if (!e) HIP_TRY(hipEventCreate(&e));
        sc->skin_marks = true;
        if (int rc = upload_skin_tables(sc)) return rc;
        if (int rc = upload_bones(sc, skin.bone0)) return rc;
    }
    if (skin_normals)
        if (int rc = apply_skin_normals(sc, skin)) return rc;
    const int nf = (int)(sc->faces.size() / 12), ne = (int)sc->edges.size();
    auto face_static = [&] {
        hipLaunchKernelGGL(mr::k_face_static<double>, dim3((nf + 255) / 256), dim3(256), 0, g_stream, nf, sc->d_faces.as<int32_t>(),
                           sc->d_face_flags.as<uint8_t>(), sc->d_verts.as<double>(), sc->d_uv.as<float>(), sc->d_normals.as<float>(),
                           sc->d_face_pos.as<mr::FacePos64>(), sc->d_face_attr.as<mr::FaceAttr>());
    };
    if (rows.empty() && !skinned && !morphed && !restore) {      // normal matrices alone: the face records take the new normals
        if (auto_n)                                  // (a flag that was turned on: d_verts holds the moved vertices already)
            if (int rc = apply_auto_normals(sc, auto_tables)) return rc;
        if (nf > 0) face_static();
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(g_stream));     // (the tables go out of scope)
        sc->pose_dirty = sc->pose_geom_dirty = sc->pose_g_dirty = sc->skin_n_dirty = sc->morph_n_dirty = false;
        sc->pose_passes += 1;
        sc->pose_written = 0;
        return MR_OK;
    }
    if (!sc->verts0_valid) {
        if (int rc = upload(sc->d_verts0, sc->verts, g_stream)) return rc;
        sc->verts0_valid = true;
    }
    // a model whose pose or bones were removed gets its own vertices back
    for (mr_scene::ModelPose &mp : sc->poses) {
        if (mp.moved() || !mp.on_device) continue;
        const size_t off = (size_t)mp.vert_off * 4 * sizeof(double), bytes = (size_t)mp.n_verts * 4 * sizeof(double);
        HIP_TRY(hipMemcpyAsync(static_cast<char *>(sc->d_verts.p) + off, static_cast<const char *>(sc->d_verts0.p) + off, bytes,
                               hipMemcpyDeviceToDevice, g_stream));
        mp.on_device = false;
        written += mp.n_verts;
    }
    // six marks round the five kernels (mr_debug_pose_times): the pass waits for the device anyway
    for (hipEvent_t &e : sc->pose_ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    int mark = 0;
    HIP_TRY(hipEventRecord(sc->pose_ev[mark++], g_stream));
    // the morphed models first: one row each (vertex range, slices, weights), into d_verts where nothing follows the
    // morph, else into d_verts_m -- a copy of d_verts0 made once, in which a model whose weights are gone gets its range back
    for (mr_scene::ModelPose &mp : sc->poses) {
        if (mp.has_weights || !mp.verts_m_morphed) continue;
        const size_t off = (size_t)mp.vert_off * 4 * sizeof(double), bytes = (size_t)mp.n_verts * 4 * sizeof(double);
        if (sc->verts_m_valid)
            HIP_TRY(hipMemcpyAsync(static_cast<char *>(sc->d_verts_m.p) + off, static_cast<const char *>(sc->d_verts0.p) + off, bytes,
                                   hipMemcpyDeviceToDevice, g_stream));
        mp.verts_m_morphed = false;
    }
    if (morphed) {
        if (!sc->verts_m_valid) {
            const size_t bytes = sc->verts.size() * sizeof(double);
            HIP_TRY(sc->d_verts_m.ensure(std::max<size_t>(bytes, 16)));
            HIP_TRY(hipMemcpyAsync(sc->d_verts_m.p, sc->d_verts0.p, bytes, hipMemcpyDeviceToDevice, g_stream));
            sc->verts_m_valid = true;
        }
        for (size_t k = 0; k < sc->poses.size(); ++k) {
            mr_scene::ModelPose &mp = sc->poses[k];
            if (!mp.has_weights) continue;
            const bool direct = !mp.posed && !mp.has_bones;
            morph.rows.push_back(morph_row(mp.vert_off, mp.n_verts, morph.blocks.size(), mp.slice0_v, morph.weight0[k], mp.n_targets, direct));
            morph.blocks.insert(morph.blocks.end(), (size_t)blocks_for(mp.n_verts, mr::POSE_BLOCK), (int32_t)morph.rows.size() - 1);
            if (!direct) mp.verts_m_morphed = true;
        }
        if (int rc = upload(sc->d_morph_rows, morph.rows, g_stream)) return rc;
        if (int rc = upload(sc->d_morph_blocks, morph.blocks, g_stream)) return rc;
        HIP_TRY(hipEventRecord(sc->morph_ev[0], g_stream));
        hipLaunchKernelGGL(mr::k_morph_vertices, dim3((unsigned)morph.blocks.size()),
                           dim3(mr::POSE_BLOCK), 0, g_stream, sc->d_morph_rows.as<mr::MorphRow>(), sc->d_morph_blocks.as<int32_t>(),
                           sc->d_morph_slices.as<int32_t>(), sc->d_morph_target.as<int32_t>(), sc->d_morph_dx.as<double>(),
                           sc->d_morph_dy.as<double>(), sc->d_morph_dz.as<double>(), sc->d_morph_weights.as<double>(),
                           sc->d_verts0.as<double4>(), sc->d_verts_m.as<double4>(), sc->d_verts.as<double4>());
        HIP_TRY(hipEventRecord(sc->morph_ev[1], g_stream));
        sc->morph_ran[0] = true;
        sc->morph_written = (int32_t)morphed;
    }
    const double4 *pristine = (sc->verts_m_valid ? sc->d_verts_m : sc->d_verts0).as<double4>();     // what the skin and the pose start from
    if (!rows.empty()) {
        if (int rc = upload(sc->d_pose_rows, rows, g_stream)) return rc;
        if (int rc = upload(sc->d_pose_blocks, block_row, g_stream)) return rc;
        hipLaunchKernelGGL(mr::k_pose_vertices, dim3((unsigned)block_row.size()), dim3(mr::POSE_BLOCK), 0, g_stream,
                           sc->d_pose_rows.as<mr::PoseRow>(), sc->d_pose_blocks.as<int32_t>(), pristine, sc->d_verts.as<double4>());
    }
    if (skinned) {
        // the skinned models: one row each (vertex range, joint / weight offset, first bone, the pose that follows)
        for (size_t k = 0; k < sc->poses.size(); ++k) {
            const mr_scene::ModelPose &mp = sc->poses[k];
            if (!mp.has_bones) continue;
            mr::SkinRow r;
            std::memset(&r, 0, sizeof r);
            r.first = mp.vert_off; r.count = mp.n_verts; r.block0 = (int32_t)skin.blocks.size();
            r.table_off = mp.table_off; r.bone0 = skin.bone0[k]; r.n_bones = mp.n_bones;
            r.has_pose = mp.posed ? 1 : 0;
            if (mp.posed) std::memcpy(r.m, mp.m, sizeof r.m);
            skin.blocks.insert(skin.blocks.end(), (size_t)blocks_for(mp.n_verts, mr::POSE_BLOCK), (int32_t)skin.rows.size());
            skin.rows.push_back(r);
        }
        if (int rc = upload(sc->d_skin_rows, skin.rows, g_stream)) return rc;
        if (int rc = upload(sc->d_skin_blocks, skin.blocks, g_stream)) return rc;
        bool staged = true;                          // the bones of every model of the pass fit the kernel's LDS table
        for (const mr::SkinRow &r : skin.rows) staged = staged && r.n_bones <= mr::SKIN_LDS_BONES;
        HIP_TRY(hipEventRecord(sc->skin_ev[0], g_stream));
        hipLaunchKernelGGL(staged ? mr::k_skin_vertices<true> : mr::k_skin_vertices<false>, dim3((unsigned)skin.blocks.size()), dim3(mr::POSE_BLOCK), 0, g_stream,
                           sc->d_skin_rows.as<mr::SkinRow>(), sc->d_skin_blocks.as<int32_t>(), pristine,
                           sc->d_skin_joints.as<int4>(), sc->d_skin_weights.as<double4>(), sc->d_bones.as<double4>(),
                           sc->d_verts.as<double4>());
        HIP_TRY(hipEventRecord(sc->skin_ev[1], g_stream));
        sc->skin_ran[0] = true;
        sc->skin_written = (int32_t)skinned;
    }
    for (mr_scene::ModelPose &mp : sc->poses)
        if (mp.moved()) mp.on_device = true;
    if (auto_n)                                      // the vertices are in place: the normals rebuilt from them
        if (int rc = apply_auto_normals(sc, auto_tables)) return rc;
    HIP_TRY(hipEventRecord(sc->pose_ev[mark++], g_stream));
    if (nf > 0) {
        hipLaunchKernelGGL(mr::k_face_normals, dim3((nf + 255) / 256), dim3(256), 0, g_stream, nf, sc->d_faces.as<int32_t>(),
                           sc->d_face_flags.as<uint8_t>(), sc->d_verts.as<double>(), sc->d_face_n.as<double>());
        HIP_TRY(hipEventRecord(sc->pose_ev[mark++], g_stream));
        if (ne > 0)
            hipLaunchKernelGGL(mr::k_edge_normals, dim3((ne + 255) / 256), dim3(256), 0, g_stream, ne, sc->d_edges.as<mr::EdgeRec>(),
                               sc->d_face_n.as<double>());
        HIP_TRY(hipEventRecord(sc->pose_ev[mark++], g_stream));
        face_static();
        HIP_TRY(hipEventRecord(sc->pose_ev[mark++], g_stream));
        const int nc = (nf + mr::CLUSTER_FACES - 1) / mr::CLUSTER_FACES;
        hipLaunchKernelGGL(mr::k_clusters, dim3((nc + 3) / 4), dim3(256), 0, g_stream, nf, sc->d_faces.as<int32_t>(),
                           sc->d_verts.as<double>(), sc->d_clusters.as<mr::ClusterRec>());
        HIP_TRY(hipEventRecord(sc->pose_ev[mark++], g_stream));
    }
    sc->pose_marks = mark;
    sc->sil.drop();                                  // the silhouette belongs to the geometry
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g_stream));         // (the tables go out of scope)
    sc->pose_dirty = sc->pose_geom_dirty = sc->pose_g_dirty = sc->skin_n_dirty = sc->morph_n_dirty = false;
    sc->pose_passes += 1;
    sc->pose_written = (int32_t)written;
    return MR_OK;
}

}  // namespace
