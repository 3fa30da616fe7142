// host_pose.h -- the pose pass: a model's pose (mr_scene_set_model_pose) applied on the device, in front of the frame.
//
// A pose changes vertex positions and nothing else, so what a commit builds from positions is rebuilt where it lives:
// the posed vertices (k_pose_vertices, from the pristine copy d_verts0 into d_verts, which is what every kernel reads),
// the face normals and their copies in the edge records, the static face records and the cluster records (k_clusters:
// commit() keeps the host builder, so a scene without poses is what it always was).  Topology, attributes, materials,
// tile histories and list capacities stay; the silhouette cache goes, it belongs to the geometry.
// The pass is synchronous: it waits for the device before it starts (frames in flight on other streams read the static
// records: the rule of commit() and mr_scene_add_model) and for its own kernels before it returns.
#pragma once

namespace {

// mr_scene_set_model_pose behind its argument checks: the matrix is kept, and when the model's float32 bit changes the
// scene is left for commit() to rebuild
void set_model_pose(mr_scene *sc, int32_t model, const double *m16)
{
    mr_scene::ModelPose &mp = sc->poses[model];
    if (!m16 && !mp.posed) return;
    if (m16 && mp.posed && !std::memcmp(mp.m, m16, sizeof mp.m)) return;
    const bool was = mp.posed;
    mp.posed = m16 != nullptr;
    if (m16) std::memcpy(mp.m, m16, sizeof mp.m);
    if (was != mp.posed && mp.verts_f32) {
        // posed vertices are float64 (the product of float64 matrices): the model's faces lose FF_VERTS_F32, or get it back
        const size_t f0 = (size_t)sc->model_face_off[model];
        const size_t f1 = (size_t)model + 1 < sc->model_face_off.size() ? (size_t)sc->model_face_off[model + 1] : sc->face_flags.size();
        for (size_t f = f0; f < f1; ++f)
            sc->face_flags[f] = (uint8_t)(mp.posed ? sc->face_flags[f] & ~mr::FF_VERTS_F32 : sc->face_flags[f] | mr::FF_VERTS_F32);
        sc->dirty = true;
    }
    sc->pose_dirty = true;
}

// Runs where commit() runs, right after it.
int apply_poses(mr_scene *sc)
{
    if (!sc->pose_dirty) return MR_OK;
    std::vector<mr::PoseRow> rows;
    std::vector<int32_t> block_row;
    bool restore = false;
    int64_t written = 0;
    for (const mr_scene::ModelPose &mp : sc->poses) {
        if (!mp.posed) { restore = restore || mp.on_device; continue; }
        mr::PoseRow r;
        std::memset(&r, 0, sizeof r);
        r.first = mp.vert_off; r.count = mp.n_verts; r.block0 = (int32_t)block_row.size();
        std::memcpy(r.m, mp.m, sizeof r.m);
        block_row.insert(block_row.end(), (size_t)blocks_for(mp.n_verts, mr::POSE_BLOCK), (int32_t)rows.size());
        rows.push_back(r);
        written += mp.n_verts;
    }
    if (rows.empty() && !restore) {                  // (a commit has just uploaded the pristine vertices)
        sc->pose_dirty = false;
        return MR_OK;
    }
    if (sc->pos32) return fail(MR_E_INVALID, "pose pass on a scene of float32 face records");   // (set_model_pose leaves such a scene dirty)
    HIP_TRY(hipDeviceSynchronize());                 // no frame may still be reading the records about to be rewritten
    if (!sc->verts0_valid) {
        if (int rc = upload(sc->d_verts0, sc->verts, g_stream)) return rc;
        sc->verts0_valid = true;
    }
    // a model whose pose was removed gets its own vertices back
    for (mr_scene::ModelPose &mp : sc->poses) {
        if (mp.posed || !mp.on_device) continue;
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
    if (!rows.empty()) {
        if (int rc = upload(sc->d_pose_rows, rows, g_stream)) return rc;
        if (int rc = upload(sc->d_pose_blocks, block_row, g_stream)) return rc;
        hipLaunchKernelGGL(mr::k_pose_vertices, dim3((unsigned)block_row.size()), dim3(mr::POSE_BLOCK), 0, g_stream,
                           sc->d_pose_rows.as<mr::PoseRow>(), sc->d_pose_blocks.as<int32_t>(), sc->d_verts0.as<double4>(),
                           sc->d_verts.as<double4>());
        for (mr_scene::ModelPose &mp : sc->poses) mp.on_device = mp.posed;
    }
    HIP_TRY(hipEventRecord(sc->pose_ev[mark++], g_stream));
    const int nf = (int)(sc->faces.size() / 12), ne = (int)sc->edges.size();
    if (nf > 0) {
        hipLaunchKernelGGL(mr::k_face_normals, dim3((nf + 255) / 256), dim3(256), 0, g_stream, nf, sc->d_faces.as<int32_t>(),
                           sc->d_face_flags.as<uint8_t>(), sc->d_verts.as<double>(), sc->d_face_n.as<double>());
        HIP_TRY(hipEventRecord(sc->pose_ev[mark++], g_stream));
        if (ne > 0)
            hipLaunchKernelGGL(mr::k_edge_normals, dim3((ne + 255) / 256), dim3(256), 0, g_stream, ne, sc->d_edges.as<mr::EdgeRec>(),
                               sc->d_face_n.as<double>());
        HIP_TRY(hipEventRecord(sc->pose_ev[mark++], g_stream));
        hipLaunchKernelGGL(mr::k_face_static<double>, dim3((nf + 255) / 256), dim3(256), 0, g_stream, nf, sc->d_faces.as<int32_t>(),
                           sc->d_face_flags.as<uint8_t>(), sc->d_verts.as<double>(), sc->d_uv.as<float>(), sc->d_normals.as<float>(),
                           sc->d_face_pos.as<mr::FacePos64>(), sc->d_face_attr.as<mr::FaceAttr>());
        HIP_TRY(hipEventRecord(sc->pose_ev[mark++], g_stream));
        const int nc = (nf + mr::CLUSTER_FACES - 1) / mr::CLUSTER_FACES;
        hipLaunchKernelGGL(mr::k_clusters, dim3((nc + 3) / 4), dim3(256), 0, g_stream, nf, sc->d_faces.as<int32_t>(),
                           sc->d_verts.as<double>(), sc->d_clusters.as<mr::ClusterRec>());
        HIP_TRY(hipEventRecord(sc->pose_ev[mark++], g_stream));
    }
    sc->pose_marks = mark;
    sc->sil.drop();                                  // the silhouette belongs to the geometry
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g_stream));         // (the two tables go out of scope)
    sc->pose_dirty = false;
    sc->pose_passes += 1;
    sc->pose_written = (int32_t)written;
    return MR_OK;
}

}  // namespace
