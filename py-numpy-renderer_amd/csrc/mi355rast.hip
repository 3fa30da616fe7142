// mi355rast.hip -- the C ABI (include/mi355rast.h) of libmi355rast.  The library is compiled from this file, from
// accum.hip, which holds the accumulation's two kernels in a code object of their own (kernels_accum.h says why), from
// ao.hip, which holds the ambient obscurance's kernel in another, from dof.hip, which holds the depth of field's, and from
// motion.hip, which holds the motion blur's two, from motion_faces.hip, which holds the per-face velocity's two, from
// taa.hip, which holds the temporal anti-aliasing's, from bloom.hip, which holds the bloom's three, from shafts.hip,
// which holds the light shafts' three, from tonemap.hip, which holds the tone mapping's three, and from layers.hip, which
// holds the data layers' one;
// the host code behind the entry points lives in the host_*.h headers beside it, one subject each:
//
//   host_device.h       error text, the library's stream, growable device buffers
//   host_env.h          the environment switches
//   host_silcache.h     the silhouette cache
//   host_scene.h        the static scene and commit()
//   host_overlay_dev.h  the debug-frustum overlay's device plumbing (host_overlay.h builds its lists)
//   host_morph.h        morph targets: the per-vertex contribution lists (plain C++, no HIP)
//   host_autonormals.h  rebuilt vertex normals: the per-normal face lists (plain C++, no HIP)
//   host_pose.h         a model's morph, skin and pose, applied on the device in front of the frame
//   host_pass.h         what the post passes share: weak launches, timing marks, the pass record, the staged table, the checks
//   host_ao.h           ambient obscurance from the z-buffer: the description, k_ao's launch, the host mirror
//   host_dof.h          depth of field from the z-buffer: the description, k_dof's launch, the host mirror
//   host_motion.h       motion blur from a velocity buffer: the description, the two launches, the host mirrors, mr_debug_motion_post
//   host_motion_faces.h the velocity of models that bend: the vertex snapshot and its serial, the two launches, the mirrors
//   host_taa.h          temporal anti-aliasing: the description, the scene's history, the launch, the host mirror, mr_debug_taa_post
//   host_bloom.h        bloom from a resolution pyramid: the description, the pyramid's layout, the launches, the host mirror, mr_debug_bloom_post
//   host_shafts.h       light shafts marched towards a light: the description, S and R, the launches, the host mirror, mr_debug_light_shafts_post
//   host_tonemap.h      tone mapping from a luminance histogram: the description, the slot's words, the scene's exposure, the launches, the host mirror, mr_debug_tone_map_post
//   host_layers.h       data layers from the winner map and the face records: the description, a slot's buffers, the launch, the host mirror, mr_debug_layers_post
//   host_frame.h        the frame slot, the frame's constants and enqueue_frame()
//   host_accum.h        the accumulation: sub-frames summed with weights on the device, finalised once
//   host_post.h         mr_debug_post: k_ao, k_dof and the accumulation's kernels on buffers a caller supplies
//
// One process drives one GPU.  A scene keeps its static arrays (vertices, attributes, index arrays, textures, the
// unique-edge table with the incident faces' normals, per-face and per-cluster records) resident in HBM; a frame is
// three kernels on one HIP stream, with no host synchronisation in between, and whatever its flags add around them:
//
//   (k_vertex_mfma  MR_VERTEX_PATH=mfma: the vertex transform on the matrix cores, in front of k_setup)
//   k_setup         faces: vertex transform, cull, set-up records, own tile lists
//                   edges: silhouette search, shadow-quad extrusion / clip / projection, for every light of the frame --
//                   or, when the silhouette cache holds this light's, the quads' projection alone
//   k_bin_work      tile lists of the large primitives (floor triangles, shadow quads)
//   k_tile          per 16x16 tile: coverage + z + winner, stencil count per light, shading, finalise -> uint8 (a
//                   supersampled frame: resolved to its output pixels in the same kernel)
//   (k_face_status  MR_FRAME_FACE_STATUS;  k_overlay / k_overlay_export  MR_FRAME_OVERLAY: drawn on a whole frame, the
//                   touched pixels' state exported from a part of one;  k_resolve_*  what a supersampled frame's
//                   overlay or MR_RESOLVE_PATH=separate leave to resolve;  D2H of the uint8 rows for mr_render;
//                   k_accum_add behind a sub-frame of mr_accum_add, k_accum_resolve for mr_accum_resolve;
//                   k_ao behind k_tile in a scene with mr_scene_set_ambient_occlusion, k_dof behind them in one with
//                   mr_scene_set_depth_of_field, k_velocity and k_mblur behind those in one with
//                   mr_scene_set_motion_blur, k_velocity and k_taa between k_ao and k_dof in one with
//                   mr_scene_set_temporal_aa, k_bloom_down, k_bloom_up and k_bloom_composite behind k_mblur in one with
//                   mr_scene_set_bloom, k_shaft_source, k_shaft_march and k_shaft_composite in front of those in one with
//                   mr_scene_set_light_shafts, k_lum_hist, k_exposure and k_tone_apply behind the bloom in one with
//                   mr_scene_set_tone_map, k_accum_resolve for the bytes of any; k_layers right behind k_tile in one with
//                   mr_scene_set_layers)
//
// Per-frame work buffers live in a "frame slot".  Every stream a caller renders on gets its own slot, so frames
// enqueued on different streams are independent and may overlap on the device.
//
// Built for gfx950 only, with -ffp-contract=off (see rast_math.h).
#include "../../include/mi355rast.h"
#include "host_overlay.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "rast_types.h"
#include "kernels_geometry.h"
#include "kernels_tile.h"
#include "kernels_overlay.h"
#include "kernels_pose.h"
#include "ao_def.h"
#include "dof_def.h"
#include "motion_def.h"
#include "motion_faces_def.h"
#include "taa_def.h"
#include "bloom_def.h"
#include "shafts_def.h"
#include "tonemap_def.h"
#include "layers_def.h"

#include "host_device.h"
#include "host_env.h"
#include "host_silcache.h"
#include "host_morph.h"
#include "host_autonormals.h"
#include "host_pass.h"
#include "host_scene.h"
#include "host_pose.h"
#include "host_overlay_dev.h"
#include "host_ao.h"
#include "host_dof.h"
#include "host_motion.h"
#include "host_motion_faces.h"
#include "host_taa.h"
#include "host_bloom.h"
#include "host_shafts.h"
#include "host_tonemap.h"
#include "host_layers.h"
#include "host_frame.h"
#include "host_accum.h"
#include "host_post.h"

// ============================================================================ C ABI

static thread_local mr_host::OverlayLists g_overlay_lists;

// mr_scene_set_ambient_occlusion, mr_scene_set_depth_of_field: the description checked and kept for the frames enqueued
// from now on; NULL switches the pass off
template <class Pass, class Desc, class Params>
static int set_pass(mr_scene *sc, Pass mr_scene::*pass, const Desc *d, int (*params)(const Desc *, Params &), int (*pass_linked)())
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    Pass &a = sc->*pass;
    if (!d) { a.on = false; return MR_OK; }      // (frames already enqueued took their copy)
    Params p;
    if (int rc = params(d, p)) return rc;
    if (int rc = pass_linked()) return rc;
    a.params = p;
    a.on = true;
    return MR_OK;
}

// mr_debug_ao, mr_debug_dof, mr_debug_motion
template <class Pass>
static int pass_counts(mr_scene *sc, Pass mr_scene::*pass, int32_t *out)
{
    if (!sc || !out) return fail(MR_E_INVALID, "NULL argument");
    const Pass &a = sc->*pass;
    out[0] = a.frames; out[1] = a.rows; out[2] = a.cols;
    return MR_OK;
}

// the mr_debug_*_times of the passes: the device time of every span (from mark, to mark) of the last frame that ran the pass
template <class Pass>
static int pass_times(mr_scene *sc, Pass mr_scene::*pass, const char *none_yet, float *out_ms, std::initializer_list<std::array<int, 2>> spans)
{
    if (!sc || !out_ms) return fail(MR_E_INVALID, "NULL argument");
    const Pass &a = sc->*pass;
    if (!a.marked) return fail(MR_E_INVALID, none_yet);
    for (const auto &span : spans)
        if (int rc = a.marks.elapsed(span[0], span[1], out_ms++)) return rc;
    return MR_OK;
}

extern "C" {

int mr_abi_version(void) { return MR_ABI_VERSION; }

int mr_abi_struct_size(int which)
{
    static const size_t size[] = { sizeof(mr_frame_desc), sizeof(mr_material), sizeof(mr_model_desc), sizeof(mr_stats),
                                   sizeof(mr_overlay_desc), sizeof(mr_light_desc), sizeof(mr_ao_desc) };
    return which >= 0 && which < 7 ? (int)size[which] : -1;
}

int mr_device_available(void)
{
    int n = 0;
    return (hipGetDeviceCount(&n) == hipSuccess && n > 0) ? 1 : 0;
}

int mr_init(int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(MR_E_DEVICE, "no HIP device visible: libmi355rast has no CPU fallback");
    if (device >= 0) {
        if (device >= n) return fail(MR_E_INVALID, "device index out of range");
        HIP_TRY(hipSetDevice(device));
    }
    return ensure_init();
}

const char *mr_last_error(void) { return g_error.c_str(); }

mr_scene *mr_scene_create(void)
{
    mr_scene *sc = new (std::nothrow) mr_scene();
    if (!sc) fail(MR_E_DEVICE, "out of host memory");
    return sc;
}

int mr_scene_clear(mr_scene *sc)
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    if (g_initialised) (void)hipDeviceSynchronize();
    for (void *p : sc->texture_allocs) (void)hipFree(p);
    sc->texture_allocs.clear(); sc->textures.clear();
    sc->verts.clear(); sc->uv.clear(); sc->normals.clear(); sc->faces.clear(); sc->face_flags.clear();
    sc->materials.clear(); sc->model_face_off.clear(); sc->edges.clear(); sc->edge_inc.clear();
    sc->edge_ids.clear(); sc->edge_raw.clear();
    sc->poses.clear(); sc->pose_dirty = 0;
    sc->skin_tables_dirty = sc->morph_tables_dirty = sc->auto_tables_dirty = true;
    sc->dirty = true;
    sc->last = nullptr;
    sc->sil.drop();
    sc->reset_caps();
    for (auto &fs : sc->slots) fs->reset_caps();
    return MR_OK;
}

int mr_scene_set_extra_lights(mr_scene *sc, const mr_light_desc *lights, int32_t n)
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    if (n < 0 || n > MR_MAX_LIGHTS - 1) return fail(MR_E_INVALID, "a frame has at most MR_MAX_LIGHTS lights: 0 <= n <= 3 extra ones");
    if (n > 0 && !lights) return fail(MR_E_INVALID, "lights is NULL");
    for (int k = 0; k < n; ++k)
        if (lights[k].type < 0 || lights[k].type > 2) return fail(MR_E_INVALID, "unknown light type");
    for (int k = 0; k < n; ++k) {
        const mr_light_desc &d = lights[k];
        sc->extra_lights[k] = light_rec(d.type, d.pos, d.dir, d.color, d.ambient, d.specular_strength, d.att_constant, d.att_linear,
                                        d.att_quadratic, d.spot_edge0, d.spot_edge1);
    }
    sc->n_extra_lights = n;
    return MR_OK;
}

int mr_scene_set_list_capacities(mr_scene *sc, uint32_t small_pairs, uint32_t big_pairs, uint32_t quads, uint32_t work)
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    if (g_initialised) (void)hipDeviceSynchronize();
    if (small_pairs) sc->bin_cap[0] = small_pairs;
    if (big_pairs) sc->bin_cap[1] = big_pairs;
    if (quads) sc->bin_cap[2] = quads;
    if (work) sc->work_cap = std::max(work, (uint32_t)mr::WORK_SHARDS);
    return MR_OK;
}

void mr_scene_destroy(mr_scene *sc)
{
    if (!sc) return;
    mr_scene_clear(sc);
    for (DevBuf *b : { &sc->d_verts, &sc->d_uv, &sc->d_normals, &sc->d_faces, &sc->d_face_flags, &sc->d_materials, &sc->d_textures, &sc->d_edges,
                       &sc->d_edges32, &sc->d_edge_inc, &sc->d_face_n, &sc->d_face_pos, &sc->d_face_attr, &sc->d_clusters, &sc->d_sky, &sc->d_gamma,
                       &sc->d_verts0, &sc->d_pose_rows, &sc->d_pose_blocks, &sc->d_normals0, &sc->d_normal_rows, &sc->d_normal_blocks,
                       &sc->d_texel_rows, &sc->d_texel_blocks, &sc->d_rebaked, &sc->d_skin_joints, &sc->d_skin_weights, &sc->d_skin_owners,
                       &sc->d_bones, &sc->d_skin_rows, &sc->d_skin_blocks, &sc->d_skin_n_rows, &sc->d_skin_n_blocks, &sc->d_morph_slices,
                       &sc->d_morph_target, &sc->d_morph_dx, &sc->d_morph_dy, &sc->d_morph_dz, &sc->d_morph_weights, &sc->d_morph_rows,
                       &sc->d_morph_blocks, &sc->d_morph_n_rows, &sc->d_morph_n_blocks, &sc->d_verts_m, &sc->d_normals_m,
                       &sc->d_auto_slices, &sc->d_auto_faces, &sc->d_auto_rows, &sc->d_auto_blocks, &sc->d_auto_kept })
        b->release();
    for (auto &fs : sc->slots) fs->release();
    sc->sil.release();
    accum_release(sc->accum);
    release_pass(sc->ao); release_pass(sc->dof); release_pass(sc->motion); release_pass(sc->bloom); release_pass(sc->shafts);
    motion_faces_release(sc);
    taa_release(sc);
    tone_release(sc);
    layers_release(sc);
    for (auto &ln : sc->lanes) if (ln.stream) (void)hipStreamDestroy(ln.stream);
    sc->marks_pose.release(); sc->marks_normals.release(); sc->marks_skin.release(); sc->marks_morph.release(); sc->marks_auto.release();
    delete sc;
}

int mr_scene_add_texture(mr_scene *sc, const float *rgb, int32_t h, int32_t w)
{
    if (!sc || !rgb) return fail(MR_E_INVALID, "NULL argument");
    if (h <= 0 || w <= 0) return fail(MR_E_INVALID, "texture size must be positive");
    if (int rc = ensure_init()) return rc;
    void *d = nullptr;
    const size_t bytes = (size_t)h * w * 3 * sizeof(float);
    HIP_TRY(hipMalloc(&d, bytes));
    hipError_t e = hipMemcpy(d, rgb, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); return fail(MR_E_DEVICE, hipGetErrorString(e)); }
    sc->texture_allocs.push_back(d);
    sc->textures.push_back({ static_cast<const float *>(d), h, w });
    sc->dirty = true;
    return (int)sc->textures.size() - 1;
}

int mr_scene_set_skybox(mr_scene *sc, const uint8_t *texels, int32_t size)
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    if (size < 0 || size > 16384 || (size > 0 && !texels)) return fail(MR_E_INVALID, "bad cubemap");
    if (int rc = ensure_init()) return rc;
    HIP_TRY(hipDeviceSynchronize());
    sc->sky_size = 0;
    if (size == 0) return MR_OK;
    const size_t bytes = (size_t)6 * size * size * 3;
    HIP_TRY(sc->d_sky.ensure(bytes));
    HIP_TRY(hipMemcpy(sc->d_sky.p, texels, bytes, hipMemcpyHostToDevice));
    sc->sky_size = size;
    return MR_OK;
}

int mr_scene_set_overlay(mr_scene *sc, const mr_overlay_desc *ov)
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    if (int rc = ensure_init()) return rc;
    sc->ov_pending.set = false;                          // explicit lists supersede cameras left earlier
    sc->ov_points = sc->ov_segments = 0;                 // (frames already enqueued keep the lists of their slot's copy)
    sc->ov_serial += 1;
    if (!ov || ov->n_points <= 0 || ov->n_segments <= 0) return MR_OK;
    if (!ov->seg_first || !ov->seg_count || !ov->target || !ov->z)
        return fail(MR_E_INVALID, "overlay description has NULL arrays");
    if (!frame_size_ok(ov->height, ov->width))
        return fail(MR_E_INVALID, "overlay description: bad frame size");
    const int np = ov->n_points;
    // validate before the kernel trusts them: segments inside the point range, one after the other; targets pixels
    // of the frame the description names.  (Which pixels a segment's points target is free: a segment that touches more
    // of them than the kernel's LDS table may hold is valid, and marked for the kernel's global path below.)
    long long expect = 0;
    for (int s = 0; s < ov->n_segments; ++s) {
        const long long first = ov->seg_first[s], count = ov->seg_count[s];
        if (first != expect || count <= 0 || first + count > np)
            return fail(MR_E_INVALID, "overlay segments must follow each other and cover the point array");
        if (count > mr::OVERLAY_MAX_SEGMENT) return fail(MR_E_INVALID, "overlay segment longer than a frame is wide or high");
        expect = first + count;
    }
    if (expect != np) return fail(MR_E_INVALID, "overlay segments must follow each other and cover the point array");
    int32_t max_target = -1;
    for (size_t i = 0; i < (size_t)mr::OVERLAY_TARGETS * np; ++i) {
        if (ov->target[i] < 0) return fail(MR_E_INVALID, "negative overlay target");
        max_target = std::max(max_target, ov->target[i]);
    }
    if ((long long)max_target >= (long long)ov->width * ov->height)
        return fail(MR_E_INVALID, "overlay description: targets outside the height x width it names");
    sc->ov_target.assign(ov->target, ov->target + (size_t)mr::OVERLAY_TARGETS * np);
    sc->ov_z.assign(ov->z, ov->z + np);
    sc->ov_seg.resize((size_t)2 * ov->n_segments);
    for (int i = 0; i < ov->n_segments; ++i) { sc->ov_seg[2 * i] = ov->seg_first[i]; sc->ov_seg[2 * i + 1] = ov->seg_count[i]; }
    mark_global_segments(sc);
    const int tiles_x = (ov->width + mr::TILE_W - 1) / mr::TILE_W, tiles_y = (ov->height + mr::TILE_H - 1) / mr::TILE_H;
    sc->ov_tile_mask.assign((size_t)tiles_x * tiles_y, 0);
    for (int32_t t : sc->ov_target) sc->ov_tile_mask[(size_t)(t / ov->width / mr::TILE_H) * tiles_x + (size_t)(t % ov->width / mr::TILE_W)] = 1;
    sc->ov_height = ov->height; sc->ov_width = ov->width;
    sc->ov_points = np; sc->ov_segments = ov->n_segments;
    return MR_OK;
}

int mr_scene_set_overlay_cameras(mr_scene *sc, const double *corners, const double *planes, const double *mvp,
                                 const double *viewport, double near_, double far_, int32_t camera_inside,
                                 int32_t height, int32_t width)
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    if (!corners || !planes || !mvp || !viewport || !frame_size_ok(height, width))
        return fail(MR_E_INVALID, "mr_scene_set_overlay_cameras: bad argument");
    if (int rc = ensure_init()) return rc;
    mr_scene::OvPending &p = sc->ov_pending;
    std::memcpy(p.corners, corners, sizeof p.corners); std::memcpy(p.planes, planes, sizeof p.planes);
    std::memcpy(p.mvp, mvp, sizeof p.mvp); std::memcpy(p.viewport, viewport, sizeof p.viewport);
    p.near_ = near_; p.far_ = far_; p.inside = camera_inside; p.height = height; p.width = width;
    p.set = true;
    return MR_OK;
}

int mr_scene_add_model(mr_scene *sc, const mr_model_desc *m)
{
    if (!sc || !m) return fail(MR_E_INVALID, "NULL argument");
    if (!m->vertices || !m->faces || !m->materials || m->n_vertices <= 0 || m->n_faces < 0 || m->n_materials <= 0)
        return fail(MR_E_INVALID, "model needs vertices, faces and at least one material");
    const int n_tex = (int)sc->textures.size();
    for (int i = 0; i < m->n_materials; ++i) {
        const mr_material &mm = m->materials[i];
        if (mm.tex_kd >= n_tex || mm.tex_norm >= n_tex || mm.tex_ks >= n_tex)
            return fail(MR_E_INVALID, "material refers to a texture id that was never added");
        if ((mm.tex_kd >= 0 || mm.tex_norm >= 0 || mm.tex_ks >= 0) && !m->uv)
            return fail(MR_E_INVALID, "textured material on a model without uv coordinates");
        if (mm.tex_norm >= 0 && mm.norm_tangent && !m->normals)
            return fail(MR_E_INVALID, "tangent-space normal map on a model without vertex normals");
    }
    // where this model's arrays start in the scene's
    const int32_t vert_off = (int32_t)(sc->verts.size() / 4), uv_off = (int32_t)(sc->uv.size() / 3), normal_off = (int32_t)(sc->normals.size() / 3);
    const int32_t face_off = (int32_t)(sc->faces.size() / 12), mat_off = (int32_t)sc->materials.size();
    // validate indices before touching the scene: the kernels trust them
    for (int64_t i = 0; i < (int64_t)m->n_faces * 3; ++i) {
        const int32_t *c = m->faces + i * 4;
        if (c[0] < 0 || c[0] >= m->n_vertices) return fail(MR_E_INVALID, "vertex index out of range");
        if (m->uv && (c[1] < 0 || c[1] >= m->n_uv)) return fail(MR_E_INVALID, "uv index out of range");
        if (m->normals && (c[2] < 0 || c[2] >= m->n_normals)) return fail(MR_E_INVALID, "normal index out of range");
        if (c[3] < 0 || c[3] >= m->n_materials) return fail(MR_E_INVALID, "material index out of range");
        if (m->edge_ids && (m->edge_ids[i] < -m->n_vertices || m->edge_ids[i] >= m->n_vertices))
            return fail(MR_E_INVALID, "edge id out of range");
    }
    if (g_initialised) (void)hipDeviceSynchronize();     // frames in flight still use the old scene
    sc->verts.insert(sc->verts.end(), m->vertices, m->vertices + (size_t)m->n_vertices * 4);
    if (m->uv) sc->uv.insert(sc->uv.end(), m->uv, m->uv + (size_t)m->n_uv * 3);
    if (m->normals) sc->normals.insert(sc->normals.end(), m->normals, m->normals + (size_t)m->n_normals * 3);
    for (int i = 0; i < m->n_materials; ++i) {
        const mr_material &mm = m->materials[i];
        mr::Material d;
        for (int j = 0; j < 3; ++j) { d.kd[j] = mm.kd[j]; d.ks255[j] = mm.ks255[j]; }
        d.ns = mm.ns; d.tex_kd = mm.tex_kd; d.tex_norm = mm.tex_norm; d.tex_ks = mm.tex_ks;
        d.norm_tangent = mm.norm_tangent;
        sc->materials.push_back(d);
    }
    const uint8_t ff = (uint8_t)((m->clip ? mr::FF_CLIP : 0) | (m->vertices_are_f32 ? mr::FF_VERTS_F32 : 0) |
                                 (m->normals ? mr::FF_HAS_NORMALS : 0) | (m->uv ? mr::FF_HAS_UV : 0) |
                                 (m->depth_test ? 0 : mr::FF_NO_DEPTH));
    sc->faces.reserve(sc->faces.size() + (size_t)m->n_faces * 12);
    for (int64_t i = 0; i < (int64_t)m->n_faces * 3; ++i) {
        const int32_t *c = m->faces + i * 4;
        sc->faces.push_back(c[0] + vert_off);
        sc->faces.push_back(m->uv ? c[1] + uv_off : 0);
        sc->faces.push_back(m->normals ? c[2] + normal_off : 0);
        sc->faces.push_back(c[3] + mat_off);
    }
    sc->face_flags.insert(sc->face_flags.end(), (size_t)m->n_faces, ff);
    // silhouette edges are matched on the corners' RAW vertex ids (see mr_model_desc.edge_ids): raw values
    // lie in [-n_vertices, n_vertices); shifted by n_vertices + 2 * vert_off they are unique per model
    for (int64_t i = 0; i < (int64_t)m->n_faces * 3; ++i) {
        const int32_t raw = m->edge_ids ? m->edge_ids[i] : m->faces[i * 4];
        sc->edge_raw.push_back(raw);
        sc->edge_ids.push_back(raw + m->n_vertices + 2 * vert_off);
    }
    sc->model_face_off.push_back(face_off);
    mr_scene::ModelPose mp;
    mp.vert_off = vert_off; mp.n_verts = m->n_vertices; mp.verts_f32 = m->vertices_are_f32 != 0;
    mp.normal_off = normal_off; mp.n_normals = m->normals ? m->n_normals : 0;
    mp.mat_off = mat_off; mp.n_mats = m->n_materials;
    sc->poses.push_back(mp);
    sc->dirty = true;
    sc->last = nullptr;
    sc->quad_cap = 0;
    for (auto &fs : sc->slots) fs->reset_caps();
    return (int)sc->model_face_off.size() - 1;
}

int mr_scene_set_model_pose(mr_scene *sc, int32_t model, const double *m16)
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    if (model < 0 || (size_t)model >= sc->poses.size()) return fail(MR_E_INVALID, "model index out of range");
    if (m16)
        for (int i = 0; i < 16; ++i)
            if (!std::isfinite(m16[i])) return fail(MR_E_INVALID, "a pose matrix must be finite");
    set_model_pose(sc, model, m16);
    return MR_OK;
}

int mr_scene_set_model_pose_normals(mr_scene *sc, int32_t model, const double *g9)
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    if (model < 0 || (size_t)model >= sc->poses.size()) return fail(MR_E_INVALID, "model index out of range");
    if (!sc->poses[model].posed) return fail(MR_E_INVALID, "a normal matrix needs a model that has a pose");
    if (g9)
        for (int i = 0; i < 9; ++i)
            if (!std::isfinite(g9[i])) return fail(MR_E_INVALID, "a normal matrix must be finite");
    set_model_pose_normals(sc, model, g9);
    return MR_OK;
}

int mr_scene_set_model_skin(mr_scene *sc, int32_t model, const int32_t *joints, const double *weights, int32_t n_bones,
                            const int32_t *normal_owner)
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    if (model < 0 || (size_t)model >= sc->poses.size()) return fail(MR_E_INVALID, "model index out of range");
    const mr_scene::ModelPose &mp = sc->poses[model];
    if (joints) {                                    // validated before the kernels trust them
        if (!weights || n_bones <= 0) return fail(MR_E_INVALID, "a skin needs joints, weights and at least one bone");
        for (size_t i = 0; i < (size_t)mp.n_verts * 4; ++i) {
            if (joints[i] < 0 || joints[i] >= n_bones) return fail(MR_E_INVALID, "joint index out of range");
            if (!std::isfinite(weights[i])) return fail(MR_E_INVALID, "skin weights must be finite");
        }
        if (normal_owner)
            for (int32_t i = 0; i < mp.n_normals; ++i)
                if (normal_owner[i] < -1 || normal_owner[i] >= mp.n_verts) return fail(MR_E_INVALID, "normal owner out of range");
    }
    set_model_skin(sc, model, joints, weights, n_bones, normal_owner);
    return MR_OK;
}

int mr_scene_set_model_bones(mr_scene *sc, int32_t model, const double *bones16, int32_t n_bones)
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    if (model < 0 || (size_t)model >= sc->poses.size()) return fail(MR_E_INVALID, "model index out of range");
    const mr_scene::ModelPose &mp = sc->poses[model];
    if (mp.n_bones == 0) return fail(MR_E_INVALID, "bones need a model that has a skin");
    if (bones16) {
        if (n_bones != mp.n_bones) return fail(MR_E_INVALID, "the skin was set for another number of bones");
        for (size_t i = 0; i < (size_t)n_bones * 16; ++i)
            if (!std::isfinite(bones16[i])) return fail(MR_E_INVALID, "bone matrices must be finite");
    }
    set_model_bones(sc, model, bones16);
    return MR_OK;
}

int mr_scene_set_model_morph(mr_scene *sc, int32_t model, int32_t n_targets, const int32_t *first, const int32_t *index,
                             const double *delta, const int32_t *nfirst, const int32_t *nindex, const double *ndelta)
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    if (model < 0 || (size_t)model >= sc->poses.size()) return fail(MR_E_INVALID, "model index out of range");
    const mr_scene::ModelPose &mp = sc->poses[model];
    if (first) {                                     // validated before the kernels trust them
        if (const char *wrong = mr_morph::check_tables(mp.n_verts, n_targets, first, index, delta)) return fail(MR_E_INVALID, wrong);
        if (nfirst) {
            if (mp.n_normals == 0) return fail(MR_E_INVALID, "normal targets on a model without normals");
            if (const char *wrong = mr_morph::check_tables(mp.n_normals, n_targets, nfirst, nindex, ndelta)) return fail(MR_E_INVALID, wrong);
        }
    }
    return set_model_morph(sc, model, n_targets, first, index, delta, nfirst, nindex, ndelta);
}

int mr_scene_set_model_morph_weights(mr_scene *sc, int32_t model, const double *w, int32_t n_targets)
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    if (model < 0 || (size_t)model >= sc->poses.size()) return fail(MR_E_INVALID, "model index out of range");
    const mr_scene::ModelPose &mp = sc->poses[model];
    if (mp.n_targets == 0) return fail(MR_E_INVALID, "morph weights need a model that has a morph");
    if (w) {
        if (n_targets != mp.n_targets) return fail(MR_E_INVALID, "the morph was set for another number of targets");
        for (int32_t k = 0; k < n_targets; ++k)
            if (!std::isfinite(w[k])) return fail(MR_E_INVALID, "morph weights must be finite");
    }
    set_model_morph_weights(sc, model, w);
    return MR_OK;
}

int mr_scene_set_model_auto_normals(mr_scene *sc, int32_t model, int32_t on)
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    if (model < 0 || (size_t)model >= sc->poses.size()) return fail(MR_E_INVALID, "model index out of range");
    if (on != 0 && on != 1) return fail(MR_E_INVALID, "auto_normals is 0 or 1");
    return set_model_auto_normals(sc, model, on != 0);
}

int mr_render(mr_scene *sc, const mr_frame_desc *fr, uint8_t *out_rgb, mr_stats *stats)
{
    if (!sc || !out_rgb) return fail(MR_E_INVALID, "NULL argument");
    int rc = validate_frame(sc, fr);
    if (rc) return rc;
    if ((rc = ensure_init())) return rc;
    FrameSlot *fs = slot_for(sc, g_stream);
    if (!fs) return fail(MR_E_DEVICE, "out of frame slots");
    if ((fr->flags & MR_FRAME_OVERLAY) && is_partial(fr))
        return fail(MR_E_INVALID, "the overlay of a frame split over devices is drawn on the assembled whole frame: render the "
                                  "part with mr_render_device (which appends the touched pixels' state), then mr_overlay_apply");
    mr_frame_desc counted = *fr;
    if (stats) counted.flags |= MR_FRAME_COUNTERS;         // whoever asks for the counters gets them
    fr = &counted;
    for (int attempt = 0; attempt < 6; ++attempt) {
        if ((rc = render_and_copy(sc, fs, fr, out_rgb, stats != nullptr))) { frame_settled(sc, fs, false); return rc; }
        const hipError_t drained = hipStreamSynchronize(g_stream);
        if (drained != hipSuccess) frame_settled(sc, fs, false);
        HIP_TRY(drained);
        rc = collect(sc, fs, true);
        frame_settled(sc, fs, rc == MR_OK);          // (a frame that overflowed adopts nothing: the next attempt reads the same history)
        if (rc == MR_OK) {
            if (stats) *stats = sc->stats;
            return MR_OK;
        }
        if (rc != MR_E_OVERFLOW) return rc;       // work lists were grown: render the frame again
    }
    return fail(MR_E_OVERFLOW, "work lists kept overflowing");
}

int mr_render_async(mr_scene *sc, const mr_frame_desc *fr, uint8_t *out_rgb, int32_t lane)
{
    if (!sc || !out_rgb) return fail(MR_E_INVALID, "NULL argument");
    if (lane < 0 || lane >= MR_ASYNC_LANES) return fail(MR_E_INVALID, "lane out of range");
    int rc = validate_frame(sc, fr);
    if (rc) return rc;
    if ((rc = ensure_init())) return rc;
    if ((fr->flags & MR_FRAME_OVERLAY) && is_partial(fr))
        return fail(MR_E_INVALID, "the overlay of a frame split over devices is drawn on the assembled whole frame (mr_overlay_apply)");
    mr_scene::Lane &ln = sc->lanes[lane];
    if (ln.busy) return fail(MR_E_INVALID, "this lane still has a frame in flight: mr_render_wait first");
    if (!ln.stream) HIP_TRY(hipStreamCreateWithFlags(&ln.stream, hipStreamNonBlocking));
    FrameSlot *fs = slot_for(sc, ln.stream);
    if (!fs) return fail(MR_E_DEVICE, "out of frame slots");
    if ((rc = render_and_copy(sc, fs, fr, out_rgb, (fr->flags & MR_FRAME_COUNTERS) != 0))) { frame_settled(sc, fs, false); return rc; }
    ln.busy = true;
    return MR_OK;
}

int mr_render_wait(mr_scene *sc, int32_t lane, mr_stats *stats)
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    if (lane < 0 || lane >= MR_ASYNC_LANES) return fail(MR_E_INVALID, "lane out of range");
    mr_scene::Lane &ln = sc->lanes[lane];
    if (!ln.busy) return fail(MR_E_INVALID, "no frame in flight on this lane");
    FrameSlot *fs = slot_for(sc, ln.stream);
    const hipError_t drained = hipStreamSynchronize(ln.stream);
    if (drained != hipSuccess && fs) frame_settled(sc, fs, false);
    HIP_TRY(drained);
    ln.busy = false;
    if (!fs) return fail(MR_E_DEVICE, "lane without a frame slot");
    const int rc = collect(sc, fs, true);
    frame_settled(sc, fs, rc == MR_OK);
    if (stats) *stats = sc->stats;
    if (rc == MR_E_OVERFLOW) return fail(MR_E_OVERFLOW, "the frame overflowed a work list (now grown): render it again");
    return rc;
}

int mr_accum_begin(mr_scene *sc)
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    mr_scene::Accum &a = sc->accum;                  // (the buffer and the events stay for the next accumulation)
    a.width = a.height = a.ss_flags = 0;
    a.count = a.rerendered = 0;
    a.add_marked = a.resolve_marked = false;
    return MR_OK;
}

int mr_accum_add(mr_scene *sc, const mr_frame_desc *fr, double weight)
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    return accum_add(sc, fr, weight);
}

int mr_accum_resolve(mr_scene *sc, double scale, uint8_t *out_rgb)
{
    if (!sc || !out_rgb) return fail(MR_E_INVALID, "NULL argument");
    return accum_resolve(sc, scale, out_rgb);
}

int mr_accum_read_f32(mr_scene *sc, float *out)
{
    if (!sc || !out) return fail(MR_E_INVALID, "NULL argument");
    const mr_scene::Accum &a = sc->accum;
    if (a.count == 0) return fail(MR_E_INVALID, "nothing accumulated yet");
    return read_back(a.d_acc, out, (size_t)a.width * a.height * 3, "accumulation");
}

int mr_debug_accum(mr_scene *sc, int32_t *out)
{
    if (!sc || !out) return fail(MR_E_INVALID, "NULL argument");
    const mr_scene::Accum &a = sc->accum;
    out[0] = a.count; out[1] = a.rerendered; out[2] = a.height; out[3] = a.width;
    return MR_OK;
}

int mr_debug_accum_times(mr_scene *sc, float *out_ms)
{
    if (!sc || !out_ms) return fail(MR_E_INVALID, "NULL argument");
    const mr_scene::Accum &a = sc->accum;
    if (!a.add_marked) return fail(MR_E_INVALID, "nothing accumulated yet");
    if (int rc = a.marks.elapsed(0, 1, &out_ms[0])) return rc;      // (mr_accum_add does not wait for its kernel)
    out_ms[1] = 0.f;                                 // (no mr_accum_resolve since mr_accum_begin)
    return a.resolve_marked ? a.marks.elapsed(2, 3, &out_ms[1]) : MR_OK;
}

int mr_host_accum(const float *frames, const double *weights, int32_t n, int32_t height, int32_t width, int32_t shift, double scale,
                  float *out_acc, uint8_t *out_rgb)
{
    return host_accum(frames, weights, n, height, width, shift, scale, out_acc, out_rgb);
}

int mr_scene_set_ambient_occlusion(mr_scene *sc, const mr_ao_desc *ao)
{
    return set_pass(sc, &mr_scene::ao, ao, ao_params, ao_linked);
}

int mr_host_ao(const double *z, const float *frame, int32_t height, int32_t width, const mr_ao_desc *ao, float *out_frame)
{
    return host_ao(z, frame, height, width, ao, out_frame);
}

int mr_debug_ao(mr_scene *sc, int32_t *out)
{
    return pass_counts(sc, &mr_scene::ao, out);
}

int mr_debug_ao_times(mr_scene *sc, float *out_ms)
{
    return pass_times(sc, &mr_scene::ao, "no frame with ambient occlusion yet", out_ms, { { 0, 1 } });
}

int mr_scene_set_depth_of_field(mr_scene *sc, const mr_dof_desc *dof)
{
    return set_pass(sc, &mr_scene::dof, dof, dof_params, dof_linked);
}

int mr_host_dof(const double *z, const float *frame, int32_t height, int32_t width, const mr_dof_desc *dof, float *out_frame)
{
    return host_dof(z, frame, height, width, dof, out_frame);
}

int mr_debug_dof(mr_scene *sc, int32_t *out)
{
    return pass_counts(sc, &mr_scene::dof, out);
}

int mr_debug_dof_times(mr_scene *sc, float *out_ms)
{
    return pass_times(sc, &mr_scene::dof, "no frame with depth of field yet", out_ms, { { 0, 1 } });
}

int mr_debug_post(mr_scene *sc, const float *frames, const double *z, int32_t n, int32_t height, int32_t width, const mr_ao_desc *ao,
                  int32_t ao_shape, const mr_dof_desc *dof, int32_t dof_shape, const double *weights, int32_t shift, double scale,
                  float *out_f32, uint8_t *out_rgb)
{
    return debug_post(sc, frames, z, n, height, width, ao, ao_shape, dof, dof_shape, weights, shift, scale, out_f32, out_rgb);
}

int mr_scene_set_motion_blur(mr_scene *sc, const mr_motion_desc *motion)
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    if (!motion) { sc->motion.on = false; return MR_OK; }      // (frames already enqueued took their copy)
    if (motion->n_models != (int32_t)sc->model_face_off.size())
        return fail(MR_E_INVALID, "motion blur: n_models is not the number of the scene's models");
    mr::MotionParams p;
    std::vector<double> tables;
    if (int rc = motion_params(motion, sc->model_face_off.data(), p, tables)) return rc;
    if (int rc = motion_linked()) return rc;
    sc->motion.params = p;
    sc->motion.tables.swap(tables);
    sc->motion.on = true;
    return MR_OK;
}

int mr_host_velocity(const double *z, const int32_t *winner, const int32_t *face_off, int32_t height, int32_t width,
                     const mr_motion_desc *motion, float *out_velocity)
{
    return host_velocity(z, winner, face_off, height, width, motion, out_velocity);
}

int mr_host_motion_blur(const double *z, const float *velocity, const float *frame, int32_t height, int32_t width,
                        const mr_motion_desc *motion, float *out_frame)
{
    return host_motion_blur(z, velocity, frame, height, width, motion, out_frame);
}

int mr_read_velocity(mr_scene *sc, float *out)
{
    FrameSlot *fs = last_slot(sc);
    if (!fs) return MR_E_INVALID;
    if (!fs->last_motion) return fail(MR_E_INVALID, "the last frame was rendered without motion blur");
    return read_back(fs->motion.d_vel, out, (size_t)fs->last_frame.width * fs->last_frame.height * 2, "velocity");
}

int mr_debug_motion(mr_scene *sc, int32_t *out)
{
    return pass_counts(sc, &mr_scene::motion, out);
}

int mr_debug_motion_times(mr_scene *sc, float *out_ms)
{
    // (a frame whose U the temporal anti-aliasing computed ran no k_velocity of its own: its velocity span is 0)
    const int rc = pass_times(sc, &mr_scene::motion, "no frame with motion blur yet", out_ms, { { 0, 1 }, { sc ? sc->motion.blur_from : 1, 3 } });
    if (rc == MR_OK && sc->motion.vel_skipped) out_ms[0] = 0.f;
    return rc;
}

int mr_debug_motion_post(mr_scene *sc, const double *z, const int32_t *winner, const float *frame, const int32_t *face_off, int32_t height,
                         int32_t width, const mr_motion_desc *motion, int32_t shape, float *out_velocity, float *out_frame)
{
    return debug_motion_post(sc, z, winner, frame, face_off, height, width, motion, shape, out_velocity, out_frame);
}

int mr_scene_set_temporal_aa(mr_scene *sc, const mr_taa_desc *taa)
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    if (!taa) {                                                // (frames already enqueued took their copy)
        if (sc->taa.on) taa_forget(sc);
        sc->taa.on = false;
        return MR_OK;
    }
    if (taa->n_models != (int32_t)sc->model_face_off.size())
        return fail(MR_E_INVALID, "temporal anti-aliasing: n_models is not the number of the scene's models");
    mr::TaaParams p;
    mr::MotionParams vel;
    std::vector<double> tables;
    if (int rc = taa_params(taa, sc->model_face_off.data(), p, vel, tables)) return rc;
    if (int rc = taa_linked()) return rc;
    sc->taa.params = p;
    sc->taa.vel = vel;
    sc->taa.tables.swap(tables);
    sc->taa.on = true;
    return MR_OK;
}

int mr_scene_reset_history(mr_scene *sc)
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    taa_forget(sc);
    return MR_OK;
}

int mr_read_history(mr_scene *sc, float *out)
{
    if (!sc || !out) return fail(MR_E_INVALID, "NULL argument");
    const mr_scene::Taa &a = sc->taa;
    if (!a.valid) return fail(MR_E_INVALID, "no temporal anti-aliasing history yet: none adopted since it was last forgotten");
    return read_back(a.d_hist[a.cur], out, (size_t)a.hist_rows * a.hist_cols * 3, "history");
}

int mr_host_taa(const float *frame, const float *velocity, const float *history, int32_t height, int32_t width, double blend, float *out_frame)
{
    return host_taa(frame, velocity, history, height, width, blend, out_frame);
}

int mr_debug_taa_post(mr_scene *sc, const float *frame, const float *velocity, const float *history, int32_t height, int32_t width, double blend,
                      int32_t shape, float *out_frame, float *out_history, int32_t *out_guard)
{
    return debug_taa_post(sc, frame, velocity, history, height, width, blend, shape, out_frame, out_history, out_guard);
}

int mr_debug_taa(mr_scene *sc, int32_t *out)
{
    if (int rc = pass_counts(sc, &mr_scene::taa, out)) return rc;
    out[3] = sc->taa.velocities; out[4] = sc->taa.adopted; out[5] = sc->taa.valid ? 1 : 0;
    return MR_OK;
}

int mr_debug_taa_times(mr_scene *sc, float *out_ms)
{
    return pass_times(sc, &mr_scene::taa, "no frame with temporal anti-aliasing yet", out_ms, { { 0, 1 }, { 1, 2 } });
}

int mr_scene_set_bloom(mr_scene *sc, const mr_bloom_desc *bloom)
{
    return set_pass(sc, &mr_scene::bloom, bloom, bloom_params, bloom_linked);
}

int mr_host_bloom(const float *frame, int32_t height, int32_t width, const mr_bloom_desc *bloom, float *out_frame, float *out_pyramid)
{
    return host_bloom(frame, height, width, bloom, out_frame, out_pyramid);
}

int mr_debug_bloom(mr_scene *sc, int32_t *out)
{
    if (int rc = pass_counts(sc, &mr_scene::bloom, out)) return rc;
    out[3] = sc->bloom.last_levels;
    return MR_OK;
}

int mr_debug_bloom_times(mr_scene *sc, float *out_ms)
{
    return pass_times(sc, &mr_scene::bloom, "no frame with bloom yet", out_ms, { { 0, 1 }, { 1, 2 }, { 2, 3 } });
}

int mr_debug_bloom_post(mr_scene *sc, const float *frame, int32_t height, int32_t width, const mr_bloom_desc *bloom, int32_t shape,
                        float *out_frame, float *out_pyramid)
{
    return debug_bloom_post(sc, frame, height, width, bloom, shape, out_frame, out_pyramid);
}

int mr_scene_set_light_shafts(mr_scene *sc, const mr_light_shafts_desc *shafts)
{
    return set_pass(sc, &mr_scene::shafts, shafts, shafts_params, shafts_linked);
}

int mr_host_light_shafts(const float *frame, const double *zbuf, int32_t height, int32_t width, const mr_light_shafts_desc *shafts, float *out_frame,
                         float *out_source, float *out_march)
{
    return host_light_shafts(frame, zbuf, height, width, shafts, out_frame, out_source, out_march);
}

int mr_debug_light_shafts(mr_scene *sc, int32_t *out)
{
    if (int rc = pass_counts(sc, &mr_scene::shafts, out)) return rc;
    out[3] = sc->shafts.last_levels;
    return MR_OK;
}

int mr_debug_light_shafts_times(mr_scene *sc, float *out_ms)
{
    return pass_times(sc, &mr_scene::shafts, "no frame with light shafts yet", out_ms, { { 0, 1 }, { 1, 2 }, { 2, 3 } });
}

int mr_debug_light_shafts_post(mr_scene *sc, const float *frame, const double *zbuf, int32_t height, int32_t width, const mr_light_shafts_desc *shafts,
                               float *out_frame, float *out_source, float *out_march)
{
    return debug_light_shafts_post(sc, frame, zbuf, height, width, shafts, out_frame, out_source, out_march);
}

int mr_scene_set_tone_map(mr_scene *sc, const mr_tone_map_desc *tone_map)
{
    const int rc = set_pass(sc, &mr_scene::tone, tone_map, tone_params, tonemap_linked);
    if (rc == MR_OK) tone_forget(sc);                          // (off, or another description: the exposure it adapted is not this one's)
    return rc;
}

int mr_scene_reset_exposure(mr_scene *sc)
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    tone_forget(sc);
    return MR_OK;
}

int mr_host_tone_map(const float *frame, int32_t height, int32_t width, const mr_tone_map_desc *tone_map, int32_t has_prev, float e_prev,
                     float *out_frame, uint32_t *out_hist, float *out_exposure)
{
    return host_tone_map(frame, height, width, tone_map, has_prev, e_prev, out_frame, out_hist, out_exposure);
}

// the words of the last frame's slot where that frame ran the pass, from word `first`
static int read_tone_words(mr_scene *sc, size_t first, size_t count, void *out, bool metered_only)
{
    if (!out) return fail(MR_E_INVALID, "NULL argument");
    FrameSlot *fs = last_slot(sc);
    if (!fs) return MR_E_INVALID;
    if (!fs->last_tone) return fail(MR_E_INVALID, "the last frame was rendered without tone mapping");
    if (fs->last_tone == 2 && metered_only) return fail(MR_E_INVALID, "the last frame's exposure was fixed: nothing was metered");
    if (fs->last_tone == 2) { std::memcpy(out, &fs->last_tone_exposure, sizeof(float)); return MR_OK; }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, fs->d_tone.as<uint32_t>() + first, count * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return MR_OK;
}

int mr_read_exposure(mr_scene *sc, float *out)
{
    return read_tone_words(sc, TONE_SLOT_CELL, 1, out, false);
}

int mr_read_luminance_histogram(mr_scene *sc, uint32_t *out)
{
    return read_tone_words(sc, TONE_SLOT_HIST, mr::TONE_BINS, out, true);
}

int mr_debug_tone_map(mr_scene *sc, int32_t *out)
{
    if (int rc = pass_counts(sc, &mr_scene::tone, out)) return rc;
    out[3] = sc->tone.last_grid; out[4] = sc->tone.adopted; out[5] = sc->tone.valid ? 1 : 0;
    return MR_OK;
}

int mr_debug_tone_map_times(mr_scene *sc, float *out_ms)
{
    return pass_times(sc, &mr_scene::tone, "no frame with tone mapping yet", out_ms, { { 0, 1 }, { 1, 2 }, { 2, 3 } });
}

int mr_debug_tone_map_post(mr_scene *sc, const float *frame, int32_t height, int32_t width, const mr_tone_map_desc *tone_map, int32_t has_prev,
                           float e_prev, int32_t grid_cap, int32_t form, float *out_frame, uint32_t *out_hist, float *out_exposure, float *out_ms)
{
    return debug_tone_map_post(sc, frame, height, width, tone_map, has_prev, e_prev, grid_cap, form, out_frame, out_hist, out_exposure, out_ms);
}

int mr_scene_set_layers(mr_scene *sc, const mr_layers_desc *layers)
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    if (!layers) { sc->layers.on = false; return MR_OK; }      // (frames already enqueued took their copy)
    mr::LayersParams p;
    if (int rc = layers_params(layers, 0, p)) return rc;
    if (layers->n_models != (int32_t)sc->model_face_off.size())
        return fail(MR_E_INVALID, "data layers: n_models is not the number of the scene's models");
    if (int rc = layers_linked()) return rc;
    sc->layers.params = p;
    sc->layers.on = true;
    return MR_OK;
}

int mr_read_layers(mr_scene *sc, int32_t layer, void *out)
{
    FrameSlot *fs = last_slot(sc);
    if (!fs) return MR_E_INVALID;
    if (layer < 0 || layer >= mr::N_LAYERS) return fail(MR_E_INVALID, "data layers: no such layer");
    if (!fs->last_layers) return fail(MR_E_INVALID, "the last frame was rendered without data layers");
    if (!(fs->last_layers & (1 << layer))) return fail(MR_E_INVALID, "the last frame was rendered without this layer");
    return read_back(fs->layers.d[layer], static_cast<uint32_t *>(out),
                     (size_t)fs->last_frame.width * fs->last_frame.height * mr::layer_words(layer), "data layers");
}

int mr_host_layers(const int32_t *winner, int32_t height, int32_t width, const void *face_pos, int32_t pos32, const float *face_attr,
                   int32_t n_faces, const int32_t *face_off, const mr_layers_desc *layers, void *const *out, int64_t *out_degenerate)
{
    return host_layers(winner, height, width, face_pos, pos32, face_attr, n_faces, face_off, layers, out, out_degenerate);
}

int mr_debug_layers(mr_scene *sc, int32_t *out)
{
    if (int rc = pass_counts(sc, &mr_scene::layers, out)) return rc;
    out[3] = sc->layers.last_mask;
    return MR_OK;
}

int mr_debug_layers_times(mr_scene *sc, float *out_ms)
{
    return pass_times(sc, &mr_scene::layers, "no frame with data layers yet", out_ms, { { 0, 1 } });
}

int mr_debug_layers_post(mr_scene *sc, const int32_t *winner, int32_t height, int32_t width, const void *face_pos, int32_t pos32,
                         const float *face_attr, int32_t n_faces, const int32_t *face_off, const mr_layers_desc *layers, void *const *out,
                         int32_t *out_guard, float *out_ms)
{
    return debug_layers_post(sc, winner, height, width, face_pos, pos32, face_attr, n_faces, face_off, layers, out, out_guard, out_ms);
}

int mr_debug_read_face_records(mr_scene *sc, void *out_pos, void *out_attr, int32_t *out_info)
{
    if (!sc || !out_info) return fail(MR_E_INVALID, "NULL argument");
    if ((out_pos == nullptr) != (out_attr == nullptr)) return fail(MR_E_INVALID, "mr_debug_read_face_records: out_pos and out_attr go together");
    if (sc->dirty || sc->pose_dirty) return fail(MR_E_INVALID, "the scene has uncommitted changes: render a frame first");
    const size_t nf = sc->faces.size() / 12;
    out_info[0] = (int32_t)nf; out_info[1] = sc->pos32 ? 1 : 0;
    if (!out_pos || nf == 0) return MR_OK;
    if (int rc = read_back(sc->d_face_pos, static_cast<unsigned char *>(out_pos), nf * (sc->pos32 ? sizeof(mr::FacePos32) : sizeof(mr::FacePos64)), "face records")) return rc;
    return read_back(sc->d_face_attr, static_cast<unsigned char *>(out_attr), nf * sizeof(mr::FaceAttr), "face records");
}

int mr_scene_set_motion_faces(mr_scene *sc, const mr_motion_faces_desc *d)
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    if (!d) { sc->mfaces.on = false; return MR_OK; }          // (frames already enqueued have run their pass)
    if (!sc->motion.on) return fail(MR_E_INVALID, "per-face velocity: the scene has no motion blur (mr_scene_set_motion_blur comes first)");
    if (d->n_models != (int32_t)sc->model_face_off.size())
        return fail(MR_E_INVALID, "per-face velocity: n_models is not the number of the scene's models");
    if (d->n_models > 0 && !d->deforming) return fail(MR_E_INVALID, "per-face velocity: deforming is NULL");
    if (!motion_faces_finite(d->s_now, d->s_prev)) return fail(MR_E_INVALID, "per-face velocity: an entry of s_now or s_prev is not finite");
    if (int rc = motion_faces_linked()) return rc;
    mr_scene::MotionFaces &a = sc->mfaces;
    std::memcpy(a.s_now, d->s_now, sizeof a.s_now); std::memcpy(a.s_prev, d->s_prev, sizeof a.s_prev);
    a.deforming.assign(d->deforming, d->deforming + d->n_models);
    a.prev_serial = d->prev_serial;
    a.on = true;
    return MR_OK;
}

int mr_scene_track_vertices(mr_scene *sc, int32_t on)
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    sc->track_verts = on != 0;
    if (!on) sc->snap_valid = false;                           // (what a later pass finds is no previous frame's)
    return MR_OK;
}

int64_t mr_scene_vertices_serial(mr_scene *sc)
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    return sc->vert_serial;
}

int mr_host_face_homographies(const double *verts_now, const double *verts_prev, int32_t n_verts, const int32_t *faces, int32_t n_faces,
                              const double *s_now, const double *s_prev, double *out_h)
{
    return host_face_homographies(verts_now, verts_prev, n_verts, faces, n_faces, s_now, s_prev, out_h);
}

int mr_host_velocity_faces(const int32_t *winner, const int32_t *face_off, const int32_t *hom_off, int32_t n_models, const double *h,
                           int32_t n_records, int32_t height, int32_t width, float *velocity_in_out)
{
    return host_velocity_faces(winner, face_off, hom_off, n_models, h, n_records, height, width, velocity_in_out);
}

int mr_debug_motion_faces_post(mr_scene *sc, const double *verts_now, const double *verts_prev, int32_t n_verts, const int32_t *faces,
                               int32_t n_faces, const int32_t *face_off, const int32_t *deforming, int32_t n_models, const double *s_now,
                               const double *s_prev, const int32_t *winner, int32_t height, int32_t width, float *velocity_in_out,
                               double *out_h, int32_t *out_guard)
{
    return debug_motion_faces_post(sc, verts_now, verts_prev, n_verts, faces, n_faces, face_off, deforming, n_models, s_now, s_prev, winner,
                                   height, width, velocity_in_out, out_h, out_guard);
}

int mr_debug_read_prev_vertices(mr_scene *sc, double *out)
{
    if (!sc || !out) return fail(MR_E_INVALID, "NULL argument");
    if (!sc->snap_valid) return fail(MR_E_INVALID, "no snapshot of the vertices yet (mr_scene_track_vertices, then a pose pass)");
    return read_back(sc->d_verts_prev, out, (size_t)sc->snap_verts * 4, "previous vertices");
}

int mr_debug_motion_faces(mr_scene *sc, int32_t *out)
{
    if (!sc || !out) return fail(MR_E_INVALID, "NULL argument");
    out[0] = sc->mfaces.ran; out[1] = sc->mfaces.skipped; out[2] = sc->mfaces.records; out[3] = sc->mfaces.snapshots;
    return MR_OK;
}

int mr_debug_motion_faces_times(mr_scene *sc, float *out_ms)
{
    return pass_times(sc, &mr_scene::mfaces, "no frame with the per-face velocity yet", out_ms, { { 0, 1 }, { 1, 2 } });
}

int64_t mr_overlay_state_bytes(mr_scene *sc)
{
    if (!sc) return fail(MR_E_INVALID, "scene is NULL");
    realize_overlay(sc);
    if (sc->ov_points == 0) return 0;
    ensure_overlay_slots(sc);
    return (int64_t)sc->ov_touched.size() * mr::OVERLAY_STATE_BYTES;
}

int mr_overlay_apply(mr_scene *sc, const void *d_parts, int64_t part_stride, int64_t state_offset, int32_t world, int32_t striped,
                     int32_t system, void *d_frame, void *stream_)
{
    using namespace mr;
    if (!sc || !d_parts || !d_frame) return fail(MR_E_INVALID, "NULL argument");
    if (world < 1 || part_stride <= 0 || state_offset < 0 || (system != 1 && system != -1)) return fail(MR_E_INVALID, "mr_overlay_apply: bad argument");
    realize_overlay(sc);
    if (sc->ov_points == 0) return MR_OK;
    if (!striped && sc->ov_height % world) return fail(MR_E_INVALID, "mr_overlay_apply: the bands of the split must be equal");
    int rc = ensure_init();
    if (rc) return rc;
    hipStream_t stream = stream_ ? (hipStream_t)stream_ : g_stream;
    FrameSlot *fs = slot_for(sc, stream);
    if (!fs) return fail(MR_E_DEVICE, "out of frame slots");
    if ((rc = sync_slot_overlay(sc, fs->ov, stream, true))) return rc;
    const int n_slots = (int)sc->ov_touched.size();
    // The compact state and the bidding words, per slot of the list of touched pixels, in a buffer of the slot's overlay
    // copy that nothing else writes: z | colour | win | any | keep, at offsets that depend on n_slots.  The kernel leaves
    // win / any zero, so they stay zero from call to call while the layout stays; with other lists (another number of
    // slots, or another serial) the words may lie where the last call kept colours or z, and the buffer is cleared.
    OverlayCopy &ov = fs->ov;
    const bool stale = ov.apply_slots != (size_t)n_slots || ov.apply_serial != sc->ov_serial;
    if ((rc = ensure_cleared(ov.apply_scratch, (size_t)n_slots * (8 + 12 + 4 + 4) + (size_t)sc->ov_points + 64, stream, 0, stale))) return rc;
    ov.apply_slots = (size_t)n_slots; ov.apply_serial = sc->ov_serial;
    char *scratch = static_cast<char *>(ov.apply_scratch.p);
    OverlayArgs oa = overlay_args(sc, fs->ov, true, reinterpret_cast<uint32_t *>(scratch + (size_t)n_slots * 20), (size_t)n_slots);
    oa.st_z = reinterpret_cast<double *>(scratch);
    oa.st_f = reinterpret_cast<float *>(scratch + (size_t)n_slots * 8);
    oa.out = static_cast<uint8_t *>(d_frame); oa.out_width = sc->ov_width; oa.out_height = sc->ov_height;
    hipLaunchKernelGGL(k_overlay_import, dim3(blocks_for(n_slots, 256)), dim3(256), 0, stream, oa.pixel_of, n_slots,
                       static_cast<const char *>(d_parts), (size_t)part_stride, (size_t)state_offset, sc->ov_width, sc->ov_height,
                       world, striped ? 1 : 0, oa.st_z, oa.st_f);
    hipLaunchKernelGGL(k_overlay, dim3(1), dim3(OVERLAY_BLOCK), 0, stream, oa, (double)system);
    HIP_TRY(hipGetLastError());
    return MR_OK;
}

void *mr_host_alloc(uint64_t bytes)
{
    if (ensure_init() != MR_OK) return nullptr;
    void *p = nullptr;
    if (hipHostMalloc(&p, (size_t)std::max<uint64_t>(bytes, 1), hipHostMallocDefault) != hipSuccess) {
        fail(MR_E_DEVICE, "hipHostMalloc failed");
        return nullptr;
    }
    return p;
}

// out[i][j] = a[i][0] * b[0][j], then fma(a[i][k], b[k][j], .) for k = 1 .. K-1: the order NumPy's BLAS uses for
// the reference's tiny host-side products, spelled out so that it is the same on any host.
// Host arithmetic for the Python mirror's per-frame constants; no device involved.
// Row r of a vertex's blend matrix: every entry rn(w0 * B[j0][r][c]) followed by fma steps over slots 1..3
static void host_skin_row(const double *bones, const int32_t *j, const double *w, int r, double s[4])
{
    for (int c = 0; c < 4; ++c) {
        double acc = w[0] * bones[(size_t)j[0] * 16 + r * 4 + c];
        for (int k = 1; k < 4; ++k) acc = std::fma(w[k], bones[(size_t)j[k] * 16 + r * 4 + c], acc);
        s[c] = acc;
    }
}

void mr_host_skin_chain(const double *verts, const int32_t *joints, const double *weights, const double *bones, int32_t n, double *out)
{
    for (int32_t i = 0; i < n; ++i) {
        const double *v = verts + (size_t)i * 4;
        double s[4], o[4];
        for (int r = 0; r < 4; ++r) {
            host_skin_row(bones, joints + (size_t)i * 4, weights + (size_t)i * 4, r, s);
            for (int c = 0; c < 4; ++c) o[c] = r == 0 ? v[0] * s[c] : std::fma(v[r], s[c], o[c]);
        }
        for (int c = 0; c < 4; ++c) out[(size_t)i * 4 + c] = o[c];
    }
}

void mr_host_skin_chain3(const double *vectors, const int32_t *owner, const int32_t *joints, const double *weights, const double *bones,
                         int32_t n, double *out)
{
    for (int32_t i = 0; i < n; ++i) {
        const double *v = vectors + (size_t)i * 3;
        double s[4], o[3] = { v[0], v[1], v[2] };
        if (owner[i] >= 0)
            for (int r = 0; r < 3; ++r) {
                host_skin_row(bones, joints + (size_t)owner[i] * 4, weights + (size_t)owner[i] * 4, r, s);
                for (int c = 0; c < 3; ++c) o[c] = r == 0 ? v[0] * s[c] : std::fma(v[r], s[c], o[c]);
            }
        for (int c = 0; c < 3; ++c) out[(size_t)i * 3 + c] = o[c];
    }
}

int mr_host_auto_normals(const double *verts, int32_t n_verts, const int32_t *faces12, int32_t n_faces, const float *normals_in,
                         int32_t n_normals, float *out)
{
    if (!verts || !normals_in || !out) return fail(MR_E_INVALID, "mr_host_auto_normals: NULL argument");
    if (const char *wrong = mr_autonormals::check_faces(faces12, n_faces, n_verts, n_normals)) return fail(MR_E_INVALID, wrong);
    mr_autonormals::Lists lists;                     // the lists the upload path builds, walked in the kernel's order
    if (!mr_autonormals::build_lists(n_normals, 0, faces12, 0, n_faces, lists))
        return fail(MR_E_INVALID, "the padded face lists do not fit 32-bit offsets");
    mr_autonormals::walk_lists(lists, verts, faces12, normals_in, out);
    return MR_OK;
}

int mr_host_morph_chain(const double *base, int32_t n, int32_t width, int32_t n_targets, const int32_t *first, const int32_t *index,
                        const double *delta, const double *w, double *out)
{
    if (!base || !w || !out || (width != 3 && width != 4)) return fail(MR_E_INVALID, "mr_host_morph_chain: bad argument");
    if (const char *wrong = mr_morph::check_tables(n, n_targets, first, index, delta)) return fail(MR_E_INVALID, wrong);
    mr_morph::Lists lists;                           // the lists the upload path builds, walked in the kernel's order
    if (!mr_morph::build_lists(n, n_targets, first, index, delta, lists))
        return fail(MR_E_INVALID, "the morph's padded lists do not fit 32-bit offsets");
    mr_morph::walk_lists(lists, base, width, w, out);
    return MR_OK;
}

void mr_host_matmul_chain(const double *a, const double *b, double *out, int32_t m, int32_t k, int32_t p)
{
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < p; ++j) {
            double acc = a[(size_t)i * k] * b[j];
            for (int x = 1; x < k; ++x) acc = std::fma(a[(size_t)i * k + x], b[(size_t)x * p + j], acc);
            out[(size_t)i * p + j] = acc;
        }
}

// Host arithmetic: everything Scene.render() derives from a camera that moved, in one call (obj/core.py:383-405,
// obj/transformation.py:57-110, obj/plane_intersection.py:43-56, as the Python mirror spells them: _look_at_axes with
// scalar arithmetic, products as ascending fma chains): look-at = translate @ rotate, MVP = look-at @ projection, and
// the six normalised frustum planes of the MVP.  `eye`, `center`, `up` are the ARGUMENTS of look_at_rotate_* (the
// reference passes the camera's centre as eye and its position as centre), `position` the camera's position (the
// translation), `lh` the handedness of the rotation.  Bit-identical to the NumPy path (tests/test_host_api.py).
void mr_host_camera_constants(const double *eye, const double *center, const double *up, const double *position,
                              const double *projection, int32_t lh, double *lookat, double *mvp, double *planes)
{
    auto unit3 = [](const double v[3], double o[3]) {
        double l = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
        if (l == 0) l = 1.0;
        for (int j = 0; j < 3; ++j) o[j] = v[j] / l;
    };
    auto cross3 = [](const double a[3], const double b[3], double o[3]) {
        o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
    };
    const double d[3] = { center[0] - eye[0], center[1] - eye[1], center[2] - eye[2] };
    double forward[3], right[3], c[3], new_up[3];
    unit3(d, forward);
    cross3(up, forward, c);
    unit3(c, right);
    cross3(forward, right, new_up);
    double rot[16] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1 }, tr[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
    for (int r = 0; r < 3; ++r) { rot[r * 4 + 0] = right[r]; rot[r * 4 + 1] = new_up[r]; rot[r * 4 + 2] = lh ? -forward[r] : forward[r]; }
    for (int j = 0; j < 3; ++j) tr[12 + j] = -position[j];
    mr_host_matmul_chain(tr, rot, lookat, 4, 4, 4);
    mr_host_matmul_chain(lookat, projection, mvp, 4, 4, 4);
    for (int axis = 0; axis < 3; ++axis)
        for (int sgn = 0; sgn < 2; ++sgn) {
            double pl[4];
            for (int r = 0; r < 4; ++r) pl[r] = sgn ? mvp[r * 4 + 3] - mvp[r * 4 + axis] : mvp[r * 4 + 3] + mvp[r * 4 + axis];
            double acc = pl[0] * pl[0];
            for (int r = 1; r < 4; ++r) acc = std::fma(pl[r], pl[r], acc);
            const double n = std::sqrt(acc);
            for (int r = 0; r < 4; ++r) planes[(2 * axis + sgn) * 4 + r] = pl[r] / n;
        }
}

// The debug-frustum overlay's statement lists on the host (host_overlay.h): build into a per-thread buffer, report
// the sizes, then copy out into arrays of those sizes.
int mr_host_overlay_build(const double *corners, const double *planes, const double *mvp, const double *viewport,
                          double near_, double far_, int32_t camera_inside, int32_t height, int32_t width,
                          int32_t *n_segments, int32_t *n_points, int32_t *n_touched)
{
    if (!corners || !planes || !mvp || !viewport || !n_segments || !n_points || !n_touched || height <= 0 || width <= 0)
        return fail(MR_E_INVALID, "mr_host_overlay_build: bad argument");
    g_overlay_lists = mr_host::OverlayLists();
    mr_host::build_overlay_lists(corners, FRUSTUM_FACES, planes, mvp, viewport, near_, far_, camera_inside != 0, height, width, 13,
                                 g_overlay_lists);
    *n_segments = (int32_t)g_overlay_lists.seg_first.size();
    *n_points = (int32_t)g_overlay_lists.z.size();
    *n_touched = (int32_t)g_overlay_lists.touched.size();
    return MR_OK;
}

int mr_host_overlay_fetch(int32_t *seg_first, int32_t *seg_count, int32_t *target, int32_t *next, double *z, int32_t *touched)
{
    const mr_host::OverlayLists &o = g_overlay_lists;
    const size_t n = o.z.size();
    if (seg_first) std::copy(o.seg_first.begin(), o.seg_first.end(), seg_first);
    if (seg_count) std::copy(o.seg_count.begin(), o.seg_count.end(), seg_count);
    for (int k = 0; k < 5; ++k) {
        if (target) std::copy(o.target[k].begin(), o.target[k].end(), target + (size_t)k * n);
        if (next) std::copy(o.next[k].begin(), o.next[k].end(), next + (size_t)k * n);
    }
    if (z) std::copy(o.z.begin(), o.z.end(), z);
    if (touched) std::copy(o.touched.begin(), o.touched.end(), touched);
    return MR_OK;
}

void mr_host_free(void *p)
{
    if (p) (void)hipHostFree(p);
}

int mr_render_device(mr_scene *sc, const mr_frame_desc *fr, void *d_out_rgb, void *stream)
{
    if (!sc || !d_out_rgb) return fail(MR_E_INVALID, "NULL argument");
    int rc = validate_frame(sc, fr);
    if (rc) return rc;
    if ((rc = ensure_init())) return rc;
    FrameSlot *fs = slot_for(sc, stream ? (hipStream_t)stream : g_stream);
    if (!fs) return fail(MR_E_INVALID, "a scene can be rendered from at most 32 different streams");
    if (sc->taa.on)
        return fail(MR_E_INVALID, "temporal anti-aliasing: its frames are rendered by mr_render or mr_render_async, whose return hands the history over");
    if (sc->tone.on && sc->tone.params.adaptive())
        return fail(MR_E_INVALID, "adaptive tone mapping: its frames are rendered by mr_render or mr_render_async, whose return hands the exposure over");
    if (sc->layers.on)
        return fail(MR_E_INVALID, "data layers: its frames are rendered by mr_render or mr_render_async, whose return says which frame mr_read_layers reads");
    return enqueue_frame(sc, fs, fr, static_cast<uint8_t *>(d_out_rgb));
}

int mr_get_stats(mr_scene *sc, mr_stats *stats)
{
    if (!sc || !stats) return fail(MR_E_INVALID, "NULL argument");
    FrameSlot *fs = last_slot(sc);
    if (!fs) return MR_E_INVALID;
    HIP_TRY(hipDeviceSynchronize());
    // a frame on any stream may have overflowed its lists: grow them all before reporting
    bool overflowed = false;
    for (auto &s : sc->slots) {
        if (!s->have_frame) continue;
        if (int rc = fetch_counters(s.get(), true)) return rc;
        HIP_TRY(hipStreamSynchronize(s->stream));
        if (collect(sc, s.get(), s->last_copied) == MR_E_OVERFLOW) { overflowed = true; frame_settled(sc, s.get(), false); }
    }
    (void)collect(sc, fs, fs->last_copied);     // report the most recent frame
    *stats = sc->stats;
    if (overflowed)
        return fail(MR_E_OVERFLOW, "a frame overflowed a work list (now grown): render it again");
    return MR_OK;
}

namespace {
// adds the marked frames of one slot (most recent first, at most `limit`) to acc; returns how many
uint64_t add_slot_times(const FrameSlot &s, uint64_t limit, double acc[MR_N_KERNEL_TIMES])
{
    const uint64_t have = std::min<uint64_t>(s.frames_enqueued, EVENT_RING);
    uint64_t taken = 0;
    for (uint64_t i = 0; i < have && taken < limit; ++i) {
        const uint64_t slot = (s.frames_enqueued - 1 - i) % EVENT_RING;
        const int marks = s.ev_marks[slot];
        if (!marks) continue;
        const hipEvent_t *ev = s.ev_ring[slot];
        auto span = [&](int a, int b) { float ms = 0; (void)hipEventElapsedTime(&ms, ev[a], ev[b]); return (double)ms; };
        if (marks == 1) {
            acc[2] += span(0, 3);
        } else {
            acc[0] += span(0, 1); acc[1] += span(1, 2); acc[2] += span(2, 3);
        }
        acc[3] += span(3, 4);
        acc[4] += span(0, 4);
        ++taken;
    }
    return taken;
}

int mean_times(const double acc[MR_N_KERNEL_TIMES], uint64_t used, float *out_ms)
{
    for (int k = 0; k < MR_N_KERNEL_TIMES; ++k) out_ms[k] = used ? (float)(acc[k] / (double)used) : 0.f;
    return (int)used;
}
}  // namespace

int mr_get_kernel_times(mr_scene *sc, int n_frames, float *out_ms, int cap)
{
    if (!sc || !out_ms || cap < MR_N_KERNEL_TIMES) return fail(MR_E_INVALID, "need room for MR_N_KERNEL_TIMES floats");
    if (!last_slot(sc)) return MR_E_INVALID;
    HIP_TRY(hipDeviceSynchronize());
    double acc[MR_N_KERNEL_TIMES] = {};
    uint64_t used = 0;
    // only the slots that render the same kind of frame as the most recent one (same flags apart from
    // the timing bits, same rows) are averaged: a whole-frame mr_render on the library's stream must
    // not be mixed into the statistics of band frames enqueued on the caller's streams
    const mr_frame_desc &ref = sc->last->last_frame;
    constexpr int timing_bits = MR_FRAME_NO_TIMING | MR_FRAME_LIGHT_TIMING;
    auto same_kind = [&](const FrameSlot &s) {
        return s.have_frame && (s.last_frame.flags & ~timing_bits) == (ref.flags & ~timing_bits) &&
               s.last_frame.row_begin == ref.row_begin && s.last_frame.row_end == ref.row_end &&
               s.last_frame.stripe_count == ref.stripe_count && s.last_frame.stripe_index == ref.stripe_index;
    };
    int active = 0;
    for (auto &s : sc->slots) active += same_kind(*s) ? 1 : 0;
    const uint64_t per_slot = std::max<uint64_t>(1, ((uint64_t)std::max(n_frames, 1) + active - 1) / std::max(active, 1));
    for (auto &s : sc->slots)
        if (same_kind(*s)) used += add_slot_times(*s, per_slot, acc);
    return mean_times(acc, used, out_ms);
}

int mr_get_stream_kernel_times(mr_scene *sc, void *stream, int n_frames, float *out_ms, int cap)
{
    if (!sc || !out_ms || cap < MR_N_KERNEL_TIMES) return fail(MR_E_INVALID, "need room for MR_N_KERNEL_TIMES floats");
    const hipStream_t want = stream ? (hipStream_t)stream : g_stream;
    HIP_TRY(hipDeviceSynchronize());
    double acc[MR_N_KERNEL_TIMES] = {};
    uint64_t used = 0;
    for (auto &s : sc->slots)
        if (s->stream == want && s->have_frame) used += add_slot_times(*s, (uint64_t)std::max(n_frames, 1), acc);
    return mean_times(acc, used, out_ms);
}

int mr_read_z(mr_scene *sc, double *out) { return read_tap(sc, MR_FRAME_KEEP_BUFFERS, "MR_FRAME_KEEP_BUFFERS", &FrameSlot::d_z, out, 1, "z"); }

int mr_read_stencil(mr_scene *sc, int16_t *out) { return mr_read_stencil_light(sc, 0, out); }

int mr_read_stencil_light(mr_scene *sc, int32_t light, int16_t *out)
{
    FrameSlot *fs = last_slot_with(sc, MR_FRAME_KEEP_BUFFERS, "MR_FRAME_KEEP_BUFFERS");
    if (!fs) return MR_E_INVALID;
    if (light < 0 || light >= fs->last_n_lights) return fail(MR_E_INVALID, "the last frame had no such light");
    const size_t n = (size_t)fs->last_frame.width * fs->last_frame.height;
    std::vector<int32_t> wide(n);           // the device accumulates in 32 bits; the reference's buffer is int16
    if (int rc = read_back(light ? fs->d_stencil_x[light - 1] : fs->d_stencil, wide.data(), n, "stencil")) return rc;
    if (!out) return fail(MR_E_INVALID, "NULL argument");
    for (size_t i = 0; i < n; ++i) out[i] = (int16_t)wide[i];
    return MR_OK;
}

int mr_read_winner(mr_scene *sc, int32_t *out) { return read_tap(sc, MR_FRAME_KEEP_BUFFERS, "MR_FRAME_KEEP_BUFFERS", &FrameSlot::d_winner, out, 1, "winner"); }

int mr_read_frame_f32(mr_scene *sc, float *out) { return read_tap(sc, MR_FRAME_KEEP_FLOAT, "MR_FRAME_KEEP_FLOAT", &FrameSlot::d_frame, out, 3, "frame"); }

int mr_read_face_status(mr_scene *sc, uint8_t *out)
{
    FrameSlot *fs = last_slot_with(sc, MR_FRAME_FACE_STATUS, "MR_FRAME_FACE_STATUS");
    if (!fs) return MR_E_INVALID;
    if (is_partial(&fs->last_frame))
        return fail(MR_E_INVALID, "per-face status needs the whole frame on one device (no row band, no stripes)");
    return read_back(fs->d_status, out, sc->faces.size() / 12, "face status");
}

int mr_debug_read_tile_records(mr_scene *sc, uint32_t *out, int32_t cap_tiles)
{
    FrameSlot *fs = last_slot(sc);
    if (!fs) return MR_E_INVALID;
    if (!out) return fail(MR_E_INVALID, "NULL argument");
    const int n = std::min(fs->last_n_tiles, cap_tiles);
    HIP_TRY(hipDeviceSynchronize());
    static_assert(mr::TILE_REC == MR_TILE_RECORD_WORDS, "tile record size is part of the ABI");
    if (n > 0) HIP_TRY(hipMemcpy(out, fs->d_tile_stats.p, (size_t)n * mr::TILE_REC * 4, hipMemcpyDeviceToHost));
    if (!fs->last_full)                              // the frame-only tile kernel does not write the counts: they read 0
        for (int t = 0; t < n; ++t)
            for (int k = 0; k < mr::TILE_STATS; ++k) out[(size_t)t * mr::TILE_REC + k] = 0u;
    return fs->last_n_tiles;
}

int mr_debug_clusters_culled(mr_scene *sc)
{
    FrameSlot *fs = last_slot(sc);
    if (!fs) return MR_E_INVALID;
    HIP_TRY(hipDeviceSynchronize());
    if (int rc = fetch_counters(fs, false)) return rc;
    HIP_TRY(hipStreamSynchronize(fs->stream));
    return (int)fs->h_counters->pad0[0];
}

int mr_debug_quad_walks(mr_scene *sc, uint32_t *out)
{
    FrameSlot *fs = last_slot(sc);
    if (!fs) return MR_E_INVALID;
    if (!out) return fail(MR_E_INVALID, "NULL argument");
    HIP_TRY(hipDeviceSynchronize());
    if (int rc = fetch_counters(fs, false)) return rc;
    HIP_TRY(hipStreamSynchronize(fs->stream));
    for (int k = 0; k < 4; ++k) out[k] = fs->h_counters->pad0[1 + k];
    return MR_OK;
}

int mr_debug_pair_log(mr_scene *sc, uint32_t *out)
{
    FrameSlot *fs = last_slot(sc);
    if (!fs) return MR_E_INVALID;
    if (!out) return fail(MR_E_INVALID, "NULL argument");
    HIP_TRY(hipDeviceSynchronize());
    if (int rc = fetch_counters(fs, false)) return rc;
    HIP_TRY(hipStreamSynchronize(fs->stream));
    for (int k = 0; k < 2; ++k) out[k] = fs->h_counters->pad0[5 + k];
    return MR_OK;
}

int mr_debug_big_tri_rejects(mr_scene *sc)
{
    FrameSlot *fs = last_slot(sc);
    if (!fs) return MR_E_INVALID;
    HIP_TRY(hipDeviceSynchronize());
    if (int rc = fetch_counters(fs, false)) return rc;
    HIP_TRY(hipStreamSynchronize(fs->stream));
    return (int)fs->h_counters->pad0[7];
}

int mr_debug_force_full(mr_scene *sc, int32_t on)
{
    if (!sc) return fail(MR_E_INVALID, "NULL argument");
    sc->force_full = on != 0;
    return MR_OK;
}

int mr_debug_frame_path(mr_scene *sc, int32_t *out)
{
    FrameSlot *fs = last_slot(sc);
    if (!fs) return MR_E_INVALID;
    if (!out) return fail(MR_E_INVALID, "NULL argument");
    out[0] = fs->last_full ? 1 : 0; out[1] = fs->last_split ? 1 : 0; out[2] = fs->last_ss_mode ? 1 : 0;
    out[3] = fs->last_n_lights > 1 ? 1 : 0; out[4] = fs->last_ordered ? 1 : 0;
    return MR_OK;
}

int mr_debug_sil_cache(mr_scene *sc, int32_t *out)
{
    if (!sc || !out) return fail(MR_E_INVALID, "NULL argument");
    out[0] = sc->sil.last_path; out[1] = (int32_t)sc->sil.last_entries; out[2] = (int32_t)sc->sil.captures;
    out[3] = sc->sil.valid_buffers();
    return MR_OK;
}

int mr_debug_pose(mr_scene *sc, int32_t *out)
{
    if (!sc || !out) return fail(MR_E_INVALID, "NULL argument");
    int32_t posed = 0;
    for (const mr_scene::ModelPose &mp : sc->poses) posed += mp.posed ? 1 : 0;
    out[0] = sc->commits; out[1] = sc->pose_passes; out[2] = posed; out[3] = sc->pose_written;
    return MR_OK;
}

int mr_debug_pose_times(mr_scene *sc, float *out_ms)
{
    if (!sc || !out_ms) return fail(MR_E_INVALID, "NULL argument");
    return sc->marks_pose.read(out_ms, "no pose pass over faces yet");
}

int mr_debug_pose_normals_times(mr_scene *sc, float *out_ms)
{
    if (!sc || !out_ms) return fail(MR_E_INVALID, "NULL argument");
    return sc->marks_normals.read(out_ms, "no pose pass over normals yet");
}

int mr_debug_skin(mr_scene *sc, int32_t *out)
{
    if (!sc || !out) return fail(MR_E_INVALID, "NULL argument");
    int32_t skinned = 0;
    for (const mr_scene::ModelPose &mp : sc->poses) skinned += mp.has_bones ? 1 : 0;
    out[0] = skinned; out[1] = sc->skin_bones; out[2] = sc->skin_written; out[3] = sc->skin_normals_written;
    return MR_OK;
}

int mr_debug_skin_times(mr_scene *sc, float *out_ms)
{
    if (!sc || !out_ms) return fail(MR_E_INVALID, "NULL argument");
    return sc->marks_skin.read(out_ms, "no pass over a skin yet");
}

int mr_debug_morph(mr_scene *sc, int32_t *out)
{
    if (!sc || !out) return fail(MR_E_INVALID, "NULL argument");
    int32_t weighted = 0;
    for (const mr_scene::ModelPose &mp : sc->poses) weighted += mp.has_weights ? 1 : 0;
    out[0] = weighted; out[1] = sc->morph_targets; out[2] = sc->morph_written; out[3] = sc->morph_normals_written;
    out[4] = sc->morph_entries;
    return MR_OK;
}

int mr_debug_auto_normals(mr_scene *sc, int32_t *out)
{
    if (!sc || !out) return fail(MR_E_INVALID, "NULL argument");
    int64_t kept = 0;
    if (sc->auto_kept_waves > 0) {                   // (the pass has waited for its kernels)
        std::vector<int32_t> waves((size_t)sc->auto_kept_waves);
        HIP_TRY(hipMemcpy(waves.data(), sc->d_auto_kept.p, waves.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (int32_t k : waves) kept += k;
    }
    out[0] = sc->auto_models; out[1] = sc->auto_written; out[2] = sc->auto_entries; out[3] = (int32_t)kept;
    return MR_OK;
}

int mr_debug_auto_normals_times(mr_scene *sc, float *out_ms)
{
    if (!sc || !out_ms) return fail(MR_E_INVALID, "NULL argument");
    return sc->marks_auto.read(out_ms, "no pass over rebuilt normals yet");
}

int mr_debug_morph_times(mr_scene *sc, float *out_ms)
{
    if (!sc || !out_ms) return fail(MR_E_INVALID, "NULL argument");
    return sc->marks_morph.read(out_ms, "no pass over a morph yet");
}

int mr_debug_read_clusters(mr_scene *sc, void *out, int32_t cap_clusters)
{
    if (!sc || !out) return fail(MR_E_INVALID, "NULL argument");
    if (sc->dirty || !sc->d_clusters.p) return fail(MR_E_INVALID, "clusters: nothing rendered since the scene changed");
    static_assert(sizeof(mr::ClusterRec) == 64, "the cluster record's layout is documented in the header");
    const int n = std::min(sc->n_clusters, cap_clusters);
    HIP_TRY(hipDeviceSynchronize());
    if (n > 0) HIP_TRY(hipMemcpy(out, sc->d_clusters.p, (size_t)n * sizeof(mr::ClusterRec), hipMemcpyDeviceToHost));
    return sc->n_clusters;
}

int mr_debug_read_tile_order(mr_scene *sc, uint32_t *out, int32_t cap_tiles)
{
    FrameSlot *fs = last_slot(sc);
    if (!fs) return MR_E_INVALID;
    if (!out) return fail(MR_E_INVALID, "NULL argument");
    const int n = std::min(fs->last_n_tiles, cap_tiles);
    HIP_TRY(hipDeviceSynchronize());
    if (n > 0 && fs->last_ordered)
        HIP_TRY(hipMemcpy(out, fs->d_hist.as<uint32_t>() + mr::ORDER_HEAD, (size_t)n * 4, hipMemcpyDeviceToHost));
    else
        for (int i = 0; i < n; ++i) out[i] = (uint32_t)i;     // frames rendered from several streams keep row-major order
    return fs->last_n_tiles;
}

int mr_read_silhouette_light(mr_scene *sc, int32_t light, int32_t *out, int32_t cap)
{
    FrameSlot *fs = last_slot(sc);
    if (!fs) return MR_E_INVALID;
    if (light < 0 || light >= fs->last_n_lights) return fail(MR_E_INVALID, "the last frame had no such light");
    if (fs->last_n_lights == 1) return mr_read_silhouette(sc, out, cap);
    // the lights' entries share the one list, each tagged with its light: this one's among all that are listed
    return decode_silhouette(sc, fs, light, std::min(sc->n_silhouette, (int)fs->quad_cap), out, cap);
}

int mr_read_silhouette(mr_scene *sc, int32_t *out, int32_t cap)
{
    FrameSlot *fs = last_slot(sc);
    if (!fs) return MR_E_INVALID;
    if (fs->last_n_lights > 1) return mr_read_silhouette_light(sc, 0, out, cap);
    // the frame's count, also when the list overflowed or the caller's array is shorter
    const int n = sc->n_silhouette;
    const int take = std::min(std::min(n, cap), (int)fs->quad_cap);
    if (take > 0 && out) {
        if (int rc = decode_silhouette(sc, fs, 0, take, out, cap); rc < 0) return rc;
    }
    return n;
}

}  // extern "C"
