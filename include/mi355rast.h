/*
 * mi355rast.h -- C ABI of libmi355rast.so, the MI355X (gfx950) rasteriser behind
 * py_numpy_renderer_amd.Scene.render().
 *
 * The reference (Denizantip/py-numpy-renderer) has no FFI: its boundary for this path is
 * the Python call Scene.render() -> uint8 (H, W, 3) (obj/core.py:587-640).  Each entry
 * point below names the reference code it stands in for; a host in any language binds
 * these symbols (INTEGRATION.md shows the ctypes stub).
 *
 * Conventions: plain pointers and sizes only; every function returns MR_OK (0) or a
 * negative MR_E_* code and never throws; mr_last_error() describes the last failure on the
 * calling thread.  The caller owns every host pointer it passes (they may be freed as soon
 * as the call returns); the library owns all device memory.  A scene is used from one
 * thread at a time.  Matrices are row-major float64 in the reference's row-vector
 * convention (clip = v @ MVP).
 */
#ifndef MI355RAST_H
#define MI355RAST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MR_ABI_VERSION 4

enum {
    MR_OK = 0,
    MR_E_INVALID = -1,      /* bad argument / inconsistent sizes */
    MR_E_DEVICE = -2,       /* HIP runtime error (no GPU, out of memory, launch failure) */
    MR_E_UNSUPPORTED = -3,  /* feature of the reference that this build does not implement */
    MR_E_OVERFLOW = -4      /* internal work list could not be grown */
};

/* light kinds: obj/lightning.py:4-7 */
enum { MR_LIGHT_DIRECTIONAL = 0, MR_LIGHT_POINT = 1, MR_LIGHT_SPOT = 2 };

/* per-face result of the lit pass, numerically the reference's Errors flag (obj/triangular.py:15-20) */
enum {
    MR_FACE_RENDERED = 0, MR_FACE_BACK_FACE_CULLING = 1, MR_FACE_WRONG_MIN_MAX = 2,
    MR_FACE_EMPTY_B = 4, MR_FACE_EMPTY_Z = 8, MR_FACE_CLIPPED = 16
};

/* mr_frame_desc.flags */
enum {
    MR_FRAME_SHADOWS = 1,     /* run the shadow-volume stencil pass (obj/core.py:610-622) */
    MR_FRAME_KEEP_FLOAT = 2,  /* also keep the float32 frame (needed by mr_read_frame_f32) */
    MR_FRAME_FACE_STATUS = 4, /* also compute the per-face status histogram (obj/core.py:625-636) */
    MR_FRAME_LIGHT_TIMING = 8, /* record only the event marks around the frame and the tile kernel */
    MR_FRAME_SKYBOX = 16,     /* fill the background from the cubemap of mr_scene_set_skybox (obj/core.py:595-596) */
    MR_FRAME_COUNTERS = 32,   /* keep the reference-equivalent fragment counters of mr_stats, and the reference's
                                 stencil values at pixels no triangle covers (mr_read_stencil).  Without it only
                                 the frame is the contract and the library skips work that cannot change it
                                 (shadow quads that cannot pass the depth test anywhere in a strip of pixels);
                                 mr_render sets it by itself when it is handed a stats pointer. */
    MR_FRAME_NO_TIMING = 128, /* record no HIP events at all for this frame (each one costs a few microseconds between
                                 two kernels): mr_stats.gpu_ms_* read 0 and mr_get_kernel_times skips the frame */
    MR_FRAME_OVERLAY = 256,   /* replay the statement lists of mr_scene_set_overlay (the debug-camera frustum of
                                 obj/core.py:638) on the frame after the tile kernel; implies MR_FRAME_KEEP_BUFFERS
                                 and MR_FRAME_KEEP_FLOAT.  On part of a frame (row band / stripes;
                                 mr_render_device only) the overlay is not drawn: the state it needs is appended to the
                                 rows for mr_overlay_apply, see there */
    MR_FRAME_SUPERSAMPLE2 = 512,   /* ordered-grid supersampling, s = 2 or 4 samples per output pixel and axis (at most one of */
    MR_FRAME_SUPERSAMPLE4 = 1024,  /* the two).  width / height, viewport, sky_* and row_begin / row_end then describe the
                                 SAMPLE grid and must be multiples of s; stripe_count > 1 is refused.  Output pixel (x, y)
                                 is the mean of samples (s x + i, s y + j), 0 <= i, j < s (rows counted from the bottom),
                                 finalised once: the output buffer holds (row_end - row_begin) / s x width / s x 3 bytes.
                                 The taps (mr_read_z / _stencil / _winner / _frame_f32) and the counters stay on the sample
                                 grid.  With MR_FRAME_OVERLAY the lines are drawn on the sample grid too (whole frames only) */
    MR_FRAME_KEEP_BUFFERS = 64 /* also write the reference's working buffers (z_buffer, stencil_buffer, winner
                                 face per pixel; obj/core.py:588-591) to device memory for mr_read_z /
                                 mr_read_stencil / mr_read_winner.  Without it they only ever exist on chip,
                                 tile by tile.  MR_FRAME_FACE_STATUS implies it. */
};

typedef struct mr_scene mr_scene;

/* Per-frame constants: what Scene.render() derives from camera / debug_camera / light /
 * resolution before its loops (obj/core.py:588-600, 394-429; obj/transformation.py:123-136;
 * obj/plane_intersection.py:43-56).  The host computes them in float64. */
typedef struct mr_frame_desc {
    int32_t width, height;          /* Scene.resolution = (height, width) */
    int32_t system;                 /* SYSTEM.RH = +1, SYSTEM.LH = -1 (obj/constants.py:29-31) */
    int32_t backface_culling;       /* Camera.backface_culling */
    int32_t light_type;             /* MR_LIGHT_* */
    int32_t flags;                  /* MR_FRAME_* */
    int32_t row_begin, row_end;     /* output rows [row_begin, row_end) this device renders;
                                       0, height for the whole frame (screen-tile split, contiguous bands) */
    int32_t stripe_count, stripe_index;  /* screen-tile split, interleaved: with stripe_count = N > 1 this device
                                       renders the tile rows (16 screen rows each, counted from the BOTTOM of the
                                       frame like the reference's buffers) t with t mod N == stripe_index;
                                       row_begin / row_end must then be 0 / height.  The output buffer holds
                                       ceil(ceil(height / 16) / N) blocks of 16 x width x 3 bytes, this device's
                                       highest tile row first, rows inside a block top-down (multigpu.py
                                       un-permutes after the all-gather).  0 or 1 = off */
    double mvp[16];                 /* camera.MVP */
    double viewport[16];            /* camera.viewport */
    double debug_mvp[16];           /* debug_camera.MVP (obj/triangular.py:39) */
    double frustum_planes[24];      /* camera.frustum_planes: left,right,bottom,top,near,far */
    double z_near, z_far;           /* camera.near / camera.far */
    double camera_pos[3];
    double light_pos[3], light_dir[3], light_color[3], light_ambient[3];
    double specular_strength;
    double att_constant, att_linear, att_quadratic;
    double spot_edge0, spot_edge1;  /* cos(20 deg), cos(10 deg) (obj/triangular.py:158-159) */
    float background[3];            /* obj/core.py:597-600 */
    uint32_t background_u8;         /* the same colour after obj/core.py:640's finalise, computed by the host:
                                       r | g << 8 | b << 16 | 1 << 24; 0 = let the device compute it */
    /* MR_FRAME_SKYBOX only (obj/cube_map.py:83-101): the two screen-filling triangles' vertices
     * truncated to int, [triangle][vertex][x, y], and their un-projected corner rays
     * face @ inv(view_without_translation @ projection) / w, [triangle][vertex][x, y, z] */
    int32_t sky_tri[12];
    double sky_rays[18];
} mr_frame_desc;

/* One material group of a model (obj/materials.py:47-55; obj/core.py:125). */
typedef struct mr_material {
    double kd[3];                   /* Material.Kd */
    double ks255[3];                /* Material.Ks * 255, evaluated by the host in Ks's dtype (obj/core.py:152) */
    double ns;                      /* Material.Ns */
    int32_t tex_kd, tex_norm, tex_ks;  /* ids from mr_scene_add_texture, or -1 */
    int32_t norm_tangent;           /* normal map is tangent-space (dtype.metadata['tangent']) */
} mr_material;

/* One Model (obj/core.py:231-251): arrays exactly as Model.load_model leaves them, with
 * indices already made non-negative. */
typedef struct mr_model_desc {
    const double *vertices;         /* (n_vertices, 4) Model.vertices widened to float64 */
    const float *uv;                /* (n_uv, 3) Model.uv, or NULL */
    const float *normals;           /* (n_normals, 3) Model.normals, or NULL */
    const int32_t *faces;           /* (n_faces, 3, 4) Model._faces: [vertex, uv, normal, material] per corner */
    const mr_material *materials;   /* (n_materials) indexed by the material column */
    const int32_t *edge_ids;        /* (n_faces, 3) the vertex column of Model._faces exactly as the loader left it
                                       (negative = relative index, obj/core.py:313), or NULL when it equals the
                                       vertex indices in `faces`.  The reference's silhouette set hashes these raw
                                       values (obj/triangular.py:286-302): an edge written once as (3, 2) and once
                                       as (-7, -8) does not cancel although both name the same two vertices */
    int32_t n_vertices, n_uv, n_normals, n_faces, n_materials;
    int32_t vertices_are_f32;       /* Model.vertices.dtype == float32: edge vectors and the silhouette
                                       normal are then formed in float32 like NumPy does */
    int32_t clip;                   /* Model.clip */
    int32_t depth_test;             /* Model.depth_test; 0: the model's fragments are tested against the z-buffer but
                                       never written to it (obj/triangular.py:117) */
} mr_model_desc;

/* Counters of the last mr_render call (BASELINE.md fragment definition). */
typedef struct mr_stats {
    int64_t frag_tri;               /* (triangle, pixel) pairs with u,v,w >= 0 (obj/triangular.py:78) */
    int64_t frag_quad;              /* (shadow quad, pixel) pairs inside the quad (obj/triangular.py:347) */
    int64_t covered_px;             /* pixels with a z-buffer winner */
    int64_t lit_px;                 /* covered pixels with stencil == 0 */
    int64_t stencil_updates;        /* quad fragments that passed the z test */
    int64_t n_faces, n_faces_setup; /* faces in the scene / faces that produced a pixel box */
    int64_t n_quads, n_quads_drawn; /* silhouette edges / quads that reached rasterisation */
    int64_t tri_bin_entries, quad_bin_entries;   /* (primitive, tile) pairs */
    float gpu_ms_total;             /* device time of the whole frame (HIP events) */
    float gpu_ms_setup;             /* k_setup: vertex transform, face set-up, silhouettes, shadow-quad set-up, own tile lists */
    float gpu_ms_binning;           /* k_bin_work: tile lists of the large primitives, leftover survivor counts */
    float gpu_ms_tile;              /* k_tile: coverage, z, stencil, shading, finalise */
    float gpu_ms_copy;              /* device -> host copy of the uint8 frame */
} mr_stats;

/* Selects the HIP device for the calling process (one process per GPU) and creates the
 * library's stream.  device < 0 keeps the current device. */
int mr_init(int device);

/* 1 when a HIP device is visible, else 0.  Never fails. */
int mr_device_available(void);

int mr_abi_version(void);

/* sizeof() of the ABI structs as this build sees them (0 mr_frame_desc, 1 mr_material,
 * 2 mr_model_desc, 3 mr_stats, 4 mr_overlay_desc, 5 mr_light_desc, 6 mr_ao_desc; -1 otherwise), so a binding can verify
 * its own layout. */
int mr_abi_struct_size(int which);

/* Scene() -- obj/core.py:563-582.  Returns NULL on failure. */
mr_scene *mr_scene_create(void);
void mr_scene_destroy(mr_scene *scene);

/* Model.textures.register / parse_mtl texture load (obj/core.py:90-105, 334-342): uploads a
 * float32 (h, w, 3) image exactly as the reference stores it.  Returns the texture id (>= 0)
 * or a negative error. */
int mr_scene_add_texture(mr_scene *scene, const float *rgb, int32_t h, int32_t w);

/* Scene(skymap=CubeMap(...)) -- obj/cube_map.py:22-34: the six cubemap faces as one uint8
 * (6, size, size, 3) stack in the reference's face order and orientation (CubeMap.textures * 255).
 * size = 0 removes the skybox.  Used by frames that set MR_FRAME_SKYBOX. */
int mr_scene_set_skybox(mr_scene *scene, const uint8_t *texels, int32_t size);

/* Scene.add_model (obj/core.py:584-585).  Returns the model index (>= 0) or a negative error. */
int mr_scene_add_model(mr_scene *scene, const mr_model_desc *model);

/* Drops all models and textures (keeps device allocations for reuse). */
int mr_scene_clear(mr_scene *scene);

/* More than one light (an addition: the reference's Scene has exactly one).  The frame descriptor's light stays light 0;
 * this sets lights 1 .. n of every frame enqueued afterwards (0 <= n <= MR_MAX_LIGHTS - 1; copied during the call;
 * n = 0: plain frames again).  With L_0 .. L_n the frame's lights, F_k the float frame the same scene gives with L_k as
 * its only light and W the winner map (which does not depend on the light), the frame is
 *     F[p] = min(F_0[p] + F_1[p] + ... + F_n[p], 1)   (float32 adds in this order)   where a face covers p,
 *     F[p] = F_0[p]                                    (background / skybox)           elsewhere,
 * then overlay and finalise (or resolve) as for any frame.  Every F_k keeps the reference's clip(0.05, 1), so a pixel
 * no light reaches shows 0.05 per light.  Visibility runs once; every light has its own silhouette, shadow quads and
 * stencil count (mr_read_stencil_light / mr_read_silhouette_light).  mr_stats: frag_tri, covered_px, n_faces*,
 * tri_bin_entries as for one light; frag_quad, stencil_updates, lit_px, n_quads, n_quads_drawn, quad_bin_entries are sums
 * over the lights.  Frames of a scene with extra lights refuse MR_FRAME_FACE_STATUS and stripe_count > 1 (MR_E_INVALID)
 * and neither read nor fill the silhouette cache. */
#define MR_MAX_LIGHTS 4
typedef struct mr_light_desc {
    int32_t type;                   /* MR_LIGHT_* */
    int32_t pad;
    double pos[3], dir[3], color[3], ambient[3];   /* as light_pos / light_dir / light_color / light_ambient of mr_frame_desc */
    double specular_strength;
    double att_constant, att_linear, att_quadratic;
    double spot_edge0, spot_edge1;
} mr_light_desc;
int mr_scene_set_extra_lights(mr_scene *scene, const mr_light_desc *lights, int32_t n);

/* Tuning / test hook: capacities of the per-frame work lists -- entries per 16x16 tile for the small
 * triangle pairs, big triangle pairs and shadow quads, and entries of the large primitives' work list;
 * 0 keeps the current value.  The lists grow by themselves (a frame that overflowed one is reported by
 * mr_render / mr_get_stats as MR_E_OVERFLOW internally and rendered again); this only sets where they start. */
int mr_scene_set_list_capacities(mr_scene *scene, uint32_t small_pairs, uint32_t big_pairs, uint32_t quads, uint32_t work);

/* The debug-camera frustum overlay (obj/core.py:638; obj/frustums.py:46-103; obj/line.py:6-16) as flat
 * statement lists.  The host walks the frustum's edges (float64 DDA) segment by segment; every kept point
 * of a segment performs the reference's writes in the reference's order: centre (z and red), then for step
 * -1 and +1: z into the row neighbour, z into the column neighbour, half blend into the row neighbour, half
 * blend into the column neighbour.  target is (5, n_points) row-major: per target set (centre, row-1, col-1,
 * row+1, col+1) the linear pixel index row * width + col (row = screen y, not flipped) in a frame of height x
 * width; segments follow each other in drawing order and cover the point array.  The device replays the segments
 * in order (csrc/kernels_overlay.h).  Pointers are read during the call only.  NULL (or n_points == 0) removes the overlay.  Frames that set
 * MR_FRAME_OVERLAY replay it; the frame must have the size named here. */
typedef struct mr_overlay_desc {
    int32_t n_segments, n_points, height, width;
    const int32_t *seg_first, *seg_count;   /* (n_segments) first point and number of points of each segment */
    const int32_t *target;                  /* (5, n_points) */
    const double *z;                        /* (n_points) linearised depth of each point */
} mr_overlay_desc;
int mr_scene_set_overlay(mr_scene *scene, const mr_overlay_desc *overlay);

/* The same overlay straight from the two cameras, everything on the host side of the library in one call
 * (replaces obj/frustums.py:61-103 + obj/line.py:6-16: clipping, projection, DDA, dashes, index wrapping; the
 * upload is one asynchronous copy in front of the overlay kernel of the next frame that draws it; the lists are built
 * when first needed -- by mr_render / mr_render_async after the frame's kernels have been launched): the frustum's eight corners
 * (8 x 4, already divided by w: CUBE @ inv(debug MVP), obj/frustums.py:52-53), the viewing camera's six planes
 * (6 x 4), its MVP and viewport (4 x 4, row vectors), near / far, whether the viewing camera sits inside the
 * frustum (obj/frustums.py:57-60), and the frame's size. */
int mr_scene_set_overlay_cameras(mr_scene *scene, const double *corners, const double *planes, const double *mvp,
                                 const double *viewport, double near_plane, double far_plane, int32_t camera_inside,
                                 int32_t height, int32_t width);

/* Scene.render() -- obj/core.py:587-640: depth/ambient pass, shadow-volume stencil pass, lit
 * pass and finalise (flip, **0.8, *255, uint8) on the GPU.  out_rgb receives
 * (row_end - row_begin) x width x 3 bytes, row 0 = top row of the band (divided by s twice with
 * MR_FRAME_SUPERSAMPLE2/4, as for mr_render_async and mr_render_device).  stats may be NULL. */
int mr_render(mr_scene *scene, const mr_frame_desc *frame, uint8_t *out_rgb, mr_stats *stats);

/* The overlay on a frame split over several devices.  The lines test z at pixels other devices own, so a device that
 * renders only part of the frame (row_begin / row_end of equal bands, or stripe_count > 1) with MR_FRAME_OVERLAY does not
 * draw the overlay; it APPENDS the state (z, float colour: 24 bytes) of every touched pixel it owns to its rows, at
 * offset round_up(bytes of its rows, 16) of d_out_rgb, mr_overlay_state_bytes() bytes in all (the same on every device:
 * one entry per touched pixel, the owner fills its own).  After the ONE all-gather of rows + state, every device calls
 * mr_overlay_apply: d_parts holds the `world` parts, part_stride bytes apart, the state at state_offset in each;
 * `striped` says how the rows were split (interleaved tile rows, else equal bands); d_frame is the assembled uint8
 * frame (height x width x 3, row 0 = top), whose touched pixels are rewritten.  The result is the frame one device
 * renders with the overlay on.  Work is enqueued on `stream` (NULL = the library's own). */
int64_t mr_overlay_state_bytes(mr_scene *scene);
int mr_overlay_apply(mr_scene *scene, const void *d_parts, int64_t part_stride, int64_t state_offset, int32_t world,
                     int32_t striped, int32_t system, void *d_frame, void *stream);

/* mr_render in two halves, for frames of a sequence: mr_render_async enqueues the frame and the device-to-host copy
 * of its uint8 rows into out_rgb on one of the scene's MR_ASYNC_LANES lanes (a stream and a set of work buffers
 * each) and returns at once; mr_render_wait blocks until that lane's frame is in out_rgb.  With two lanes the copy
 * of frame i (6 MB at 1080p: longer than the frame's kernels) runs beside the kernels of frame i + 1 and beside the
 * host's preparation of frame i + 2.  out_rgb should be page-locked (mr_host_alloc) for the copy to be
 * asynchronous at all.  A frame that overflowed a work list is reported by mr_render_wait as MR_E_OVERFLOW (the
 * lists have been grown): render it again.  stats may be NULL. */
#define MR_ASYNC_LANES 4
int mr_render_async(mr_scene *scene, const mr_frame_desc *frame, uint8_t *out_rgb, int32_t lane);
int mr_render_wait(mr_scene *scene, int32_t lane, mr_stats *stats);

/* Page-locked host memory for mr_render's out_rgb (hipHostMalloc / hipHostFree): the device-to-host copy
 * of the frame then runs at the full PCIe rate instead of being staged through the runtime's own buffers.
 * Optional: mr_render accepts any host pointer.  mr_host_alloc returns NULL on failure. */
void *mr_host_alloc(uint64_t bytes);
void mr_host_free(void *p);

/* Host arithmetic, no device involved: out (m x p) = a (m x k) @ b (k x p) in float64, every element
 * rn(a[i][0] * b[0][j]) followed by fma steps in ascending k -- the order the reference's NumPy / OpenBLAS stack
 * uses for its 4x4 products (obj/core.py:383-405, obj/transformation.py), which the per-frame constants must
 * reproduce bit for bit.  The Python mirror builds its matrices, planes and overlay polygons with it. */
void mr_host_matmul_chain(const double *a, const double *b, double *out, int32_t m, int32_t k, int32_t p);

/* Host arithmetic too: what Scene.render() derives from a camera that moved, in one call -- look-at = translate @
 * rotate, MVP = look-at @ projection (obj/core.py:383-405, obj/transformation.py:57-110) and the six normalised
 * frustum planes of the MVP (obj/plane_intersection.py:43-56), with the operation order of the Python mirror (scalar
 * look-at axes, products as ascending fma chains).  eye / center / up are the arguments of look_at_rotate_lh|rh (the
 * reference passes the camera's centre as eye and its position as centre), position the camera's position,
 * projection the 4 x 4 projection matrix (row vectors), lh != 0 the left-handed rotation.  Outputs: lookat (4 x 4),
 * mvp (4 x 4), planes (6 x 4: left, right, bottom, top, near, far). */
void mr_host_camera_constants(const double *eye, const double *center, const double *up, const double *position,
                              const double *projection, int32_t lh, double *lookat, double *mvp, double *planes);

/* Host arithmetic too: the statement lists of the debug-camera frustum overlay (what mr_scene_set_overlay takes),
 * from the frustum's eight corners (8 x 4, already divided by w: CUBE @ inv(debug MVP), obj/frustums.py:52-53), the
 * viewing camera's six planes (6 x 4), its MVP and viewport (4 x 4, row vectors), near / far, and whether the
 * viewing camera sits inside the frustum (obj/frustums.py:57-60).  Replaces obj/frustums.py:61-103 +
 * obj/line.py:6-16 on the host: clipping, projection, DDA, dashes, index wrapping, same-target links.
 * _build leaves the lists in a per-thread buffer and reports their sizes; _fetch copies them into the caller's
 * arrays (target / next: 5 x n_points, row-major; any pointer may be NULL). */
int mr_host_overlay_build(const double *corners, const double *planes, const double *mvp, const double *viewport,
                          double near_plane, double far_plane, int32_t camera_inside, int32_t height, int32_t width,
                          int32_t *n_segments, int32_t *n_points, int32_t *n_touched);
int mr_host_overlay_fetch(int32_t *seg_first, int32_t *seg_count, int32_t *target, int32_t *next, double *z,
                          int32_t *touched);

/* Same, but leaves the uint8 band in device memory at d_out_rgb (a device pointer owned by
 * the caller, e.g. a torch tensor's data_ptr) and does not synchronise the host: work is
 * enqueued on `stream` (a hipStream_t; NULL = the library's own stream).  Used by the
 * multi-GPU path, which all-gathers the bands with RCCL. */
int mr_render_device(mr_scene *scene, const mr_frame_desc *frame, void *d_out_rgb, void *stream);

/* Counters / timings of the last mr_render on this scene. */
int mr_get_stats(mr_scene *scene, mr_stats *stats);

/* Average device time in milliseconds (HIP events on the stream the kernels ran on) of each
 * stage over the most recent frames that carry event marks (at most n_frames of them; 64 frames per
 * stream are remembered, frames rendered with MR_FRAME_NO_TIMING are skipped).
 *   [0] k_vertex_mfma (0 unless MR_VERTEX_PATH=mfma)   [1] k_setup   [2] k_bin_work   [3] k_tile
 *   [4] whole frame (start -> after k_tile)
 * Frames rendered with MR_FRAME_LIGHT_TIMING report [0..1] as 0 and [2] as the span from the start of
 * the frame to the start of k_tile.
 * Synchronises the device.  Returns the number of frames averaged or a negative error. */
#define MR_N_KERNEL_TIMES 5
int mr_get_kernel_times(mr_scene *scene, int n_frames, float *out_ms, int cap);
/* The same over the frames enqueued on ONE stream (as passed to mr_render_device; NULL = the library's own). */
int mr_get_stream_kernel_times(mr_scene *scene, void *stream, int n_frames, float *out_ms, int cap);

/* Debug taps for parity tests: the reference's working buffers after the last render
 * (obj/core.py:588-591).  Row = screen y (not flipped), as in the reference.  (H, W) is the frame's
 * width / height as passed, i.e. the sample grid of a supersampled frame. */
/* z, stencil and winner need a frame rendered with MR_FRAME_KEEP_BUFFERS. */
int mr_read_z(mr_scene *scene, double *out_hw);            /* z_buffer, float64 (H, W) */
int mr_read_stencil(mr_scene *scene, int16_t *out_hw);     /* stencil_buffer, int16 (H, W) */
int mr_read_winner(mr_scene *scene, int32_t *out_hw);      /* face that owns each pixel, -1 = none */
int mr_read_frame_f32(mr_scene *scene, float *out_hw3);    /* float frame before finalise (needs MR_FRAME_KEEP_FLOAT) */
int mr_read_face_status(mr_scene *scene, uint8_t *out_faces);  /* MR_FACE_* per face (needs MR_FRAME_FACE_STATUS) */
/* Silhouette edges of the last frame as (model, a, b) triples, oriented like the entries of
 * the reference's model.silhouette (obj/triangular.py:294-302).  Returns the number of edges
 * (may exceed cap; only cap are written) or a negative error. */
int mr_read_silhouette(mr_scene *scene, int32_t *out_triples, int32_t cap);
/* The same two taps for light k of the last frame (0 = the descriptor's light: what the two above read; 1.. = the
 * lights of mr_scene_set_extra_lights).  A light's silhouette edges come in no particular order. */
int mr_read_stencil_light(mr_scene *scene, int32_t light, int16_t *out_hw);
int mr_read_silhouette_light(mr_scene *scene, int32_t light, int32_t *out_triples, int32_t cap);

/* Diagnostics: the tile kernel's per-tile records of the last frame, MR_TILE_RECORD_WORDS uint32 per tile:
 * [0..4] triangle fragments, quad fragments, stencil updates, covered px, lit px (MR_FRAME_COUNTERS);
 * [5..7] lengths of the tile's lists: small triangle pairs, big triangle pairs, shadow quads;
 * [8],[9] start and end of the tile's workgroup in 10 ns ticks (low 32 bits); [10],[11] the ticks at
 * which its coverage / z phase and its shadow-quad phase ended.
 * Words [0..4] and [8..11] are the general kernel's (mr_debug_frame_path out[0] == 1; mr_debug_force_full): the frame-only
 * kernel writes neither: [0..4] and [8..11] read 0 after such a frame.
 * Returns the number of tiles (tiles are 16 x 16 px, row-major over the rendered rows) or a negative error. */
#define MR_TILE_RECORD_WORDS 12
int mr_debug_read_tile_records(mr_scene *scene, uint32_t *out, int32_t cap_tiles);

/* Diagnostic: how many 64-face clusters the last frame's set-up kernel dropped whole (off the screen, off this device's
 * rows, or -- when the frame culls back faces -- turned away from the camera) before reading a face of them.  Counted
 * only when the environment has MR_CLUSTER_CULL=count; 0 otherwise.  The faces that ARE set up, and the frame, do not
 * depend on it.  By default clusters are culled on partial frames (a row band, stripes), where most of them go, and not
 * on whole frames, where the test costs more than it saves; MR_CLUSTER_CULL=0 / 1 / box force it off / on /
 * on with the screen and row test only. */
int mr_debug_clusters_culled(mr_scene *scene);

/* Diagnostic: how the tile kernel walked the last frame's shadow quads (frames with MR_FRAME_COUNTERS and one light; 0
 * otherwise): out[0] = (quad, row) items of the span walk, out[1] = (quad, strip) pairs walked a pixel per lane, out[2] =
 * those of out[1] whose polygon has more than four vertices, out[3] = those with a non-finite edge value (the two kinds
 * the span walk is not defined for).
 * MR_QUAD_WALK=strips | spans in the environment (read once per process) forces either walk; the frames do not depend on
 * it. */
int mr_debug_quad_walks(mr_scene *scene, uint32_t *out);

/* Diagnostic: where the winners' sweep over the last frame's small (triangle, tile) pairs got its z keys (frames with
 * MR_FRAME_COUNTERS; 0 otherwise): out[0] = covered samples answered from the lanes' logs, out[1] = samples walked again
 * by lanes whose log had run over (or that met a face of a depth_test == 0 model).  The general kernel of a frame with
 * several lights keeps no log: out[0] = 0 there.
 * MR_PAIR_LOG=0 .. 4 in the environment (read once per process) sets the entries a lane's log may hold, 0 for none: every
 * sample is then walked again; the frames do not depend on it. */
int mr_debug_pair_log(mr_scene *scene, uint32_t *out);

/* Diagnostic: how many (large triangle, tile) pairs the last frame's k_bin_work left out of the tile lists because the
 * triangle can cover no sample of the tile (frames with MR_FRAME_COUNTERS; 0 otherwise).  Such a pair added nothing but
 * work: the frame, z, winner, stencil and every statistic but tri_bin_entries, which is smaller by this number, do not
 * depend on it.  MR_BIG_TRI_REJECT=0 in the environment (looked up for every frame) lists every tile of a large
 * triangle's box as before. */
int mr_debug_big_tri_rejects(mr_scene *scene);

/* The set-up and tile kernels exist in two variants of one source: the frame-only ones, which count nothing, and the
 * general ones.  A frame takes the general kernels when it carries MR_FRAME_COUNTERS or MR_FRAME_FACE_STATUS or the
 * scene has a model with depth_test == 0; every other frame the frame-only ones.  The frame, z, winner and stencil do
 * not depend on the variant.  mr_debug_force_full(scene, 1) makes every later frame of the scene take the general
 * kernels, (scene, 0) returns to the rule.  Launches nothing. */
int mr_debug_force_full(mr_scene *scene, int32_t on);

/* Which kernels the most recent frame launched: out[0] = 1 the general variants (k_setup_full, k_tile_full), 0 the
 * frame-only ones; out[1] = 1 the tile kernel that shares heavy tiles out (SPLIT); out[2] = 1 the supersampled one;
 * out[3] = 1 the multi-light ones; out[4] = 1 the tile kernel followed the heaviest-first order, 0 row-major.  Does not wait for the device. */
int mr_debug_frame_path(mr_scene *scene, int32_t *out);

/* Diagnostics of the silhouette cache: out[0] = the path the edge half of the most recently enqueued frame
 * with shadows took (0 fused: every edge tested against the light; 1 fused, and captured into the cache; 2 read from the
 * cache; -1 no such frame yet), out[1] = the entries that frame read from the cache (0 unless out[0] == 2), out[2] =
 * captures started on this scene so far, out[3] = cache buffers that hold a usable silhouette.  A silhouette is captured
 * when two consecutive frames have the same light (type, position and direction, compared bit for bit) and is dropped
 * with the geometry; MR_SIL_CACHE=0 in the environment (looked up per frame) keeps every frame on the fused path.  The
 * frames do not depend on it.  Does not wait for the device. */
int mr_debug_sil_cache(mr_scene *scene, int32_t *out);

/* Diagnostics: the order in which the most recent frame's tile kernel took its tiles (entry b = the tile
 * of workgroup b): heaviest first by the estimate the slot's previous frame left, row-major for a first
 * frame or a new tile grid.  Always a permutation of 0 .. n_tiles-1.  Returns the number of tiles. */
int mr_debug_read_tile_order(mr_scene *scene, uint32_t *out, int32_t cap_tiles);

/* A model's pose: the model (index as mr_scene_add_model returned it) renders as if its vertices were the float64 array
 * V' = vertices @ m16, every element rn(v[0] * m[0][j]) followed by fma steps in ascending k (mr_host_matmul_chain) --
 * the reference's `Model @ M` with the product's rounding pinned.  m16 is a row-major 4 x 4 in the row-vector
 * convention; NULL removes the pose.  Vertices only: vertex normals (but see mr_scene_set_model_pose_normals), uv, materials and topology stay.  The pose is
 * absolute (it replaces the one before) and the vertices passed to mr_scene_add_model are never changed.  V' is float64,
 * so a posed model behaves as one with vertices_are_f32 == 0.
 * The call copies m16 and launches nothing.  The next frame applies what changed in one pass on the device (vertices,
 * face normals, edge records, per-face and per-cluster records); that pass waits for the device before and after, like
 * a commit.  When a model with vertices_are_f32 != 0 goes from un-posed to posed or back, one ordinary commit of the
 * scene comes first.  MR_E_INVALID for a model index out of range or an entry that is not finite. */
int mr_scene_set_model_pose(mr_scene *scene, int32_t model, const double *m16);

/* A posed model's normal matrix: with g9 = G (row-major 3 x 3, row vectors; the caller passes the inverse transpose of the
 * pose's upper-left 3 x 3) the model renders as if its vertex normals were float32(normals @ G) and every object-space
 * normal map of its materials (tex_norm >= 0, norm_tangent == 0) held float32(texel @ G) -- every component
 * rn(n[0] * G[0][j]) followed by fma steps in ascending k, in float64, rounded to float32 once; nothing is re-normalised.
 * Tangent-space maps, tex_kd and tex_ks are not touched, and a texture shared with another model stays what it was for
 * that model.  NULL: the normals stay as they were passed (the default).  Valid only for a model that has a pose;
 * removing the pose removes the matrix.  The call copies g9 and launches nothing: the next frame's pose pass does the
 * work (a matrix alone, the pose as it was, leaves the vertices' part of the pass out).
 * MR_E_INVALID for a model index out of range, a model without a pose or an entry that is not finite. */
int mr_scene_set_model_pose_normals(mr_scene *scene, int32_t model, const double *g9);

/* Diagnostics of the pose pass: out[0] = full commits of this scene so far, out[1] = pose passes so far, out[2] = models
 * that have a pose now, out[3] = vertices the last pass wrote.  Does not wait for the device. */
int mr_debug_pose(mr_scene *scene, int32_t *out);

/* Device time in milliseconds (HIP events on the library's stream) of the five steps of the last pose pass:
 *   [0] k_pose_vertices (with the copies that give un-posed models their vertices back)   [1] k_face_normals
 *   [2] k_edge_normals   [3] k_face_static   [4] k_clusters
 * MR_E_INVALID before the first pass.  The pass has waited for its kernels: this call does not wait. */
#define MR_N_POSE_TIMES 5
int mr_debug_pose_times(mr_scene *scene, float *out_ms);

/* The same for the two kernels of the last pass that had normal matrices to apply: [0] k_pose_normals  [1] k_pose_texels
 * (0 for one that pass did not launch: no normals, or no object-space map).  MR_E_INVALID before the first such pass. */
#define MR_N_POSE_NORMALS_TIMES 2
int mr_debug_pose_normals_times(mr_scene *scene, float *out_ms);

/* A model's skin (linear-blend skinning): joints and weights are (n_vertices, 4), row-major -- vertex i follows the bones
 * joints[i][0..3] by the weights weights[i][0..3], used as given (not normalised; a slot may repeat a joint or weigh 0).
 * Every joint lies in [0, n_bones).  normal_owner is (n_normals) -- for every vertex normal of the model the index of the
 * vertex whose blend matrix it takes, -1 for a normal that stays -- or NULL when the normals do not follow the skin (it
 * is ignored for a model without normals).  joints == NULL removes the skin and its bones.  Everything is copied during
 * the call and nothing is launched; a skin alone changes no frame.  Setting a skin puts the model in the rest position
 * (no bones).  MR_E_INVALID for a model index out of range, missing weights, n_bones <= 0, a joint or an owner out of
 * range or a weight that is not finite. */
int mr_scene_set_model_skin(mr_scene *scene, int32_t model, const int32_t *joints, const double *weights, int32_t n_bones,
                            const int32_t *normal_owner);

/* The bones of a model that has a skin: bones16 is (n_bones, 4, 4), row-major, row-vector convention like a pose; NULL is
 * the rest position (the model as it was added).  With bones B the model renders as if its vertices were the float64 array
 *   S_i[r][c] = rn(w[i][0] * B[j[i][0]][r][c]) followed by fma steps over slots 1, 2, 3        (the blend matrix of vertex i)
 *   V'[i]     = vertices[i] @ S_i, the chain of mr_scene_set_model_pose
 * and, where the skin has a normal_owner table, its vertex normals float32(float64(normal) @ S_owner[:3][:3]) (the same
 * chain over three terms; not re-normalised, not the inverse transpose: exact in direction for bones that rotate,
 * translate and scale uniformly).  A pose set as well follows the skin: V' @ m16, and normals @ G before the one rounding
 * to float32.  Object-space normal maps do not follow a skin.  V' is float64: the model behaves as one with
 * vertices_are_f32 == 0, as a posed one does.  The call copies the matrices and launches nothing; the next frame's pose
 * pass does the work (k_skin_vertices, k_skin_normals, then the kernels of every pose pass).
 * MR_E_INVALID for a model index out of range, a model without a skin, n_bones other than the skin's, or an entry that
 * is not finite. */
int mr_scene_set_model_bones(mr_scene *scene, int32_t model, const double *bones16, int32_t n_bones);

/* Host arithmetic, no device needed: V' of mr_scene_set_model_bones for n vertices -- verts and out are (n, 4) float64,
 * joints (n, 4) int32, weights (n, 4) float64, bones (any, 4, 4) float64 -- in the chains the device uses, bit for bit. */
void mr_host_skin_chain(const double *verts, const int32_t *joints, const double *weights, const double *bones, int32_t n, double *out);

/* The same for n 3-vectors (normals, already widened to float64): out[i] = vectors[i] @ S[:3][:3] of vertex owner[i],
 * or vectors[i] itself where owner[i] < 0.  joints and weights are the model's (n_vertices, 4) tables.  Not rounded to
 * float32: out is (n, 3) float64. */
void mr_host_skin_chain3(const double *vectors, const int32_t *owner, const int32_t *joints, const double *weights, const double *bones,
                         int32_t n, double *out);

/* Diagnostics of the skin: out[0] = models that have bones now, out[1] = bone matrices the last pose pass uploaded,
 * out[2] = vertices and out[3] = normals the last pose pass skinned.  Does not wait for the device. */
int mr_debug_skin(mr_scene *scene, int32_t *out);

/* Device time in milliseconds of the two skin kernels of the last pose pass that had a skin to apply:
 * [0] k_skin_vertices  [1] k_skin_normals (0 for one that pass did not launch).  k_skin_vertices runs inside span [0]
 * of mr_debug_pose_times.  MR_E_INVALID before the first such pass. */
#define MR_N_SKIN_TIMES 2
int mr_debug_skin_times(mr_scene *scene, float *out_ms);

/* A model's morph targets (blend shapes), CSR by target: target k displaces vertex index[j] by delta[3 j .. 3 j + 2] for
 * j in [first[k], first[k + 1]); first has n_targets + 1 offsets and starts at 0.  nfirst / nindex / ndelta are the same
 * for the model's vertex normals (their indices count the normals, not the vertices), or NULL when the normals do not
 * follow the morph.  first == NULL removes the morph and its weights.  Every index lies inside the model's vertex (normal)
 * count and is named at most once per target, every delta is finite, n_targets >= 1: checked here, so that the kernels
 * index without checks.  Everything is copied during the call (as per-vertex lists in ascending target order, padded per
 * 64 vertices to the longest list among them; the padded totals must fit 32 bits) and nothing is launched; a morph alone
 * changes no frame.  Setting a morph puts the model in the rest shape (no weights).  MR_E_INVALID otherwise, also for
 * normal tables on a model without normals. */
int mr_scene_set_model_morph(mr_scene *scene, int32_t model, int32_t n_targets, const int32_t *first, const int32_t *index,
                             const double *delta, const int32_t *nfirst, const int32_t *nindex, const double *ndelta);

/* The weights of a model that has a morph: w is (n_targets) float64, used as given (not clamped); NULL is the rest shape
 * (the model as it was added).  With weights w the model renders as if its vertices were the float64 array
 *   V_m[i][c] = vertices[i][c], then acc = fma(w[k], delta_k[i][c], acc) for every target k that lists i, k ascending  (c < 3)
 *   V_m[i][3] = vertices[i][3]
 * -- a listed target takes its step also with a weight of 0 -- and, with normal tables, its vertex normals the float32
 * array formed by the same chain from float64(normal), rounded once.  Skin, pose and normal matrix apply to that model:
 * morph first, then skin, then pose.  V_m is float64: the model behaves as one with vertices_are_f32 == 0, as a posed one
 * does.  The call copies w and launches nothing; the next frame's pose pass does the work (k_morph_vertices,
 * k_morph_normals, then the kernels of every pose pass).  MR_E_INVALID for a model index out of range, a model without a
 * morph, n_targets other than the morph's, or a weight that is not finite. */
int mr_scene_set_model_morph_weights(mr_scene *scene, int32_t model, const double *w, int32_t n_targets);

/* Host arithmetic, no device needed: V_m of mr_scene_set_model_morph_weights for n vectors -- base and out are (n, width)
 * float64, width 4 (vertices; the fourth component passes through) or 3 (normals widened to float64; out is not rounded)
 * -- from the tables as mr_scene_set_model_morph takes them and n_targets weights.  It builds the per-vertex lists the
 * device path builds and walks them in the kernels' order, bit for bit.  MR_OK, or MR_E_INVALID for tables
 * mr_scene_set_model_morph would refuse or a width other than 3 and 4. */
int mr_host_morph_chain(const double *base, int32_t n, int32_t width, int32_t n_targets, const int32_t *first, const int32_t *index,
                        const double *delta, const double *w, double *out);

/* Diagnostics of the morphs: out[0] = models that have weights now, out[1] = targets (weights) the last pose pass
 * uploaded, out[2] = vertices and out[3] = normals it morphed, out[4] = entries, padding included, of the lists on the
 * device.  Does not wait for the device. */
int mr_debug_morph(mr_scene *scene, int32_t *out);

/* Device time in milliseconds of the two morph kernels of the last pose pass: [0] k_morph_vertices  [1] k_morph_normals
 * (0 for one that pass did not launch).  k_morph_vertices runs inside span [0] of mr_debug_pose_times.  MR_E_INVALID
 * before the first pass over a morph. */
#define MR_N_MORPH_TIMES 2
int mr_debug_morph_times(mr_scene *scene, float *out_ms);

/* on = 1: while the model moves (weights on its morph, bones on its skin, or a pose) and has vertex normals, the pose
 * pass rebuilds those normals from the moved vertices V -- the float64 array the model renders with -- whenever it
 * rewrites the model's geometry.  For normal q, L(q) is every face of the model that has at least one corner whose
 * normal column is q, once, in ascending face order; with a, b, c the vertices of the face's corners 0, 1, 2,
 *   cr(f) = (b - a) x (c - a)        every operation rounded on its own, no fma
 *   acc   = cr(L[0]), then acc = acc + cr(L[k]) for k = 1 .. in order, component by component
 *   l     = sqrt((acc0 * acc0 + acc1 * acc1) + acc2 * acc2);   N[q] = float32(acc / l)
 * and the normal as it was added stays where L(q) is empty, l is 0, or a component of acc or l is not finite.  For these
 * normals it takes the place of the morph's normal tables, of the skin's normal owners and of the vector part of the
 * normal matrix: none of them is applied first (k_morph_normals, k_skin_normals and k_pose_normals leave the model out);
 * object-space normal maps are re-baked with the normal matrix as ever.  on = 0 (the default) brings those paths back.
 * The call launches nothing and passes no tables: the per-normal face lists are built from the faces the scene holds
 * when the flag is first on (sliced per 64 normals, padded to the longest list among them; the padded total must fit
 * 32 bits).  For a model at rest or without normals the flag changes nothing.  MR_E_INVALID for a model index out of
 * range or a value other than 0 and 1. */
int mr_scene_set_model_auto_normals(mr_scene *scene, int32_t model, int32_t on);

/* Host arithmetic, no device needed: N of mr_scene_set_model_auto_normals for one model -- verts (n_verts, 4) float64,
 * faces12 (n_faces, 12) int32 as the library keeps face rows (corner k at [4 k .. 4 k + 3]: vertex, uv, normal, material;
 * indices count this model's arrays), normals_in and out (n_normals, 3) float32.  It builds the lists the device path
 * builds and walks them in the kernel's order, bit for bit.  MR_OK, or MR_E_INVALID for a vertex or normal index out
 * of range. */
int mr_host_auto_normals(const double *verts, int32_t n_verts, const int32_t *faces12, int32_t n_faces, const float *normals_in,
                         int32_t n_normals, float *out);

/* Diagnostics of the rebuilt normals: out[0] = models the last pose pass rebuilt, out[1] = normals it wrote, out[2] =
 * entries, padding included, of the face lists on the device, out[3] = normals among out[1] that kept the value they
 * were added with.  Reads a few counters back from the device (the pass has waited for its kernels). */
int mr_debug_auto_normals(mr_scene *scene, int32_t *out);

/* Device time in milliseconds of k_auto_normals in the last pose pass (0 if that pass did not launch it); it runs
 * inside span [0] of mr_debug_pose_times.  MR_E_INVALID before the first pass that rebuilt normals. */
#define MR_N_AUTO_NORMALS_TIMES 1
int mr_debug_auto_normals_times(mr_scene *scene, float *out_ms);

/* The accumulation: a weighted sum of float frames on the device, finalised once (motion blur over poses or bones, an
 * area light as a point light averaged over positions, a jittered camera, progressive refinement of any of them).  It
 * lives on the sample grid (Hs, Ws) of its sub-frames -- the frame descriptor's height and width, (s H, s W) with
 * MR_FRAME_SUPERSAMPLE2/4 -- rows bottom-up like every tap.  With F_k the float32 frame mr_read_frame_f32 would return
 * after sub-frame k rendered with MR_FRAME_KEEP_FLOAT (after the overlay, after the sum over the lights) and w_k its
 * weight converted to float32, every operation float32 and rounded on its own (no fma):
 *   A_0 = w_0 * F_0
 *   A_k = A_{k-1} + (w_k * F_k)                       k = 1, 2, ...
 *   M   = the mean of A over each s x s block         (summed row by row from the block's bottom-left sample, times 1 / s^2;
 *                                                      s = 1: A itself)
 *   R   = min(M * scale, 1.0f)
 *   out = uint8(R ** 0.8 * 255), rows flipped         (uint8 (H, W, 3), row 0 = top)
 * A scene has one accumulation.  Frames rendered in between (mr_render, mr_render_async, mr_render_device) and
 * mr_scene_clear leave it alone.
 *
 * mr_accum_begin empties it (the buffer is kept for reuse).  Launches nothing.
 * mr_accum_add renders the frame like mr_render does -- on the library's stream, MR_FRAME_KEEP_FLOAT forced on, again
 * (up to six attempts) after a work list overflowed -- and adds it with k_accum_add once its lists are known to have
 * held.  It does not wait for that kernel, and no frame bytes are copied to the host.  The first add fixes width, height
 * and the supersample flags.  MR_E_INVALID for a later add that differs in one of them, for a partial frame (row band,
 * stripes), for MR_FRAME_FACE_STATUS and for a weight that is not finite and > 0 as float32.
 * mr_accum_resolve finalises the sum as it stands with `scale` (finite and > 0 as float32) into out_rgb, (H, W, 3)
 * bytes, and waits.  The sum stays: it may be called again, and adds may follow it.  MR_E_INVALID before the first add.
 * mr_accum_read_f32 is the tap: A as it stands, float32 (Hs, Ws, 3).  Synchronises the device. */
int mr_accum_begin(mr_scene *scene);
int mr_accum_add(mr_scene *scene, const mr_frame_desc *frame, double weight);
int mr_accum_resolve(mr_scene *scene, double scale, uint8_t *out_rgb);
int mr_accum_read_f32(mr_scene *scene, float *out_hw3);

/* Diagnostics of the accumulation: out[0] = sub-frames added since mr_accum_begin, out[1] = sub-frames among them that
 * were rendered again after an overflow (counted per extra attempt), out[2], out[3] = the sample grid's height and
 * width (0 before the first add).  Does not wait for the device. */
int mr_debug_accum(mr_scene *scene, int32_t *out);

/* Device time in milliseconds (HIP events on the library's stream): [0] the last k_accum_add, [1] the last
 * k_accum_resolve (0 if there was none since mr_accum_begin).  Waits for the last add's kernel.  MR_E_INVALID before
 * the first add. */
#define MR_N_ACCUM_TIMES 2
int mr_debug_accum_times(mr_scene *scene, float *out_ms);

/* Host arithmetic, no device needed: the accumulation's definition for n frames -- frames is (n, height, width, 3)
 * float32 on the sample grid, weights (n) float64, shift = log2 s (0, 1 or 2) -- bit for bit what the device path
 * gives for the same F_k.  out_acc receives A, (height, width, 3); out_rgb the bytes, (height >> shift, width >> shift, 3),
 * each (uint8_t)(powf(R, 0.8f) * 255.0f): the function the device's step table is built from.  Either may be NULL.
 * MR_E_INVALID for n < 1, a weight or a scale that is not finite and > 0 as float32, a shift outside 0 .. 2, or a
 * height or width that is no multiple of 1 << shift. */
int mr_host_accum(const float *frames, const double *weights, int32_t n, int32_t height, int32_t width, int32_t shift,
                  double scale, float *out_acc, uint8_t *out_rgb);

/* Ambient obscurance from the z-buffer, applied to a frame's float colours before they are finalised: creases and the
 * space between a model and the floor it stands on get darker than open surfaces.  It lives on the frame's sample grid
 * (Hs, Ws), rows bottom-up like every tap.  With Z the z-buffer as mr_read_z returns it and F the float frame after the
 * sum over the lights and BEFORE the overlay:
 *
 *   eye depth   e = (float)((m0 * Z + m1) / (m2 * Z + m3)), m = depth_map: the two products, the two sums and the
 *               quotient float64, each rounded on its own (no fma), the result rounded once to float32.  A sample whose Z
 *               or whose e is not finite is background.  The z-buffer is no distance (it holds the reference's
 *               linearize_z of the viewport-transformed z); depth_map is the inverse of the chain from a point z_e on
 *               the view axis to Z -- projection, division by w, viewport, linearize_z, each a Moebius map, so the chain
 *               is a product of 2x2 matrices and its inverse the adjugate -- signed so that e > 0 in front of the camera.
 *               The caller builds it per view; the library only applies it.
 *   footprint   rp = perspective ? k / e_p : k, then rp = min(max(rp, 1), 32): float32, an IEEE division, in samples.
 *               k = float32(radius * 0.5 * Hs * |P[1][1]|) makes radius a length in world units.
 *   taps        eight antipodal pairs i = 0 .. 7 with unit offsets u_i = (cos(i pi / 8), sin(i pi / 8)) * (1 for even i,
 *               0.5 for odd i), float32 literals (csrc/ao_def.h): dx = (int)rintf(u_i.x * rp), dy likewise, ties to even;
 *               a = e(x + dx, y + dy), b = e(x - dx, y - dy).
 *   obscurance  float32, every operation rounded on its own, i ascending:
 *                 valid_i = both taps inside the frame and not background, fabsf(e_p - a) <= depth_range and
 *                           fabsf(e_p - b) <= depth_range        (an invalid pair contributes 0: the pair, not one tap)
 *                 c   = (e_p - a) + (e_p - b)          > 0 in a crease, <= 0 on a plane under perspective and on convex shapes
 *                 t   = (c - bias) * inv_fall          inv_fall = float32(1 / radius), the quotient in float64
 *                 occ = t < 0 ? 0 : (t > 1 ? 1 : t);   sum = sum + occ
 *               ao = 1 - strength * (sum * 0.125f);  ao = ao < 0 ? 0 : ao
 *   F'[p][ch] = F[p][ch] * ao;  a background sample keeps F.
 *
 * Where the frame draws an overlay it goes on F' and Z as ever: its lines are not darkened, and the Z they write is not
 * seen.  The bytes are the finalise of the result -- block mean, min(., 1), the gamma step, rows flipped: what
 * mr_host_accum gives for that one frame with weight 1 and scale 1.  mr_read_frame_f32 then returns the final float frame;
 * mr_read_z is unchanged.  By this definition the whole colour is darkened, not the ambient term alone; with several
 * lights the obscurance is applied once, after their sum; and a model that writes no z (depth_test = 0) is shaded by what
 * the buffer holds behind it.
 *
 * mr_scene_set_ambient_occlusion copies the description (NULL: off, the default); every frame enqueued afterwards, by
 * any entry point, uses the copy of its moment, so a caller may set another map per view while frames are in flight.
 * Such a frame keeps its z-buffer and float frame (MR_FRAME_KEEP_BUFFERS | MR_FRAME_KEEP_FLOAT are implied, every tile
 * writes its taps) and runs k_ao behind the tile kernel.  A scene without it enqueues what it always did.
 * MR_E_INVALID for radius, strength, depth_range or k that are not finite and > 0 as float32, strength > 8, a bias that
 * is not finite and >= 0, an entry of depth_map that is not finite, or perspective other than 0 / 1; and, from the
 * rendering entry points, for a partial frame (row band, stripes) of such a scene, before any device work: the taps
 * cross the bands.  MR_E_UNSUPPORTED from a library linked without ao.hip or accum.hip. */
typedef struct mr_ao_desc {
    double depth_map[4];       /* m0 .. m3 */
    double k;                  /* footprint in samples at eye depth 1 (perspective) or everywhere; used as float32 */
    double radius, strength, depth_range, bias;      /* used as float32 (radius also as 1 / radius) */
    int32_t perspective;       /* 1: the footprint shrinks with the eye depth; 0: an orthographic camera */
    int32_t pad;
} mr_ao_desc;
int mr_scene_set_ambient_occlusion(mr_scene *scene, const mr_ao_desc *ao);

/* Host arithmetic, no device needed: the definition above for one frame -- z is (height, width) float64, frame and
 * out_frame (height, width, 3) float32 (they may be the same array) -- bit for bit what k_ao leaves in the float frame.
 * MR_E_INVALID for what mr_scene_set_ambient_occlusion refuses, a NULL array or a height or width outside 1 .. 32767. */
int mr_host_ao(const double *z, const float *frame, int32_t height, int32_t width, const mr_ao_desc *ao, float *out_frame);

/* Diagnostics: out[0] = frames of this scene that enqueued k_ao (every enqueue, also one rendered again after an
 * overflow), out[1], out[2] = the sample rows and columns of the last of them (0 before the first).  Does not wait. */
int mr_debug_ao(mr_scene *scene, int32_t *out);

/* Device time in milliseconds of the last k_ao (HIP events on its frame's stream).  Waits for that kernel.
 * MR_E_INVALID before the first such frame. */
#define MR_N_AO_TIMES 1
int mr_debug_ao_times(mr_scene *scene, float *out_ms);

/* Depth of field from the z-buffer, a thin lens focused at eye depth `focus`, applied to a frame's float colours before
 * they are finalised: every sample is gathered from the samples whose circle of confusion reaches it.  It lives on the
 * frame's sample grid (Hs, Ws), rows bottom-up like every tap.  With Z the z-buffer as mr_read_z returns it and F the
 * float frame after the sum over the lights, after the ambient obscurance where that is on, and BEFORE the overlay:
 *
 *   eye depth   e as for the ambient obscurance above (depth_map, the same float64 chain, one rounding to float32); a
 *               sample whose Z or whose e is not finite is background, e = +inf.
 *   circle      s = perspective ? kf * (1 - focus / e) : kf * (e - focus): float32 from here on, every operation rounded
 *               on its own, IEEE divisions.  Signed: > 0 behind the plane in focus.  A background sample has s = kf under
 *               perspective and +inf under an orthographic camera.  kf = float32(lens_radius * 0.5 * Hs * |P[1][1]| /
 *               focus), the quotient chain in float64: a point at eye depth e spreads over a disc of lens_radius *
 *               |e - focus| / focus world units at its own depth, which is |s| samples.
 *   radius      c = min(|s|, 16);  rr = max(c * c, 0.25f): the squared radius; a sample always covers itself.
 *   gather      for dy = -16 .. 16 ascending, for dx = -16 .. 16 ascending, q = p + (dx, dy) inside the frame:
 *                 rr_t = s_q > s_p ? min(rr_q, rr_p) : rr_q      (q behind p: a blurred background does not bleed over a
 *                                                                 sharper foreground)
 *                 if (float)(dx * dx + dy * dy) <= rr_t:          (a tap that fails is skipped, not added as a zero)
 *                     w = 1.0f / rr_t;  W = W + w;  S[ch] = S[ch] + w * F[q][ch]        (the product rounded, then the sum)
 *   F'[p][ch] = S[ch] / W
 *
 * Background samples take part: a sky blurs.  Where c < 0.5 for p and for every q in front of it within 16 samples,
 * F'[p] == F[p] bit for bit.  One layer only: what a real lens sees round an occluder is not in F; no circle wider than 16
 * samples; a blurred foreground lets 4 / (4 + pi) of a sharp sample behind it through (that sample's own tap weighs 4, the
 * foreground's disc over it pi).
 *
 * Where the frame draws an overlay it goes on F' and Z as ever: its lines stay sharp.  The bytes are the finalise of the
 * result, as for the ambient obscurance: what mr_host_accum gives for that one frame with weight 1 and scale 1.
 * mr_read_frame_f32 then returns the final float frame (the accumulation adds it); mr_read_z is unchanged.
 *
 * mr_scene_set_depth_of_field copies the description (NULL: off, the default); every frame enqueued afterwards, by any
 * entry point, uses the copy of its moment.  Such a frame keeps its z-buffer and float frame (MR_FRAME_KEEP_BUFFERS |
 * MR_FRAME_KEEP_FLOAT are implied), runs k_dof behind the tile kernel and behind k_ao, and owns a second float frame.  A
 * scene without it enqueues what it always did.  MR_E_INVALID for focus or kf that are not finite and > 0 as float32, an
 * entry of depth_map that is not finite, or perspective other than 0 / 1; and, from the rendering entry points, for a
 * partial frame (row band, stripes) of such a scene, before any device work: the taps cross the bands.
 * MR_E_UNSUPPORTED from a library linked without dof.hip or accum.hip. */
typedef struct mr_dof_desc {
    double depth_map[4];       /* m0 .. m3, as in mr_ao_desc */
    double kf;                 /* circle of confusion in samples per unit of (1 - focus / e), or per unit of depth: float32 */
    double focus;              /* eye depth of the plane in focus, in world units; used as float32 */
    int32_t perspective;       /* 1: a perspective camera; 0: an orthographic one */
    int32_t pad;
} mr_dof_desc;
int mr_scene_set_depth_of_field(mr_scene *scene, const mr_dof_desc *dof);

/* Host arithmetic, no device needed: the definition above for one frame -- z is (height, width) float64, frame and
 * out_frame (height, width, 3) float32, two different arrays (neighbours' colours are read) -- bit for bit what k_dof
 * writes.  MR_E_INVALID for what mr_scene_set_depth_of_field refuses, a NULL array, out_frame == frame, or a height or
 * width outside 1 .. 32767. */
int mr_host_dof(const double *z, const float *frame, int32_t height, int32_t width, const mr_dof_desc *dof, float *out_frame);

/* Diagnostics: out[0] = frames of this scene that enqueued k_dof (every enqueue, also one rendered again after an
 * overflow), out[1], out[2] = the sample rows and columns of the last of them (0 before the first).  Does not wait. */
int mr_debug_dof(mr_scene *scene, int32_t *out);

/* Device time in milliseconds of the last k_dof (HIP events on its frame's stream).  Waits for that kernel.
 * MR_E_INVALID before the first such frame. */
#define MR_N_DOF_TIMES 1
int mr_debug_dof_times(mr_scene *scene, float *out_ms);

/* Diagnostics: the post-frame kernels on buffers the caller supplies -- no frame is rendered.  frames is (n, height,
 * width, 3) float32 and z (height, width) float64, both on the sample grid, rows bottom-up.  Each frame is uploaded,
 * darkened in place by k_ao where ao is not NULL (workgroup shape ao_shape: 0 = 64 x 64 samples, 1 = 32 x 32, 2 = 64 x
 * 16), blurred by k_dof into a second buffer where dof is not NULL (dof_shape: 0 = 32 x 32 samples and 1 024 threads, 1 =
 * 32 x 32 and 256, 2 = 16 x 16), and, where weights (n) is not NULL, added by k_accum_add into a sum that was filled with
 * 0xFF bytes first.  out_f32, (height, width, 3), receives the sum, or without weights the one processed frame; out_rgb,
 * ((height >> shift), (width >> shift), 3) or NULL, k_accum_resolve of it with the shift and the scale.  The shapes come
 * from the arguments, never from MR_AO_TILE / MR_DOF_TILE.  The scene lends its stream, its step table and the error
 * text: its frame slots, its last frame and what mr_debug_ao, mr_debug_dof and mr_debug_accum report stay as they were.
 * The device buffers are the entry's own and released before it returns; it waits for the device.
 * MR_E_INVALID, before any device call: a NULL scene, frames, z or out_f32; n < 1; height or width outside 1 .. 32767;
 * n > 1 without weights; a shape outside 0 .. 2 for a description that is given; a shift outside 0 .. 2 or one that does
 * not divide height and width; a weight or a scale that is not finite and > 0 as float32; whatever
 * mr_scene_set_ambient_occlusion or mr_scene_set_depth_of_field refuse.  MR_E_UNSUPPORTED from a library linked without
 * the translation unit of a kernel that is asked for. */
int mr_debug_post(mr_scene *scene, const float *frames, const double *z, int32_t n, int32_t height, int32_t width,
                  const mr_ao_desc *ao, int32_t ao_shape, const mr_dof_desc *dof, int32_t dof_shape, const double *weights,
                  int32_t shift, double scale, float *out_f32, uint8_t *out_rgb);

/* Motion blur from a per-sample velocity buffer, applied to a frame's float colours before they are finalised: every
 * sample is gathered from the samples whose motion segment passes over it.  It lives on the frame's sample grid (Hs, Ws),
 * rows bottom-up like every tap, at integer screen coordinates (x, y).  The library is stateless about time: the caller
 * hands over the matrices that lead from this frame's samples to where their surface points were on the previous frame's
 * sample grid (the Python layer keeps the previous camera and poses and builds them, _pack.motion_matrices).  With Z the
 * z-buffer (mr_read_z), w the winner map (mr_read_winner) and F the float frame after the sum over the lights, after the
 * ambient obscurance and the depth of field where they are on, and BEFORE the overlay:
 *
 *   velocity    class = w < 0 ? 0 : class_of_model[model of face w]     (model: the last m whose first face is <= w)
 *               T = matrices[class], 4 x 3 row-major;  B = background, 3 x 3 row-major
 *               finite Z:    u_c = ((x*Z)*T[0][c] + (y*Z)*T[1][c] + Z*T[2][c]) + T[3][c]         c = 0, 1, 2
 *               background (Z not finite):   u_c = (x*B[0][c] + y*B[1][c]) + B[2][c]
 *               front = finite Z ? u_2 * Z > 0 : u_2 > 0       (u is Z / w times the previous homogeneous screen position)
 *               U = front ? ((float)(x - u_0/u_2), (float)(y - u_1/u_2)) : (0, 0), and (0, 0) unless both are finite
 *               float64, left to right, every operation rounded on its own, IEEE divisions, one rounding to float32.  U is
 *               the displacement in samples since the previous frame, unclamped: what mr_read_velocity returns.
 *   segment     v = shutter * U;  L = sqrtf(v.x*v.x + v.y*v.y): float32 from here on, every operation rounded on its own
 *               0.5f <= L <= FLT_MAX:  h = min(L*0.5f, 16),  d = (v.x / L, v.y / L);   else  h = 0,  d = (1, 0)
 *   gather      e = the eye depth as for the ambient obscurance (a sample whose Z or e is not finite: e = +inf);
 *               for dy = -16 .. 16 ascending, for dx = -16 .. 16 ascending, q = p + (dx, dy) inside the frame:
 *                 o = (-dx, -dy);  along = o.x*d_q.x + o.y*d_q.y;  perp = o.x*d_q.y - o.y*d_q.x
 *                 h_t = (e_q > e_p && h_p < h_q) ? h_p : h_q       (a moving background does not smear over a stiller
 *                                                                    foreground)
 *                 if fabsf(along) <= h_t + 0.5f && fabsf(perp) <= 0.5f:       (a tap that fails is skipped)
 *                     w = 1.0f / (2.0f*h_t + 1.0f);  W = W + w;  S[ch] = S[ch] + w * F[q][ch]
 *   F'[p][ch] = S[ch] / W
 *
 * Class 0 is "the camera only": the background's class and that of every model whose pose did not change; a model whose
 * pose changed has a class of its own.  Where h = 0 for p and for every q in front of it within 16 samples, F'[p] == F[p]
 * bit for bit: a frame in which nothing moves by half a sample is the frame without the pass, byte for byte.  One layer
 * only: what shows behind a moving object is not in F; no segment longer than 33 samples.  The z-buffer interpolates
 * linearised depth linearly in screen space, so U is exact at vertices and on faces parallel to the image plane and
 * inherits that interpolation inside a large slanted triangle.
 *
 * Where the frame draws an overlay it goes on F' and Z as ever: its lines stay sharp.  The bytes are the finalise of the
 * result, as for the ambient obscurance.  mr_read_frame_f32 then returns the final float frame; mr_read_z and
 * mr_read_winner are unchanged.
 *
 * mr_scene_set_motion_blur copies everything during the call (NULL: off, the default); every frame enqueued afterwards, by
 * any entry point, uses the copy of its moment.  Such a frame keeps its z-buffer, winner map and float frame
 * (MR_FRAME_KEEP_BUFFERS | MR_FRAME_KEEP_FLOAT are implied), runs k_velocity and k_mblur behind the tile kernel, k_ao and
 * k_dof, and owns a second float frame and a velocity buffer.  A scene without it enqueues what it always did.
 * MR_E_INVALID for a shutter outside (0, 1] as float32, an entry of depth_map, of a matrix or of background that is not
 * finite, n_classes < 1, a class outside 0 .. n_classes - 1, or n_models other than the scene's; and, from the rendering
 * entry points, for a partial frame (row band, stripes) of such a scene, for a sub-frame of an accumulation, and for a
 * scene whose number of models changed since the call -- all before any device work.  MR_E_UNSUPPORTED from a library
 * linked without motion.hip or accum.hip. */
typedef struct mr_motion_desc {
    double depth_map[4];           /* m0 .. m3, as in mr_ao_desc */
    double shutter;                /* the part of the frame interval the shutter is open: (0, 1] as float32 */
    const double *matrices;        /* n_classes x 12: T of every class, 4 x 3 row-major */
    double background[9];          /* B, 3 x 3 row-major */
    const int32_t *class_of_model; /* n_models classes (may be NULL when n_models is 0) */
    int32_t n_classes, n_models;
} mr_motion_desc;
int mr_scene_set_motion_blur(mr_scene *scene, const mr_motion_desc *motion);

/* Host arithmetic, no device needed: the definition above, bit for bit what k_velocity and k_mblur write.  z is (height,
 * width) float64, winner (height, width) int32, face_off the first face of each of motion->n_models models (ascending from
 * 0), velocity and out_velocity (height, width, 2) float32, frame and out_frame (height, width, 3) float32, two different
 * arrays.  mr_host_motion_blur reads the description's depth_map and shutter only (its matrices must still be valid).
 * MR_E_INVALID for what mr_scene_set_motion_blur refuses, a NULL array, out_frame == frame, or a height or width outside
 * 1 .. 32767. */
int mr_host_velocity(const double *z, const int32_t *winner, const int32_t *face_off, int32_t height, int32_t width,
                     const mr_motion_desc *motion, float *out_velocity);
int mr_host_motion_blur(const double *z, const float *velocity, const float *frame, int32_t height, int32_t width,
                        const mr_motion_desc *motion, float *out_frame);

/* The last frame's velocity buffer U: float32 (Hs, Ws, 2), rows bottom-up.  MR_E_INVALID when the last frame ran without
 * motion blur.  Waits for the device. */
int mr_read_velocity(mr_scene *scene, float *out);

/* Diagnostics: out[0] = frames of this scene that enqueued k_velocity and k_mblur (every enqueue, also one rendered again
 * after an overflow), out[1], out[2] = the sample rows and columns of the last of them (0 before the first).  Does not wait. */
int mr_debug_motion(mr_scene *scene, int32_t *out);

/* Device times in milliseconds of the last k_velocity and the last k_mblur (HIP events on their frame's stream).  Waits for
 * them.  MR_E_INVALID before the first such frame.  A frame of a scene with temporal anti-aliasing took its U from the
 * k_velocity in front of k_taa and ran none of its own: its velocity span reads 0 (mr_debug_taa_times has that launch). */
#define MR_N_MOTION_TIMES 2
int mr_debug_motion_times(mr_scene *scene, float *out_ms);

/* Diagnostics: k_velocity and k_mblur on buffers the caller supplies -- no frame is rendered.  z, winner and frame as for
 * the host mirrors, face_off the first face of each of motion->n_models models; shape is k_mblur's workgroup: 0 = 32 x 32
 * samples and 1 024 threads, 1 = 32 x 32 and 256, 2 = 16 x 16 (never MR_MBLUR_TILE's).  out_velocity (height, width, 2)
 * and out_frame (height, width, 3) receive U and F'.  The scene lends its error text only: its frame slots, its last frame
 * and what mr_debug_motion reports stay as they were.  The device buffers are the entry's own and released before it
 * returns; it waits for the device.  MR_E_INVALID, before any device call, for a NULL argument, a height or width outside
 * 1 .. 32767, a shape outside 0 .. 2 and whatever mr_host_velocity refuses. */
int mr_debug_motion_post(mr_scene *scene, const double *z, const int32_t *winner, const float *frame, const int32_t *face_off,
                         int32_t height, int32_t width, const mr_motion_desc *motion, int32_t shape, float *out_velocity,
                         float *out_frame);

/* The velocity of models that bend.  The matrices of mr_motion_desc know the camera and every model's pose; a model whose
 * bones or morph weights changed moves vertex by vertex.  For the models flagged here, a frame with motion blur computes U
 * per winner face from the previous frame's deformed vertices instead, without the z-buffer.  With V_k the current world
 * positions of a face's corners, P_k their positions at the previous frame, Sn = s_now and Sp = s_prev the (x, y, w)
 * columns of the two frames' view . projection . viewport on the sample grid (4 x 3, row vectors, row-major), in float64,
 * left to right, every operation rounded on its own:
 *
 *   X_k = ((V_k.x*Sn[0][0] + V_k.y*Sn[1][0]) + V_k.z*Sn[2][0]) + Sn[3][0]    likewise Y_k, W_k (columns 1, 2), q_k from P_k, Sp
 *   A[0] = Y x W,  A[1] = W x X,  A[2] = X x Y          each component  a*b - c*d
 *   det  = (X_0*A[0][0] + X_1*A[0][1]) + X_2*A[0][2]
 *   H[r][c] = (A[r][0]*q_0[c] + A[r][1]*q_1[c]) + A[r][2]*q_2[c];   s = max |H[r][c]|
 *   H = 0 (all nine) unless det and s are finite, det != 0 and s > 0;  else H[r][c] = (det < 0 ? -H[r][c] : H[r][c]) / s
 *   u_c = (x*H[0][c] + y*H[1][c]) + H[2][c];  front = u_2 > 0;  U as for the background above
 *
 * (x, y, 1) . A are the sample's perspective-correct barycentrics on the face's plane, so U is exact there, also inside a
 * large slanted triangle; a degenerate face or a vertex that is no number has U = (0, 0).  Samples of other models and
 * uncovered samples keep the U of the matrices.  Frame order: k_velocity, k_face_homography, k_velocity_faces, k_mblur.
 *
 * The previous vertices are the library's one piece of state.  While tracking is on (mr_scene_track_vertices; off by
 * default, and then nothing is copied), every pose pass that is about to rewrite the vertices first copies them all,
 * device to device.  The vertex serial (mr_scene_vertices_serial) counts the states the device's vertices have held: + 1 for
 * every commit that uploads them and every pass that rewrites them.  prev_serial is the serial the caller read when the
 * previous frame was issued: the per-face pass runs only if the copy holds exactly that state.  Otherwise -- a commit or
 * other passes in between, tracking switched on too late -- the pass is skipped, counted, and the frame's U is the
 * matrices'.  A frame with no flagged model launches neither kernel.
 *
 * mr_scene_set_motion_faces copies everything during the call (NULL: off, the default) and needs
 * mr_scene_set_motion_blur before it.  MR_E_INVALID for an entry of s_now or s_prev that is not finite, n_models other than
 * the scene's or a NULL array; the mirrors and the debug entry refuse also a vertex index outside the vertex array, first
 * faces that do not ascend from 0 and a winner of a flagged model beyond the records -- all before any device work.
 * MR_E_UNSUPPORTED from a library linked without motion_faces.hip. */
typedef struct mr_motion_faces_desc {
    double s_now[12], s_prev[12];  /* Sn, Sp: 4 x 3 row-major */
    const int32_t *deforming;      /* n_models flags */
    int32_t n_models;
    int64_t prev_serial;
} mr_motion_faces_desc;
int mr_scene_set_motion_faces(mr_scene *scene, const mr_motion_faces_desc *faces);
int mr_scene_track_vertices(mr_scene *scene, int32_t on);
int64_t mr_scene_vertices_serial(mr_scene *scene);

/* Host arithmetic, no device needed: the definition above, bit for bit what the two kernels write.  verts_now and verts_prev
 * are (n_verts, 4) float64, faces n_faces records of 12 int32 with the corners' vertex indices at 0, 4 and 8; out_h receives
 * 9 doubles a face.  mr_host_velocity_faces overwrites, in velocity_in_out (height, width, 2), U of every sample whose
 * winner w >= 0 belongs to a model m with hom_off[m] >= 0, from record hom_off[m] + w - face_off[m] of h (n_records x 9);
 * every other float keeps its bits. */
int mr_host_face_homographies(const double *verts_now, const double *verts_prev, int32_t n_verts, const int32_t *faces, int32_t n_faces,
                              const double *s_now, const double *s_prev, double *out_h);
int mr_host_velocity_faces(const int32_t *winner, const int32_t *face_off, const int32_t *hom_off, int32_t n_models, const double *h,
                           int32_t n_records, int32_t height, int32_t width, float *velocity_in_out);

/* Diagnostics: k_face_homography and k_velocity_faces on arrays the caller supplies -- no frame is rendered.  The flagged
 * models' faces get records one model after the other; out_h receives them (9 doubles each: room for n_faces), and
 * velocity_in_out is read, overwritten as above and returned.  On the device both outputs lie between 256 bytes of
 * sentinel either side; out_guard receives the number of those bytes that changed (0 unless a kernel wrote out of bounds).
 * The scene lends its error text only.  Waits for the device. */
int mr_debug_motion_faces_post(mr_scene *scene, const double *verts_now, const double *verts_prev, int32_t n_verts, const int32_t *faces,
                               int32_t n_faces, const int32_t *face_off, const int32_t *deforming, int32_t n_models, const double *s_now,
                               const double *s_prev, const int32_t *winner, int32_t height, int32_t width, float *velocity_in_out,
                               double *out_h, int32_t *out_guard);

/* Diagnostics: the snapshot of the vertices, (n_verts, 4) float64 (MR_E_INVALID before the first); out[0] = frames that ran the
 * per-face pass, out[1] = frames that had flagged models and skipped it, out[2] = the records of the last pass, out[3] =
 * snapshots taken; and the device milliseconds of the last k_face_homography and the last k_velocity_faces. */
int mr_debug_read_prev_vertices(mr_scene *scene, double *out);
int mr_debug_motion_faces(mr_scene *scene, int32_t *out);
#define MR_N_MOTION_FACES_TIMES 2
int mr_debug_motion_faces_times(mr_scene *scene, float *out_ms);

/* Temporal anti-aliasing: a frame's float colours blended into the colours the previous frame of the scene left, fetched
 * where every sample's surface point was.  It lives on the frame's sample grid (Hs, Ws), rows bottom-up, at integer screen
 * coordinates p = (x, y).  With F the float frame after the sum over the lights and the ambient obscurance -- BEFORE the
 * depth of field, the motion blur and the overlay -- U the velocity (as for the motion blur: mr_read_velocity), P the
 * history or none and a = blend, float32 throughout, every operation rounded on its own:
 *
 *   C = F[p];   no history: out = C
 *   rx = (float)x - U.x;  ry = (float)y - U.y;   unless rx in [0, Ws-1] and ry in [0, Hs-1] (or no number): out = C
 *   x0 = (int)floorf(rx), fx = rx - (float)x0, x1 = min(x0 + 1, Ws-1);   y0, fy, y1 likewise
 *   t0 = P[y0][x0] + fx*(P[y0][x1] - P[y0][x0]);  t1 likewise on row y1;  H = t0 + fy*(t1 - t0)            per channel
 *   mn, mx = fminf / fmaxf over F at the 3 x 3 samples round p, coordinates clamped to the frame, rows then columns ascending
 *   Hk = fminf(fmaxf(H, mn), mx);   out = Hk + a*(C - Hk);   P'[p] = out for every sample
 *
 * U == 0 fetches H == P[p] bit for bit, and P == F then gives out == C bit for bit.  The neighbourhood clamp is the only
 * rejection of stale history.  Frame order: the lights' sum, k_ao, k_velocity (and the per-face pair where due), k_taa,
 * k_dof, k_mblur, the overlay, the finalise of the result; the history holds the frame as k_taa left it.  With motion blur
 * on as well, one k_velocity serves both: both descriptions must carry the same matrices, background and classes.
 *
 * The scene owns the history: two float frames on the sample grid.  A frame reads the one left by the last frame with the
 * pass whose mr_render or mr_render_wait returned MR_OK and writes the other, which that return hands over.  A frame that
 * overflowed a work list hands nothing over: rendered again, it reads the same history.  The history is forgotten by
 * mr_scene_reset_history, by mr_scene_set_temporal_aa(NULL) and by a frame on a sample grid of another size; the next
 * frame then has none, and a frame still in flight hands nothing over.
 *
 * mr_scene_set_temporal_aa copies everything during the call (NULL: off, the default); every frame enqueued afterwards
 * by mr_render or mr_render_async uses the copy of its moment, keeps its z-buffer, winner map and float frame
 * (MR_FRAME_KEEP_BUFFERS | MR_FRAME_KEEP_FLOAT are implied) and owns a second float frame and a velocity buffer.  A scene
 * without it enqueues what it always did.  MR_E_INVALID for a blend outside (0, 1] as float32 and whatever
 * mr_scene_set_motion_blur refuses of the matrices; and, from the rendering entry points, for a partial frame (row band,
 * stripes), a sub-frame of an accumulation, mr_render_device, a scene whose number of models changed since the call,
 * table blocks that differ from the motion blur's, and a frame enqueued while an earlier one with the pass has not been
 * waited for (host order is the only ordering between the frames' lanes) -- all before any device work.
 * MR_E_UNSUPPORTED from a library linked without taa.hip, motion.hip or accum.hip. */
typedef struct mr_taa_desc {
    double blend;                  /* the share of the new frame: (0, 1] as float32 */
    const double *matrices;        /* as in mr_motion_desc: n_classes x 12 */
    double background[9];
    const int32_t *class_of_model; /* n_models classes (may be NULL when n_models is 0) */
    int32_t n_classes, n_models;
} mr_taa_desc;
int mr_scene_set_temporal_aa(mr_scene *scene, const mr_taa_desc *taa);
int mr_scene_reset_history(mr_scene *scene);

/* The history as the scene holds it now: float32 (Hs, Ws, 3), rows bottom-up.  MR_E_INVALID, with a text, when there is
 * none.  Waits for the device. */
int mr_read_history(mr_scene *scene, float *out);

/* Host arithmetic, no device needed: the definition above, bit for bit what k_taa writes.  frame, history and out_frame
 * are (height, width, 3) float32, velocity (height, width, 2); history may be NULL (no history).  MR_E_INVALID for a NULL
 * array, out_frame == frame or == history, a blend outside (0, 1] as float32, or a height or width outside 1 .. 32767. */
int mr_host_taa(const float *frame, const float *velocity, const float *history, int32_t height, int32_t width, double blend,
                float *out_frame);

/* Diagnostics: out[0] = frames of this scene that enqueued k_taa (every enqueue, also one rendered again after an
 * overflow), out[1], out[2] = the sample rows and columns of the last of them (0 before the first), out[3] = k_velocity
 * launches made in front of k_taa, out[4] = histories handed over, out[5] = 1 while the scene holds a history.  Does not wait. */
#define MR_N_TAA_COUNTS 6
int mr_debug_taa(mr_scene *scene, int32_t *out);

/* Device times in milliseconds of the last frame with the pass: its k_velocity (with the per-face pair where that ran) and
 * its k_taa.  Waits for them.  MR_E_INVALID before the first such frame.  For a frame that ran both this pass and the
 * motion blur, mr_debug_motion_times reports a velocity span of 0: the one k_velocity is counted here. */
#define MR_N_TAA_TIMES 2
int mr_debug_taa_times(mr_scene *scene, float *out_ms);

/* Diagnostics: k_taa on buffers the caller supplies -- no frame is rendered.  Arrays as for mr_host_taa; shape is the
 * workgroup: 0 = 32 x 8 samples, 1 = 64 x 4, 2 = 16 x 16, 256 threads each (never MR_TAA_TILE's).  out_frame and
 * out_history receive the kernel's two outputs; on the device both lie between 256 bytes of sentinel either side, and
 * out_guard receives the number of those bytes that changed (0 unless the kernel wrote out of bounds).  The scene lends its
 * error text only: its frame slots, its history and what mr_debug_taa reports stay as they were.  Waits for the device.
 * MR_E_INVALID, before any device call, for a NULL argument (history may be NULL), a height or width outside 1 .. 32767, a
 * shape outside 0 .. 2 and a blend outside (0, 1] as float32. */
int mr_debug_taa_post(mr_scene *scene, const float *frame, const float *velocity, const float *history, int32_t height,
                      int32_t width, double blend, int32_t shape, float *out_frame, float *out_history, int32_t *out_guard);

/* Bloom: a glow round the samples brighter than a threshold, gathered from a resolution pyramid on the device.  It lives on
 * the frame's sample grid (Hs, Ws), rows bottom-up.  With F the float frame behind the motion blur and IN FRONT of the
 * overlay, t = threshold, g = gain, L = levels, float32 throughout, every operation rounded on its own, every weight dyadic:
 *
 *   bright pass   m = fmaxf(fmaxf(r, g), b);  k = m > t ? (m - t) / m : 0;  B0 = F * k                      per channel
 *   level sizes   H0, W0 = Hs, Ws;  H_l = (H_{l-1} + 1) / 2, W_l = (W_{l-1} + 1) / 2 (the ceiling; 1 x 1 halves to 1 x 1)
 *   down          D_0 = B0;  D_l[y][x] from D_{l-1} at the taps 2x-1 .. 2x+2 by 2y-1 .. 2y+2, coordinates clamped to the
 *                 source level; rows first, ascending: r_j = (a0 + a3) + 3*(a1 + a2); v = (r0 + r3) + 3*(r1 + r2);
 *                 D_l = v * (1/64)
 *   up            up(C) onto a finer grid: for a fine index i, near = i / 2, far = near - 1 (i even) or near + 1 (i odd),
 *                 clamped to the coarse level; per coarse row h = 3*C[near_x] + C[far_x]; v = 3*h[near_y] + h[far_y];
 *                 up = v * (1/16)
 *   up chain      U_L = D_L;  U_l = D_l + up(U_{l+1}), l = L-1 .. 1
 *   composite     out = F + g * up(U_1)
 *
 * Where no sample exceeds t every level is +0 and out == F bit for bit.  A uniform field stays uniform at every level.
 * Frame order: the lights' sum, k_ao, k_velocity, k_taa (whose history is written before this pass and never holds
 * glow), k_dof, k_mblur, the bloom's 2 L launches (L of k_bloom_down, the first with the bright pass; L - 1 of k_bloom_up;
 * k_bloom_composite), the overlay (drawn over the glow, not bloomed), the finalise of the result.  The pass keeps nothing
 * from frame to frame: it composes with accumulations, frames in flight (every frame slot owns a pyramid buffer of the
 * sum over l = 1 .. L of 3 H_l W_l floats) and every other pass.
 *
 * mr_scene_set_bloom copies the description during the call (NULL: off, the default); every frame enqueued afterwards uses
 * the copy of its moment and keeps its z-buffer, winner map and float frame (MR_FRAME_KEEP_BUFFERS | MR_FRAME_KEEP_FLOAT
 * are implied).  A scene without it enqueues what it always did.  MR_E_INVALID for a threshold that is not finite and
 * >= 0 as float32, a gain that is not finite and > 0 as float32, levels outside 1 .. 8; and, from the rendering entry
 * points, for a partial frame (row band, stripes), before any device work.  MR_E_UNSUPPORTED from a library linked without
 * bloom.hip or accum.hip. */
typedef struct mr_bloom_desc {
    double threshold;              /* t: >= 0 as float32 */
    double gain;                   /* g: > 0 as float32 */
    int32_t levels;                /* L: 1 .. 8 */
    int32_t pad;
} mr_bloom_desc;
int mr_scene_set_bloom(mr_scene *scene, const mr_bloom_desc *bloom);

/* Host arithmetic, no device needed: the definition above, bit for bit what the kernels write.  frame and out_frame are
 * (height, width, 3) float32.  out_pyramid may be NULL; else it receives D_1 .. D_L and then U_{L-1} .. U_1, packed in that
 * order, level l being (H_l, W_l, 3): 2 * (n_1 + .. + n_L) - n_L floats with n_l = 3 H_l W_l.  MR_E_INVALID for a NULL
 * argument, out_frame == frame, what mr_scene_set_bloom refuses, or a height or width outside 1 .. 32767. */
int mr_host_bloom(const float *frame, int32_t height, int32_t width, const mr_bloom_desc *bloom, float *out_frame, float *out_pyramid);

/* Diagnostics: out[0] = frames of this scene that enqueued the pass, out[1], out[2] = the sample rows and columns of the last
 * of them (0 before the first), out[3] = its levels (it made 2 * out[3] launches).  Does not wait. */
#define MR_N_BLOOM_COUNTS 4
int mr_debug_bloom(mr_scene *scene, int32_t *out);

/* Device times in milliseconds of the last frame with the pass: its down chain (L launches), its up chain (L - 1; the span
 * between two marks with nothing in it at L = 1) and its composite.  Waits for them.  MR_E_INVALID before the first such
 * frame. */
#define MR_N_BLOOM_TIMES 3
int mr_debug_bloom_times(mr_scene *scene, float *out_ms);

/* Diagnostics: the three kernels on a frame the caller supplies -- no frame is rendered.  Arrays as for mr_host_bloom; shape is
 * k_bloom_down's workgroup: 0 = 32 x 8 output samples, 1 = 64 x 4, 2 = 16 x 16, 256 threads each (never MR_BLOOM_TILE's).
 * On the device the frame and the pyramid lie between 256 bytes of sentinel either side: MR_E_DEVICE, with a text, when one
 * of those bytes changed.  The scene lends its error text only: its frame slots and what mr_debug_bloom reports stay as
 * they were, and the entry's device buffers are released when it returns.  Waits for the device.  MR_E_INVALID, before any
 * device call, for a NULL argument (out_pyramid may be NULL), a height or width outside 1 .. 32767, a shape outside 0 .. 2
 * and what mr_scene_set_bloom refuses. */
int mr_debug_bloom_post(mr_scene *scene, const float *frame, int32_t height, int32_t width, const mr_bloom_desc *bloom, int32_t shape,
                        float *out_frame, float *out_pyramid);

/* Light shafts: the sky's light streaming past occluders towards a light's place on the screen, marched on the device at a
 * half or a quarter of the output resolution.  It lives on the frame's sample grid (Hs, Ws), rows bottom-up.  With F the
 * float frame behind the motion blur and IN FRONT of the bloom and the overlay, Z the z-buffer, t = threshold, g = gain,
 * d = halvings (1 .. 4), n = samples, (lx, ly) the light on level d, float32 throughout, every operation rounded on its
 * own, no fma:
 *
 *   source       a sample is SKY when Z is not finite;  S_0 = F * k at a sky sample, k the bloom's bright factor
 *                (m = fmaxf(fmaxf(r, g), b);  k = m > t ? (m - t) / m : 0), +0 elsewhere
 *   level sizes  H_0, W_0 = Hs, Ws;  H_l = (H_{l-1} + 1) / 2, W_l = (W_{l-1} + 1) / 2
 *   reduction    B_0 = S_0;  B_{l+1}[y][x] = ((a00 + a01) + (a10 + a11)) * 0.25 over B_l at (2y, 2x), (2y, 2x+1), (2y+1, 2x),
 *                (2y+1, 2x+1), a sample outside the level counting +0;  S = B_d
 *   fetch        fetch(A, qx, qy), A of (H, W): for -0.5 <= qx <= W - 0.5 and -0.5 <= qy <= H - 0.5 (tested on the floats;
 *                a position outside fetches nothing and its tap contributes +0): qx clamped to [0, W - 1], x0 = (int)qx,
 *                x1 = min(x0 + 1, W - 1), fx = qx - (float)x0, likewise y; per channel h0 = a00 + fx*(a01 - a00),
 *                h1 = a10 + fx*(a11 - a10), v = h0 + fy*(h1 - h0)
 *   march        for the coarse sample (x, y), cx = (float)x, cy = (float)y: dx = (lx - cx) * step, dy = (ly - cy) * step;
 *                q_i = (cx + dx*(float)i, cy + dy*(float)i), i = 0 .. n-1;  R = sum_i weights[i] * fetch(S, q_i), summed in
 *                ascending i as acc = acc + w_i * v from +0
 *   composite    out = F + g * fetch(R, (x + 0.5) * 2^-d - 0.5, (y + 0.5) * 2^-d - 0.5)
 *
 * Where no sky sample exceeds t, S = R = +0 and out == F bit for bit.  Frame order: the lights' sum, k_ao, k_velocity,
 * k_taa (whose history never holds shafts), k_dof, k_mblur, k_shaft_source, k_shaft_march, k_shaft_composite, the bloom's
 * launches (a bright shaft may glow), the overlay (neither a source nor brightened), the finalise of the result.  The pass
 * keeps nothing from frame to frame: it composes with accumulations, frames in flight (every frame slot owns S and R, 16
 * bytes a sample each) and every other pass.
 *
 * mr_scene_set_light_shafts copies the description during the call (NULL: off, the default); every frame enqueued
 * afterwards uses the copy of its moment and keeps its z-buffer, winner map and float frame (MR_FRAME_KEEP_BUFFERS |
 * MR_FRAME_KEEP_FLOAT are implied).  A scene without it enqueues what it always did.  MR_E_INVALID for a light position,
 * threshold, gain or step that is not finite, a threshold < 0, a gain or step <= 0, samples outside 1 .. 128, halvings
 * outside 1 .. 4, one of the first `samples` weights not finite or < 0; and, from the rendering entry points, for a partial
 * frame (row band, stripes), before any device work.  MR_E_UNSUPPORTED from a library linked without shafts.hip or
 * accum.hip. */
typedef struct mr_light_shafts_desc {
    float light_x, light_y;        /* the light on level d: (screen x + 0.5) / 2^d - 0.5, likewise y */
    float threshold;               /* t: >= 0 */
    float gain;                    /* g: > 0 */
    float step;                    /* density / samples: > 0; 1 / samples reaches the light with tap n */
    int32_t samples;               /* n: 1 .. 128 */
    int32_t halvings;              /* d: 1 .. 4, the halvings of the sample grid (a supersampled grid's own included) */
    float weights[128];            /* w_i, i < n: finite and >= 0; the others are not read */
} mr_light_shafts_desc;
int mr_scene_set_light_shafts(mr_scene *scene, const mr_light_shafts_desc *shafts);

/* Host arithmetic, no device needed: the definition above, bit for bit what the kernels write.  frame and out_frame are
 * (height, width, 3) float32, zbuf (height, width) float64.  out_source and out_march may be NULL; else they receive S and R,
 * (H_d, W_d, 3) float32 each.  MR_E_INVALID for a NULL argument, out_frame == frame, what mr_scene_set_light_shafts
 * refuses, or a height or width outside 1 .. 32767. */
int mr_host_light_shafts(const float *frame, const double *zbuf, int32_t height, int32_t width, const mr_light_shafts_desc *shafts,
                         float *out_frame, float *out_source, float *out_march);

/* Diagnostics: out[0] = frames of this scene that enqueued the pass, out[1], out[2] = the sample rows and columns of the last
 * of them (0 before the first), out[3] = its halvings d.  Does not wait. */
#define MR_N_LIGHT_SHAFTS_COUNTS 4
int mr_debug_light_shafts(mr_scene *scene, int32_t *out);

/* Device times in milliseconds of the last frame with the pass: k_shaft_source, k_shaft_march, k_shaft_composite.  Waits
 * for them.  MR_E_INVALID before the first such frame. */
#define MR_N_LIGHT_SHAFTS_TIMES 3
int mr_debug_light_shafts_times(mr_scene *scene, float *out_ms);

/* Diagnostics: the three kernels on a frame and a z-buffer the caller supplies -- no frame is rendered.  Arrays as for
 * mr_host_light_shafts.  On the device the frame, the z-buffer, S and R each lie between 256 bytes of sentinel either side:
 * MR_E_DEVICE, with a text, when one of those bytes changed.  The scene lends its error text only: its frame slots and what
 * mr_debug_light_shafts reports stay as they were, and the entry's device buffers are released when it returns.  Waits for
 * the device.  MR_E_INVALID, before any device call, for a NULL argument (out_source and out_march may be NULL), a height or
 * width outside 1 .. 32767 and what mr_scene_set_light_shafts refuses. */
int mr_debug_light_shafts_post(mr_scene *scene, const float *frame, const double *zbuf, int32_t height, int32_t width,
                               const mr_light_shafts_desc *shafts, float *out_frame, float *out_source, float *out_march);

/* Tone mapping: an exposure metered from a luminance histogram of the frame, and a tone curve, on the device.  It lives on
 * the frame's sample grid, behind the bloom and IN FRONT of the overlay, whose lines keep their colours.  With F the float
 * frame there (F >= 0 and finite), all arithmetic float32 with every operation rounded on its own, or integer:
 *
 *   luminance   Y = (0.2126f*r + 0.7152f*g) + 0.0722f*b
 *   bin         b = clamp((bits(Y) >> 20) - ((127 - 24) << 3), 0, 255)     8 bins a stop over 32 stops from 2^-24
 *   histogram   n[i] = samples in bin i (uint32); n[0] (black) is metered out: n[0] := 0
 *   trim        N = sum n;  lo = N*low_pm / 1000;  hi = N*high_pm / 1000;  C_i = n[1] + .. + n[i-1];
 *               u_i = max(0, min(C_i + n[i], hi) - max(C_i, lo))
 *   centre      c_i = ((i >> 3) - 24) * 256 + FRAC[i & 7],  FRAC = {22, 63, 100, 134, 165, 193, 220, 244}     1/256 stops
 *   mean        S = sum u_i*c_i;  M = sum u_i (int64);  q = floor((2S + M) / (2M))
 *   target      -q = 256*a + f, 0 <= f < 256;  e_t = clamp(ldexpf(key * exp2[f], a), min_exposure, max_exposure)
 *   adapt       e = e_prev + speed * (e_t - e_prev) where the scene has a previous exposure, else e_t;
 *               M == 0 (nothing metered): e = e_prev, else 1.0f
 *   curve       x = F * e per channel;  linear: x;  reinhard: (x * (1 + x / (white*white))) / (1 + x);
 *               aces: min((x*(2.51f*x + 0.03f)) / (x*(2.43f*x + 0.59f) + 0.14f), 1)
 *
 * exp2[f] = float32(2^(f/256)) comes with the description, so that kernel, mirror and caller read the same bits.  With
 * `fixed` nothing is metered and e = float32(exposure).  Every count and sum is an integer: the result does not depend on
 * the order in which the device counts the samples.  Frame order: ... k_mblur, the light shafts, the bloom, k_lum_hist,
 * k_exposure, k_tone_apply (the last alone where the exposure is fixed), the overlay, the finalise of the result; k_taa's
 * history was written in front of the pass and never holds tone-mapped colours.
 *
 * A scene has a previous exposure only while it is ADAPTIVE (metered with speed < 1): then a frame's e becomes the scene's
 * previous exposure when that frame's mr_render or mr_render_wait returns MR_OK (a frame rendered again after an overflow
 * reads the same e_prev), one frame of the scene is in flight at a time (MR_E_INVALID from the rendering entry points while
 * an earlier one has not been waited for), and mr_render_device and the sub-frames of an accumulation refuse the scene.
 * mr_scene_set_tone_map (every call, NULL included) and mr_scene_reset_exposure forget the previous exposure.  Metered with
 * speed == 1, or fixed, the pass keeps nothing from frame to frame and composes with accumulations (sub-frames are tone-
 * mapped before they are summed), frames in flight (every frame slot owns its slab, histogram and exposure cell) and every
 * other pass.
 *
 * mr_scene_set_tone_map copies the description during the call (NULL: off, the default); every frame enqueued afterwards
 * uses the copy of its moment and keeps its z-buffer, winner map and float frame (MR_FRAME_KEEP_BUFFERS |
 * MR_FRAME_KEEP_FLOAT are implied).  A scene without it enqueues what it always did.  MR_E_INVALID for an operator outside
 * 0 .. 2, a fixed flag that is not 0 or 1, key, white, exposure, min_exposure or max_exposure not finite and > 0 as float32,
 * min_exposure > max_exposure, speed outside (0, 1] as float32, low_pm and high_pm not 0 <= low_pm < high_pm <= 1000, a
 * table with exp2[0] != 1, not strictly increasing or not < 2; and, from the rendering entry points, for a partial frame
 * (row band, stripes), before any device work.  MR_E_UNSUPPORTED from a library linked without tonemap.hip or accum.hip. */
#define MR_TONE_LINEAR 0
#define MR_TONE_REINHARD 1
#define MR_TONE_ACES 2
typedef struct mr_tone_map_desc {
    int32_t op;                    /* MR_TONE_* */
    int32_t fixed;                 /* 1: e = exposure, nothing is metered; 0: metered */
    double exposure;               /* > 0 as float32 (checked in either case) */
    double key;                    /* the luminance the metered mean is brought to: > 0 as float32 */
    double white;                  /* reinhard's white point: > 0 as float32 */
    double speed;                  /* in (0, 1] as float32; 1: no adaptation, no state */
    double min_exposure, max_exposure;
    int32_t low_pm, high_pm;       /* the trims in permille of the metered samples */
    float exp2[256];               /* float32(2^(f/256)) */
} mr_tone_map_desc;
int mr_scene_set_tone_map(mr_scene *scene, const mr_tone_map_desc *tone_map);

/* Forgets the scene's previous exposure: the next adaptive frame takes e = e_t, and a frame in flight hands nothing over. */
int mr_scene_reset_exposure(mr_scene *scene);

/* Host arithmetic, no device needed: the definition above, bit for bit what the kernels write.  frame and out_frame are
 * (height, width, 3) float32 (out_frame may be the frame); out_hist receives the 256 counts n (n[0] = 0; all 0 where the
 * exposure is fixed), out_exposure e.  has_prev != 0: e_prev is the scene's previous exposure.  out_hist and out_exposure may
 * be NULL.  MR_E_INVALID for a NULL argument, what mr_scene_set_tone_map refuses, a height or width outside 1 .. 32767, or
 * has_prev with an e_prev that is not finite and > 0. */
int mr_host_tone_map(const float *frame, int32_t height, int32_t width, const mr_tone_map_desc *tone_map, int32_t has_prev, float e_prev,
                     float *out_frame, uint32_t *out_hist, float *out_exposure);

/* The exposure e of the last frame enqueued, where it ran the pass (waits for it), and its 256 counts n.  MR_E_INVALID
 * where the last frame ran without the pass; the histogram also where that frame's exposure was fixed: nothing was metered. */
int mr_read_exposure(mr_scene *scene, float *out);
int mr_read_luminance_histogram(mr_scene *scene, uint32_t *out);

/* Diagnostics: out[0] = frames of this scene that enqueued the pass, out[1], out[2] = the sample rows and columns of the last
 * of them (0 before the first), out[3] = the workgroups of its k_lum_hist (0: fixed exposure, not metered), out[4] = exposures
 * handed over as the scene's previous one, out[5] = 1 while the scene holds a previous exposure.  Does not wait. */
#define MR_N_TONE_MAP_COUNTS 6
int mr_debug_tone_map(mr_scene *scene, int32_t *out);

/* Device times in milliseconds of the last frame with the pass: k_lum_hist, k_exposure (the spans between two marks with
 * nothing in them where the exposure is fixed), k_tone_apply.  Waits for them.  MR_E_INVALID before the first such frame. */
#define MR_N_TONE_MAP_TIMES 3
int mr_debug_tone_map_times(mr_scene *scene, float *out_ms);

/* Diagnostics: the kernels on a frame the caller supplies -- no frame is rendered.  Arrays as for mr_host_tone_map, none
 * may be NULL; out_exposure receives TWO floats, the exposure cell and the state cell a scene would adopt (both e; the fixed
 * exposure where nothing is metered).  grid_cap is the cap of k_lum_hist's grid: 0 for the library's default, else 1 ..
 * 1024 -- a small field then walks the stride loop, or fills many slab rows, or one; form is k_lum_hist's: 0 an LDS add a
 * sample, 1 an add per distinct bin of a wavefront, -1 the library's default.  On the device the frame, the block of
 * histogram, cell and slab, and the two state cells each lie between 256 bytes of sentinel either side, and the slab is
 * sentinel too before k_lum_hist writes it: MR_E_DEVICE, with a text, when a guard byte changed.  The scene lends its error
 * text only: its frame slots, its previous exposure and what mr_debug_tone_map reports stay as they were, and the entry's
 * device buffers are released when it returns.  Waits for the device.  MR_E_INVALID, before any device call, for a NULL
 * argument (but out_ms), a height or width outside 1 .. 32767, a grid_cap outside 0 .. 1024, a form outside -1 .. 1 and what
 * mr_host_tone_map refuses.  out_ms may be NULL; else it receives the device milliseconds of k_lum_hist, k_exposure and
 * k_tone_apply between events of the entry's own (the first two spans hold no kernel where the exposure is fixed). */
int mr_debug_tone_map_post(mr_scene *scene, const float *frame, int32_t height, int32_t width, const mr_tone_map_desc *tone_map,
                           int32_t has_prev, float e_prev, int32_t grid_cap, int32_t form, float *out_frame, uint32_t *out_hist,
                           float *out_exposure, float *out_ms);

/* Data layers: per-sample ids, barycentrics, depth, position, normals and texture coordinates of what a frame shows, on the
 * device, for callers who render frames as data (ground truth for depth, normals, segmentation, correspondence).  One
 * kernel, k_layers, right behind k_tile and in front of every post pass, from the winner map and the scene's static face
 * records alone: it reads no z-buffer and never touches the float frame, so the frame's bytes are what they are without
 * it.  csrc/layers_def.h states the definition; on the sample grid, rows bottom-up, for winner face w of sample (x, y):
 *
 *   bit  layer        type         w >= 0                                                          w < 0
 *   0    model        int32        the model that owns w (the last m with face_off[m] <= w)          -1
 *   1    face         int32        w - face_off[model]                                               -1
 *   2    material     int32        the face record's global material index                           -1
 *   3    barycentric  float32 x3   perspective-correct barycentrics lambda on the face's plane         0
 *   4    depth        float32      eye depth sum lambda_k E_k, > 0 in front of the camera            +inf
 *   5    position     float32 x3   world position sum lambda_k V_k                                     0
 *   6    face_normal  float32 x3   unit normal (V_1 - V_0) x (V_2 - V_0) of the world-space triangle   0
 *   7    normal       float32 x3   the vertex normals blended with lambda, normalised; the face        0
 *                                  normal where the face has none or the blend has no length
 *   8    uv           float32 x2   sum lambda_k uv_k; 0 where the face has no texture coordinates      0
 *
 * lambda comes from the adjugate of the corners' (x, y, w) under `s`, the 4 x 4 matrix of the description (row vectors,
 * row-major): columns 0, 1, 2 are x, y, w of view . projection . viewport on the sample grid as the frame is rendered (a
 * sub-sample offset included), column 3 maps a world point to its eye depth.  A sample whose lambda is not finite is
 * degenerate: it keeps its ids and takes the w < 0 column elsewhere.
 *
 * mr_scene_set_layers copies the description during the call (NULL: off, the default); every frame enqueued afterwards
 * computes the layers of `mask` into buffers its frame slot owns -- frames in flight keep their own -- and keeps its winner
 * map (MR_FRAME_KEEP_BUFFERS is implied).  A scene without it enqueues what it always did.  MR_E_INVALID for a mask that
 * is 0 or has a bit above 8, an entry of s that is not finite, an n_models that is not the number of the scene's models;
 * and, from the rendering entry points, for a partial frame (row band, stripes), for mr_render_device and for the
 * sub-frames of an accumulation, before any device work.  MR_E_UNSUPPORTED from a library linked without layers.hip. */
#define MR_N_LAYERS 9
typedef struct mr_layers_desc {
    double s[16];
    int32_t mask;                  /* bit i: layer i */
    int32_t n_models;              /* the scene's models (mr_scene_set_layers), or the entries of face_off (the host mirror) */
} mr_layers_desc;
int mr_scene_set_layers(mr_scene *scene, const mr_layers_desc *layers);

/* Layer `layer` (0 .. 8) of the last frame enqueued, which computed it: height x width samples of 1, 2 or 3 32-bit words as
 * in the table.  Waits for the device.  MR_E_INVALID where that frame ran without the pass or without this layer. */
int mr_read_layers(mr_scene *scene, int32_t layer, void *out);

/* Host arithmetic, no device needed: the definition above, bit for bit what k_layers writes.  winner is (height, width)
 * int32; face_pos holds n_faces records of 64 bytes (pos32 != 0: float32 corners [3][4], int32 material, uint32 flags, 8
 * bytes of padding) or 112 bytes (float64 corners likewise); face_attr n_faces records of 16 float32 (uv [3][2], normals
 * [3][3], one of padding); face_off the n_models first faces, ascending from 0.  out[i] receives layer i where the mask
 * names it and is not read otherwise; out_degenerate, unless NULL, the number of degenerate samples.  MR_E_INVALID for a
 * NULL argument, what mr_scene_set_layers refuses of the description, a height or width outside 1 .. 32767, first faces
 * that do not ascend from 0 to at most n_faces, or a winner >= n_faces. */
int mr_host_layers(const int32_t *winner, int32_t height, int32_t width, const void *face_pos, int32_t pos32, const float *face_attr,
                   int32_t n_faces, const int32_t *face_off, const mr_layers_desc *layers, void *const *out, int64_t *out_degenerate);

/* Diagnostics: out[0] = frames of this scene that enqueued the pass, out[1], out[2] = the sample rows and columns of the last
 * of them (0 before the first), out[3] = its mask.  Does not wait. */
#define MR_N_LAYERS_COUNTS 4
int mr_debug_layers(mr_scene *scene, int32_t *out);

/* Device time in milliseconds of the last frame's k_layers.  Waits for it.  MR_E_INVALID before the first such frame. */
int mr_debug_layers_times(mr_scene *scene, float *out_ms);

/* Diagnostics: k_layers on arrays the caller supplies -- no frame is rendered.  Arguments as for mr_host_layers; EVERY out[i]
 * must be given, named by the mask or not.  On the device every layer's buffer lies between 256 bytes of sentinel either
 * side and is filled with the sentinel byte 0xa5 before the kernel runs, so a layer the mask does not name comes back as
 * sentinel; out_guard receives the number of guard bytes that changed.  The scene lends its error text only, and the
 * entry's device buffers are released when it returns.  Waits for the device.  out_ms, unless NULL, receives the kernel's
 * device milliseconds between events of the entry's own. */
int mr_debug_layers_post(mr_scene *scene, const int32_t *winner, int32_t height, int32_t width, const void *face_pos, int32_t pos32,
                         const float *face_attr, int32_t n_faces, const int32_t *face_off, const mr_layers_desc *layers, void *const *out,
                         int32_t *out_guard, float *out_ms);

/* Diagnostics: the scene's static face records as the device holds them now, after the last commit and pose pass -- what
 * k_layers and the shading read.  out_info receives { number of faces, pos32 }; out_pos (faces x 64 or 112 bytes) and
 * out_attr (faces x 64 bytes) may both be NULL to ask for out_info alone.  Waits for the device.  MR_E_INVALID for a scene
 * that has uncommitted changes (render a frame first). */
int mr_debug_read_face_records(mr_scene *scene, void *out_pos, void *out_attr, int32_t *out_info);

/* Diagnostics: the scene's per-cluster records as the set-up kernel reads them, one per 64 consecutive faces, 16 32-bit
 * words each: float32 lo[3], hi[3] (the faces' bounding box, rounded outwards; NaN = no box), float32 axis[3] (the unit
 * axis of the cone the faces' unit normals lie in), float32 cos_half, sin_half (every normal n has n . axis >= cos_half;
 * cos_half < -1 = no cone), 5 pad words.  Copies at most cap_clusters records; returns the number of clusters of the
 * last commit or a negative error.  Synchronises the device. */
int mr_debug_read_clusters(mr_scene *scene, void *out, int32_t cap_clusters);

/* Human-readable description of the last error on this thread ("" if none). */
const char *mr_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MI355RAST_H */
