"""ctypes binding of ``libmi355rast.so`` (C ABI: ``include/mi355rast.h``).

``DeviceRenderer`` is what ``Scene.render`` talks to: it mirrors the scene into the
library (re-uploading only when a model or texture changed), fills the per-frame constant
block and calls ``mr_render``.  There is no CPU fallback: if the library is missing or no
GPU is visible the calls raise ``RuntimeError``.
"""
import ctypes as C
import os
import zlib

import numpy as np

from ._pack import active_morph, active_skin, ao_constants, auto_normals_active, bloom_constants, dof_constants, layer_mask, layer_matrix, light_shafts_constants, morph_csr, motion_matrices, motion_vertices, normal_owners, pack_frame, pack_model, pose_normal_matrix, sample_grid, taa_jitter, tone_map_constants

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libmi355rast.so"
LIB_PATH = os.path.join(_HERE, LIB_NAME)

MR_OK = 0
MR_E_INVALID = -1
MR_E_OVERFLOW = -4
FRAME_SHADOWS, FRAME_KEEP_FLOAT, FRAME_FACE_STATUS, FRAME_LIGHT_TIMING, FRAME_SKYBOX, FRAME_COUNTERS = 1, 2, 4, 8, 16, 32
FRAME_KEEP_BUFFERS = 64
FRAME_NO_TIMING = 128
FRAME_OVERLAY = 256
FRAME_SUPERSAMPLE2, FRAME_SUPERSAMPLE4 = 512, 1024
_SUPERSAMPLE_FLAGS = {1: 0, 2: FRAME_SUPERSAMPLE2, 4: FRAME_SUPERSAMPLE4}
ABI_VERSION = 4
MAX_LIGHTS = 4
TILE_RECORD_WORDS = 12


class FrameDesc(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("system", C.c_int32),
                ("backface_culling", C.c_int32), ("light_type", C.c_int32), ("flags", C.c_int32),
                ("row_begin", C.c_int32), ("row_end", C.c_int32),
                ("stripe_count", C.c_int32), ("stripe_index", C.c_int32),
                ("mvp", C.c_double * 16), ("viewport", C.c_double * 16), ("debug_mvp", C.c_double * 16),
                ("frustum_planes", C.c_double * 24), ("z_near", C.c_double), ("z_far", C.c_double),
                ("camera_pos", C.c_double * 3), ("light_pos", C.c_double * 3), ("light_dir", C.c_double * 3),
                ("light_color", C.c_double * 3), ("light_ambient", C.c_double * 3),
                ("specular_strength", C.c_double), ("att_constant", C.c_double), ("att_linear", C.c_double),
                ("att_quadratic", C.c_double), ("spot_edge0", C.c_double), ("spot_edge1", C.c_double),
                ("background", C.c_float * 3), ("background_u8", C.c_uint32),
                ("sky_tri", C.c_int32 * 12), ("sky_rays", C.c_double * 18)]


class LightDesc(C.Structure):
    _fields_ = [("type", C.c_int32), ("pad", C.c_int32),
                ("pos", C.c_double * 3), ("dir", C.c_double * 3), ("color", C.c_double * 3), ("ambient", C.c_double * 3),
                ("specular_strength", C.c_double), ("att_constant", C.c_double), ("att_linear", C.c_double),
                ("att_quadratic", C.c_double), ("spot_edge0", C.c_double), ("spot_edge1", C.c_double)]


def fill_light_desc(pl):
    """``mr_light_desc`` of a ``_pack.PackedLight``."""
    d = LightDesc()
    d.type = int(pl.light_type)
    for name, src in (("pos", pl.light_pos), ("dir", pl.light_dir), ("color", pl.light_color), ("ambient", pl.light_ambient)):
        for i in range(3):
            getattr(d, name)[i] = float(src[i])
    d.specular_strength = pl.specular_strength
    d.att_constant, d.att_linear, d.att_quadratic = pl.att_constant, pl.att_linear, pl.att_quadratic
    d.spot_edge0, d.spot_edge1 = pl.spot_edge0, pl.spot_edge1
    return d


class MaterialDesc(C.Structure):
    _fields_ = [("kd", C.c_double * 3), ("ks255", C.c_double * 3), ("ns", C.c_double),
                ("tex_kd", C.c_int32), ("tex_norm", C.c_int32), ("tex_ks", C.c_int32),
                ("norm_tangent", C.c_int32)]


class ModelDesc(C.Structure):
    _fields_ = [("vertices", C.c_void_p), ("uv", C.c_void_p), ("normals", C.c_void_p), ("faces", C.c_void_p),
                ("materials", C.POINTER(MaterialDesc)), ("edge_ids", C.c_void_p),
                ("n_vertices", C.c_int32), ("n_uv", C.c_int32), ("n_normals", C.c_int32),
                ("n_faces", C.c_int32), ("n_materials", C.c_int32),
                ("vertices_are_f32", C.c_int32), ("clip", C.c_int32), ("depth_test", C.c_int32)]


class OverlayDesc(C.Structure):
    _fields_ = [("n_segments", C.c_int32), ("n_points", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("seg_first", C.c_void_p), ("seg_count", C.c_void_p), ("target", C.c_void_p), ("z", C.c_void_p)]


class AoDesc(C.Structure):
    _fields_ = [("depth_map", C.c_double * 4), ("k", C.c_double), ("radius", C.c_double), ("strength", C.c_double),
                ("depth_range", C.c_double), ("bias", C.c_double), ("perspective", C.c_int32), ("pad", C.c_int32)]


def fill_ao_desc(ao, depth_map, k, perspective):
    """``mr_ao_desc`` of an ``AmbientOcclusion`` (or anything with its four attributes) and a view's constants
    (``_pack.ao_constants``)."""
    d = AoDesc()
    for i in range(4):
        d.depth_map[i] = float(depth_map[i])
    d.k, d.perspective = float(k), int(perspective)
    d.radius, d.strength, d.depth_range, d.bias = float(ao.radius), float(ao.strength), float(ao.depth_range), float(ao.bias)
    return d


class DofDesc(C.Structure):
    _fields_ = [("depth_map", C.c_double * 4), ("kf", C.c_double), ("focus", C.c_double), ("perspective", C.c_int32),
                ("pad", C.c_int32)]


def fill_dof_desc(depth_map, kf, perspective, focus):
    """``mr_dof_desc`` of a view's constants (``_pack.dof_constants``)."""
    d = DofDesc()
    for i in range(4):
        d.depth_map[i] = float(depth_map[i])
    d.kf, d.focus, d.perspective = float(kf), float(focus), int(perspective)
    return d


class BloomDesc(C.Structure):
    _fields_ = [("threshold", C.c_double), ("gain", C.c_double), ("levels", C.c_int32), ("pad", C.c_int32)]


def fill_bloom_desc(threshold, gain, levels):
    """``mr_bloom_desc`` of a frame's constants (``_pack.bloom_constants``)."""
    d = BloomDesc()
    d.threshold, d.gain, d.levels = float(threshold), float(gain), int(levels)
    return d


class LightShaftsDesc(C.Structure):
    _fields_ = [("light_x", C.c_float), ("light_y", C.c_float), ("threshold", C.c_float), ("gain", C.c_float), ("step", C.c_float),
                ("samples", C.c_int32), ("halvings", C.c_int32), ("weights", C.c_float * 128)]


def fill_light_shafts_desc(light_x, light_y, threshold, gain, step, samples, levels, weights):
    """``mr_light_shafts_desc`` of a frame's constants (``_pack.light_shafts_constants``); *levels* is the library's
    ``halvings``, those of a supersampled grid included.  At most the first 128 of *weights* are taken."""
    d = LightShaftsDesc()
    d.light_x, d.light_y, d.threshold, d.gain, d.step = (float(v) for v in (light_x, light_y, threshold, gain, step))
    d.samples, d.halvings = int(samples), int(levels)
    for i, w in enumerate(np.asarray(weights, dtype=np.float32).ravel()[:128]):
        d.weights[i] = float(w)
    return d


class ToneMapDesc(C.Structure):
    _fields_ = [("op", C.c_int32), ("fixed", C.c_int32), ("exposure", C.c_double), ("key", C.c_double), ("white", C.c_double),
                ("speed", C.c_double), ("min_exposure", C.c_double), ("max_exposure", C.c_double), ("low_pm", C.c_int32),
                ("high_pm", C.c_int32), ("exp2", C.c_float * 256)]


def fill_tone_map_desc(op, fixed, exposure, key, white, speed, min_exposure, max_exposure, low_pm, high_pm, table):
    """``mr_tone_map_desc`` of a frame's constants (``_pack.tone_map_constants``); *table* is ``EXP2``, 256 float32."""
    d = ToneMapDesc()
    d.op, d.fixed, d.low_pm, d.high_pm = int(op), int(fixed), int(low_pm), int(high_pm)
    d.exposure, d.key, d.white, d.speed, d.min_exposure, d.max_exposure = (float(v) for v in (exposure, key, white, speed, min_exposure, max_exposure))
    table = np.ascontiguousarray(table, dtype=np.float32).ravel()
    if table.size != 256:
        raise ValueError(f"the exp2 table has 256 entries, got {table.size}")
    C.memmove(d.exp2, table.ctypes.data, 1024)
    return d


class LayersDesc(C.Structure):
    _fields_ = [("s", C.c_double * 16), ("mask", C.c_int32), ("n_models", C.c_int32)]


def fill_layers_desc(S, mask, n_models):
    """``mr_layers_desc``: *S* float64 ``(4, 4)`` (``_pack.layer_matrix``), the layers' bit mask and the number of models."""
    S = np.ascontiguousarray(S, dtype=np.float64)
    if S.shape != (4, 4):
        raise ValueError(f"S must be (4, 4), got {S.shape}")
    d = LayersDesc()
    C.memmove(d.s, S.ctypes.data, 128)
    d.mask, d.n_models = int(mask), int(n_models)
    return d


class MotionDesc(C.Structure):
    _fields_ = [("depth_map", C.c_double * 4), ("shutter", C.c_double), ("matrices", C.c_void_p), ("background", C.c_double * 9),
                ("class_of_model", C.c_void_p), ("n_classes", C.c_int32), ("n_models", C.c_int32)]


def fill_motion_desc(depth_map, shutter, matrices, background, class_of_model):
    """``mr_motion_desc`` of a frame's motion (``_pack.motion_matrices``): *matrices* ``(n_classes, 4, 3)``, *background*
    ``(3, 3)``, *class_of_model* ``(n_models,)``.  The description points into float64 / int32 copies of the arrays, which it
    keeps alive (``_arrays``); the library copies everything during the call it is handed to."""
    matrices = np.ascontiguousarray(matrices, dtype=np.float64).reshape(-1, 4, 3)
    background = np.ascontiguousarray(background, dtype=np.float64).reshape(3, 3)
    class_of_model = np.ascontiguousarray(class_of_model, dtype=np.int32).ravel()
    d = MotionDesc()
    for i in range(4):
        d.depth_map[i] = float(depth_map[i])
    for i in range(9):
        d.background[i] = float(background.flat[i])
    d.shutter = float(shutter)
    d.matrices = matrices.ctypes.data
    d.class_of_model = class_of_model.ctypes.data if len(class_of_model) else None
    d.n_classes, d.n_models = len(matrices), len(class_of_model)
    d._arrays = (matrices, class_of_model)
    return d


class TaaDesc(C.Structure):
    _fields_ = [("blend", C.c_double), ("matrices", C.c_void_p), ("background", C.c_double * 9), ("class_of_model", C.c_void_p),
                ("n_classes", C.c_int32), ("n_models", C.c_int32)]


def fill_taa_desc(blend, matrices, background, class_of_model):
    """``mr_taa_desc``: *blend* and the velocity's tables as ``fill_motion_desc`` takes them (``_pack.motion_matrices``).  The
    description keeps its copies of the arrays alive (``_arrays``); the library copies everything during the call it is
    handed to."""
    matrices = np.ascontiguousarray(matrices, dtype=np.float64).reshape(-1, 4, 3)
    background = np.ascontiguousarray(background, dtype=np.float64).reshape(3, 3)
    class_of_model = np.ascontiguousarray(class_of_model, dtype=np.int32).ravel()
    d = TaaDesc()
    d.blend = float(blend)
    for i in range(9):
        d.background[i] = float(background.flat[i])
    d.matrices = matrices.ctypes.data
    d.class_of_model = class_of_model.ctypes.data if len(class_of_model) else None
    d.n_classes, d.n_models = len(matrices), len(class_of_model)
    d._arrays = (matrices, class_of_model)
    return d


class MotionFacesDesc(C.Structure):
    _fields_ = [("s_now", C.c_double * 12), ("s_prev", C.c_double * 12), ("deforming", C.c_void_p), ("n_models", C.c_int32),
                ("prev_serial", C.c_int64)]


def fill_motion_faces_desc(s_now, s_prev, deforming, prev_serial):
    """``mr_motion_faces_desc`` of a frame (``_pack.motion_vertices``): *s_now*, *s_prev* ``(4, 3)``, *deforming*
    ``(n_models,)``.  The description keeps its int32 copy of the flags alive (``_arrays``); the library copies everything
    during the call it is handed to."""
    s_now = np.ascontiguousarray(s_now, dtype=np.float64).reshape(12)
    s_prev = np.ascontiguousarray(s_prev, dtype=np.float64).reshape(12)
    deforming = np.ascontiguousarray(deforming, dtype=np.int32).ravel()
    d = MotionFacesDesc()
    for i in range(12):
        d.s_now[i], d.s_prev[i] = float(s_now[i]), float(s_prev[i])
    d.deforming = deforming.ctypes.data if len(deforming) else None
    d.n_models, d.prev_serial = len(deforming), int(prev_serial)
    d._arrays = (deforming,)
    return d


class Stats(C.Structure):
    _fields_ = ([(n, C.c_int64) for n in (
        "frag_tri", "frag_quad", "covered_px", "lit_px", "stencil_updates", "n_faces", "n_faces_setup",
        "n_quads", "n_quads_drawn", "tri_bin_entries", "quad_bin_entries")] +
        [(n, C.c_float) for n in ("gpu_ms_total", "gpu_ms_setup", "gpu_ms_binning", "gpu_ms_tile", "gpu_ms_copy")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# every symbol include/mi355rast.h declares: (restype, argtypes)
_PROTOTYPES = {
    "mr_init": (C.c_int, [C.c_int]),
    "mr_device_available": (C.c_int, []),
    "mr_abi_version": (C.c_int, []),
    "mr_abi_struct_size": (C.c_int, [C.c_int]),
    "mr_scene_create": (C.c_void_p, []),
    "mr_scene_destroy": (None, [C.c_void_p]),
    "mr_scene_add_texture": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "mr_scene_set_skybox": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "mr_scene_add_model": (C.c_int, [C.c_void_p, C.POINTER(ModelDesc)]),
    "mr_scene_clear": (C.c_int, [C.c_void_p]),
    "mr_scene_set_overlay": (C.c_int, [C.c_void_p, C.POINTER(OverlayDesc)]),
    "mr_scene_set_overlay_cameras": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double,
                                               C.c_int32, C.c_int32, C.c_int32]),
    "mr_scene_set_list_capacities": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "mr_scene_set_extra_lights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "mr_read_stencil_light": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "mr_read_silhouette_light": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    "mr_render": (C.c_int, [C.c_void_p, C.POINTER(FrameDesc), C.c_void_p, C.POINTER(Stats)]),
    "mr_overlay_state_bytes": (C.c_int64, [C.c_void_p]),
    "mr_overlay_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "mr_render_async": (C.c_int, [C.c_void_p, C.POINTER(FrameDesc), C.c_void_p, C.c_int32]),
    "mr_render_wait": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(Stats)]),
    "mr_host_alloc": (C.c_void_p, [C.c_uint64]),
    "mr_host_free": (None, [C.c_void_p]),
    "mr_render_device": (C.c_int, [C.c_void_p, C.POINTER(FrameDesc), C.c_void_p, C.c_void_p]),
    "mr_get_stats": (C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    "mr_get_kernel_times": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_int]),
    "mr_get_stream_kernel_times": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_int]),
    "mr_read_z": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_read_stencil": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_read_winner": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_read_frame_f32": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_read_face_status": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_read_silhouette": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "mr_host_matmul_chain": (None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "mr_host_overlay_build": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int32,
                                        C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mr_host_overlay_fetch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mr_debug_read_tile_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "mr_debug_clusters_culled": (C.c_int, [C.c_void_p]),
    "mr_debug_quad_walks": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_debug_pair_log": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_debug_big_tri_rejects": (C.c_int, [C.c_void_p]),
    "mr_host_camera_constants": (None, [C.c_void_p] * 5 + [C.c_int32] + [C.c_void_p] * 3),
    "mr_debug_read_tile_order": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "mr_debug_sil_cache": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_debug_force_full": (C.c_int, [C.c_void_p, C.c_int32]),
    "mr_debug_frame_path": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_scene_set_model_pose": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "mr_scene_set_model_pose_normals": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "mr_debug_pose_normals_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mr_debug_pose": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_debug_pose_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mr_debug_read_clusters": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "mr_scene_set_model_skin": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "mr_scene_set_model_bones": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    "mr_host_skin_chain": (None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "mr_host_skin_chain3": (None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "mr_debug_skin": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_debug_skin_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mr_scene_set_model_morph": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 6),
    "mr_scene_set_model_morph_weights": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    "mr_host_morph_chain": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 5),
    "mr_debug_morph": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_debug_morph_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mr_scene_set_model_auto_normals": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "mr_host_auto_normals": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "mr_debug_auto_normals": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_debug_auto_normals_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mr_accum_begin": (C.c_int, [C.c_void_p]),
    "mr_accum_add": (C.c_int, [C.c_void_p, C.POINTER(FrameDesc), C.c_double]),
    "mr_accum_resolve": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p]),
    "mr_accum_read_f32": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_debug_accum": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_debug_accum_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mr_host_accum": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p]),
    "mr_scene_set_ambient_occlusion": (C.c_int, [C.c_void_p, C.POINTER(AoDesc)]),
    "mr_host_ao": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(AoDesc), C.c_void_p]),
    "mr_debug_ao": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_debug_ao_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mr_scene_set_depth_of_field": (C.c_int, [C.c_void_p, C.POINTER(DofDesc)]),
    "mr_host_dof": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(DofDesc), C.c_void_p]),
    "mr_debug_dof": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_debug_dof_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mr_debug_post": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(AoDesc), C.c_int32,
                                C.POINTER(DofDesc), C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p]),
    "mr_scene_set_motion_blur": (C.c_int, [C.c_void_p, C.POINTER(MotionDesc)]),
    "mr_host_velocity": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(MotionDesc), C.c_void_p]),
    "mr_host_motion_blur": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(MotionDesc), C.c_void_p]),
    "mr_read_velocity": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_debug_motion": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_debug_motion_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mr_debug_motion_post": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                       C.POINTER(MotionDesc), C.c_int32, C.c_void_p, C.c_void_p]),
    "mr_scene_set_motion_faces": (C.c_int, [C.c_void_p, C.POINTER(MotionFacesDesc)]),
    "mr_scene_track_vertices": (C.c_int, [C.c_void_p, C.c_int32]),
    "mr_scene_vertices_serial": (C.c_int64, [C.c_void_p]),
    "mr_host_face_homographies": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mr_host_velocity_faces": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_void_p]),
    "mr_debug_motion_faces_post": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                             C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "mr_debug_read_prev_vertices": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_debug_motion_faces": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_debug_motion_faces_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mr_scene_set_temporal_aa": (C.c_int, [C.c_void_p, C.POINTER(TaaDesc)]),
    "mr_scene_reset_history": (C.c_int, [C.c_void_p]),
    "mr_read_history": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_host_taa": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_void_p]),
    "mr_debug_taa": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_debug_taa_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mr_debug_taa_post": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_int32,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "mr_scene_set_bloom": (C.c_int, [C.c_void_p, C.POINTER(BloomDesc)]),
    "mr_host_bloom": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(BloomDesc), C.c_void_p, C.c_void_p]),
    "mr_debug_bloom": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_debug_bloom_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mr_debug_bloom_post": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(BloomDesc), C.c_int32, C.c_void_p, C.c_void_p]),
    "mr_scene_set_light_shafts": (C.c_int, [C.c_void_p, C.POINTER(LightShaftsDesc)]),
    "mr_host_light_shafts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(LightShaftsDesc), C.c_void_p, C.c_void_p, C.c_void_p]),
    "mr_debug_light_shafts": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_debug_light_shafts_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mr_debug_light_shafts_post": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(LightShaftsDesc), C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "mr_scene_set_tone_map": (C.c_int, [C.c_void_p, C.POINTER(ToneMapDesc)]),
    "mr_scene_reset_exposure": (C.c_int, [C.c_void_p]),
    "mr_host_tone_map": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(ToneMapDesc), C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mr_read_exposure": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_read_luminance_histogram": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_debug_tone_map": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_debug_tone_map_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mr_debug_tone_map_post": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(ToneMapDesc), C.c_int32, C.c_float, C.c_int32, C.c_int32,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mr_scene_set_layers": (C.c_int, [C.c_void_p, C.POINTER(LayersDesc)]),
    "mr_read_layers": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "mr_host_layers": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(LayersDesc),
                                  C.c_void_p, C.c_void_p]),
    "mr_debug_layers": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mr_debug_layers_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "mr_debug_layers_post": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                        C.POINTER(LayersDesc), C.c_void_p, C.c_void_p, C.c_void_p]),
    "mr_debug_read_face_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mr_last_error": (C.c_char_p, []),
}
EXPORTED_SYMBOLS = tuple(_PROTOTYPES)

_lib = None


def _prefer_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm ships its own ``libamdhip64.so``; ``multigpu.py`` hands
    torch's streams and tensors to this library, so both must run on the same copy.  Whichever copy is
    loaded first serves both (same SONAME) -- but a torch imported AFTER the system copy finds no
    device.  So when torch is installed its copy is loaded first, without importing torch itself."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(path):
            C.CDLL(path, mode=C.RTLD_GLOBAL)
    except (OSError, ImportError, ValueError):
        pass                                    # no torch, or not a ROCm build: the system runtime serves


def load_library():
    """Load the HIP library; raises RuntimeError (never falls back) when it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                               "g.build()'` (hipcc --offload-arch=gfx950); there is no CPU fallback")
        _prefer_torch_hip_runtime()
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOTYPES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        if lib.mr_abi_version() != ABI_VERSION:
            raise RuntimeError(f"{LIB_NAME}: ABI version {lib.mr_abi_version()}, this binding speaks {ABI_VERSION}; rebuild")
        for which, struct in enumerate((FrameDesc, MaterialDesc, ModelDesc, Stats, OverlayDesc, LightDesc, AoDesc)):
            if lib.mr_abi_struct_size(which) != C.sizeof(struct):
                raise RuntimeError(f"{LIB_NAME}: layout of {struct.__name__} differs from the binding "
                                   f"({lib.mr_abi_struct_size(which)} vs {C.sizeof(struct)} bytes); rebuild")
        _lib = lib
    return _lib


def _check(rc, what):
    if rc < 0:
        msg = load_library().mr_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed ({rc}): {msg}")
    return rc


def _check_accum(rc, what):
    """``_check`` for the accumulation's calls: what the library refuses as an argument (``MR_E_INVALID``) is a
    ``ValueError`` with its text, everything else a ``RuntimeError``."""
    if rc == MR_E_INVALID:
        raise ValueError(f"{what}: " + load_library().mr_last_error().decode(errors="replace"))
    return _check(rc, what)


def host_accum(frames, weights, shift=0, scale=1.0, want_acc=True, want_rgb=True):
    """``mr_host_accum``: the accumulation's definition on the host, no device.  *frames* is ``(n, Hs, Ws, 3)`` float32
    (a sequence of ``(Hs, Ws, 3)`` frames will do), *weights* ``(n,)``; returns ``(A, bytes)`` -- float32 ``(Hs, Ws, 3)``
    and uint8 ``(Hs >> shift, Ws >> shift, 3)``, ``None`` for the one not asked for.  ``ValueError`` with the library's
    text for what it refuses."""
    frames = np.ascontiguousarray(frames, dtype=np.float32)
    weights = np.ascontiguousarray(weights, dtype=np.float64).ravel()
    if frames.ndim != 4 or frames.shape[3] != 3 or frames.shape[0] != len(weights):
        raise ValueError(f"frames must be (n, H, W, 3) with one weight each, got {frames.shape} and {len(weights)} weights")
    n, h, w, _ = frames.shape
    shift = int(shift)
    acc = np.empty((h, w, 3), dtype=np.float32) if want_acc else None
    rgb = np.empty((h >> shift, w >> shift, 3), dtype=np.uint8) if want_rgb and 0 <= shift <= 2 else None
    ptr = lambda a: None if a is None else a.ctypes.data
    _check_accum(load_library().mr_host_accum(frames.ctypes.data, weights.ctypes.data, n, h, w, shift, float(scale), ptr(acc),
                                              ptr(rgb)), "mr_host_accum")
    return acc, rgb


def host_ao(z, frame, desc):
    """``mr_host_ao``: the ambient obscurance's definition on the host, no device.  *z* is ``(Hs, Ws)`` float64, *frame*
    ``(Hs, Ws, 3)`` float32, *desc* an ``AoDesc``; returns the darkened frame, float32 ``(Hs, Ws, 3)``.  ``ValueError``
    with the library's text for what it refuses."""
    z = np.ascontiguousarray(z, dtype=np.float64)
    frame = np.ascontiguousarray(frame, dtype=np.float32)
    if z.ndim != 2 or frame.shape != z.shape + (3,):
        raise ValueError(f"z must be (H, W) and frame (H, W, 3), got {z.shape} and {frame.shape}")
    out = np.empty_like(frame)
    _check_accum(load_library().mr_host_ao(z.ctypes.data, frame.ctypes.data, z.shape[0], z.shape[1], C.byref(desc), out.ctypes.data),
                 "mr_host_ao")
    return out


def host_dof(z, frame, desc):
    """``mr_host_dof``: the depth of field's definition on the host, no device.  *z* is ``(Hs, Ws)`` float64, *frame*
    ``(Hs, Ws, 3)`` float32, *desc* a ``DofDesc``; returns the blurred frame, float32 ``(Hs, Ws, 3)``.  ``ValueError``
    with the library's text for what it refuses."""
    z = np.ascontiguousarray(z, dtype=np.float64)
    frame = np.ascontiguousarray(frame, dtype=np.float32)
    if z.ndim != 2 or frame.shape != z.shape + (3,):
        raise ValueError(f"z must be (H, W) and frame (H, W, 3), got {z.shape} and {frame.shape}")
    out = np.empty_like(frame)
    _check_accum(load_library().mr_host_dof(z.ctypes.data, frame.ctypes.data, z.shape[0], z.shape[1], C.byref(desc), out.ctypes.data),
                 "mr_host_dof")
    return out


def debug_post(handle, frames, z, ao=None, ao_shape=0, dof=None, dof_shape=0, weights=None, shift=0, scale=1.0, want_rgb=True):
    """``mr_debug_post``: k_ao, k_dof, k_accum_add and k_accum_resolve on the caller's arrays, no frame rendered.  *handle*
    is a scene handle (``mr_scene_create``, or a ``DeviceRenderer``'s), *frames* ``(n, Hs, Ws, 3)`` float32 (one ``(Hs, Ws,
    3)`` frame will do), *z* ``(Hs, Ws)`` float64, *ao* an ``AoDesc`` or None, *dof* a ``DofDesc`` or None, the shapes 0 .. 2,
    *weights* ``(n,)`` or None.  Returns ``(float32 (Hs, Ws, 3), uint8 (Hs >> shift, Ws >> shift, 3) or None)``.
    ``ValueError`` with the library's text for what it refuses."""
    frames = np.ascontiguousarray(frames, dtype=np.float32)
    if frames.ndim == 3:
        frames = frames[None]
    z = np.ascontiguousarray(z, dtype=np.float64)
    if frames.ndim != 4 or frames.shape[3] != 3 or z.shape != frames.shape[1:3]:
        raise ValueError(f"frames must be (n, H, W, 3) and z (H, W), got {frames.shape} and {z.shape}")
    n, h, w, _ = frames.shape
    if weights is not None:
        weights = np.ascontiguousarray(weights, dtype=np.float64).ravel()
        if len(weights) != n:
            raise ValueError(f"{n} frames and {len(weights)} weights")
    shift = int(shift)
    out = np.empty((h, w, 3), dtype=np.float32)
    rgb = np.empty((h >> shift, w >> shift, 3), dtype=np.uint8) if want_rgb and 0 <= shift <= 2 else None
    ptr = lambda a: None if a is None else a.ctypes.data
    ref = lambda d: None if d is None else C.byref(d)
    _check_accum(load_library().mr_debug_post(handle, frames.ctypes.data, z.ctypes.data, n, h, w, ref(ao), int(ao_shape), ref(dof),
                                              int(dof_shape), ptr(weights), shift, float(scale), out.ctypes.data, ptr(rgb)),
                 "mr_debug_post")
    return out, rgb


def _motion_arrays(z, winner, frame, face_off, desc):
    z = np.ascontiguousarray(z, dtype=np.float64)
    winner = None if winner is None else np.ascontiguousarray(winner, dtype=np.int32)
    frame = None if frame is None else np.ascontiguousarray(frame, dtype=np.float32)
    face_off = None if face_off is None else np.ascontiguousarray(face_off, dtype=np.int32).ravel()
    if z.ndim != 2 or (winner is not None and winner.shape != z.shape) or (frame is not None and frame.shape != z.shape + (3,)):
        raise ValueError(f"z and winner must be (H, W) and frame (H, W, 3), got {z.shape}, "
                         f"{None if winner is None else winner.shape} and {None if frame is None else frame.shape}")
    if face_off is not None and len(face_off) != desc.n_models:
        raise ValueError(f"{len(face_off)} first faces for {desc.n_models} models")
    return z, winner, frame, face_off


def host_velocity(z, winner, face_off, desc):
    """``mr_host_velocity``: the velocity's definition on the host, no device.  *z* ``(Hs, Ws)`` float64, *winner* ``(Hs, Ws)``
    int32, *face_off* the models' first faces, *desc* a ``MotionDesc``; returns U, float32 ``(Hs, Ws, 2)``.  ``ValueError``
    with the library's text for what it refuses."""
    z, winner, _, face_off = _motion_arrays(z, winner, None, face_off, desc)
    out = np.empty(z.shape + (2,), dtype=np.float32)
    _check_accum(load_library().mr_host_velocity(z.ctypes.data, winner.ctypes.data, face_off.ctypes.data if len(face_off) else None,
                                                 z.shape[0], z.shape[1], C.byref(desc), out.ctypes.data), "mr_host_velocity")
    return out


def host_motion_blur(z, velocity, frame, desc):
    """``mr_host_motion_blur``: the blur's definition on the host, no device.  *velocity* ``(Hs, Ws, 2)`` float32, *frame*
    ``(Hs, Ws, 3)`` float32; returns the blurred frame."""
    z, _, frame, _ = _motion_arrays(z, None, frame, None, desc)
    velocity = np.ascontiguousarray(velocity, dtype=np.float32)
    if velocity.shape != z.shape + (2,):
        raise ValueError(f"velocity must be (H, W, 2), got {velocity.shape}")
    out = np.empty_like(frame)
    _check_accum(load_library().mr_host_motion_blur(z.ctypes.data, velocity.ctypes.data, frame.ctypes.data, z.shape[0], z.shape[1],
                                                    C.byref(desc), out.ctypes.data), "mr_host_motion_blur")
    return out


def debug_motion_post(handle, z, winner, frame, face_off, desc, shape=0):
    """``mr_debug_motion_post``: k_velocity and k_mblur on the caller's arrays, no frame rendered; *shape* 0 .. 2 is
    k_mblur's workgroup.  Returns ``(U float32 (Hs, Ws, 2), blurred frame float32 (Hs, Ws, 3))``."""
    z, winner, frame, face_off = _motion_arrays(z, winner, frame, face_off, desc)
    vel = np.empty(z.shape + (2,), dtype=np.float32)
    out = np.empty_like(frame)
    _check_accum(load_library().mr_debug_motion_post(handle, z.ctypes.data, winner.ctypes.data, frame.ctypes.data,
                                                     face_off.ctypes.data if len(face_off) else None, z.shape[0], z.shape[1],
                                                     C.byref(desc), int(shape), vel.ctypes.data, out.ctypes.data),
                 "mr_debug_motion_post")
    return vel, out


def bloom_levels(height, width, levels):
    """The pyramid of a ``(height, width)`` sample grid: ``[(H_1, W_1), ..., (H_L, W_L)]``, every extent the ceiling of half
    the one before."""
    sizes = []
    for _ in range(int(levels)):
        height, width = (height + 1) // 2, (width + 1) // 2
        sizes.append((height, width))
    return sizes


def _bloom_pyramid(flat, height, width, levels):
    """What ``mr_host_bloom`` packs, as ``(D, U)``: ``D[l - 1]`` is ``D_l``, ``U[l - 1]`` is ``U_l`` (``U[L - 1]`` is ``D_L`` itself)."""
    sizes = bloom_levels(height, width, levels)
    at, down = 0, []
    for h, w in sizes:
        down.append(flat[at:at + h * w * 3].reshape(h, w, 3))
        at += h * w * 3
    up = [None] * len(sizes)
    up[-1] = down[-1]
    for l in range(len(sizes) - 2, -1, -1):
        h, w = sizes[l]
        up[l] = flat[at:at + h * w * 3].reshape(h, w, 3)
        at += h * w * 3
    assert at == len(flat)
    return down, up


def _bloom_call(entry, name, head, frame, desc, tail, pyramid, guard):
    frame = np.ascontiguousarray(frame, dtype=np.float32)
    if frame.ndim != 3 or frame.shape[2] != 3:
        raise ValueError(f"frame must be (H, W, 3), got {frame.shape}")
    h, w = frame.shape[:2]
    sizes = bloom_levels(h, w, max(min(int(desc.levels), 8), 0))
    n_pyr = 2 * sum(a * b * 3 for a, b in sizes) - (sizes[-1][0] * sizes[-1][1] * 3 if sizes else 0)
    # (both outputs between `guard` floats of a value the library never writes: the entry fills its float counts and no more)
    out = np.full(frame.size + 2 * guard, -7.5, dtype=np.float32)
    pyr = np.full(n_pyr + 2 * guard, -7.5, dtype=np.float32)
    _check_accum(entry(*head, frame.ctypes.data, h, w, C.byref(desc), *tail, out[guard:].ctypes.data,
                       pyr[guard:].ctypes.data if pyramid else None), name)
    touched = sum(int((a[:guard] != -7.5).sum() + (a[len(a) - guard:] != -7.5).sum()) for a in (out, pyr)) if guard else 0
    if touched:
        raise AssertionError(f"{name}: {touched} guard floats round the outputs changed")
    result = out[guard:guard + frame.size].reshape(frame.shape)
    if not pyramid:
        return result
    return (result,) + _bloom_pyramid(pyr[guard:guard + n_pyr], h, w, len(sizes))


def host_bloom(frame, desc, pyramid=False, guard=16):
    """``mr_host_bloom``: the bloom's definition on the host, no device.  *frame* ``(Hs, Ws, 3)`` float32, *desc* a
    ``BloomDesc``; returns the frame with the glow, and with *pyramid* ``(frame, D, U)``: the levels ``D_1 .. D_L`` and ``U_1 ..
    U_L`` as lists of ``(H_l, W_l, 3)`` arrays (``U[-1]`` is ``D[-1]``).  Both outputs are handed over between *guard* floats,
    which must come back untouched.  ``ValueError`` with the library's text for what it refuses."""
    return _bloom_call(load_library().mr_host_bloom, "mr_host_bloom", (), frame, desc, (), pyramid, guard)


def debug_bloom_post(handle, frame, desc, shape=0, pyramid=False, guard=16):
    """``mr_debug_bloom_post``: the bloom's kernels on the caller's frame, no frame rendered; *shape* 0 .. 2 is
    ``k_bloom_down``'s workgroup.  Returns what ``host_bloom`` returns."""
    return _bloom_call(load_library().mr_debug_bloom_post, "mr_debug_bloom_post", (handle,), frame, desc, (int(shape),), pyramid, guard)


def shafts_level(height, width, levels):
    """``(H_d, W_d)``: a ``(height, width)`` sample grid halved *levels* times, every extent the ceiling of half the one before."""
    for _ in range(int(levels)):
        height, width = (height + 1) // 2, (width + 1) // 2
    return height, width


def _shafts_call(entry, name, head, frame, zbuf, desc, fields, guard):
    frame = np.ascontiguousarray(frame, dtype=np.float32)
    zbuf = np.ascontiguousarray(zbuf, dtype=np.float64)
    if frame.ndim != 3 or frame.shape[2] != 3:
        raise ValueError(f"frame must be (H, W, 3), got {frame.shape}")
    if zbuf.shape != frame.shape[:2]:
        raise ValueError(f"zbuf must be (H, W) = {frame.shape[:2]}, got {zbuf.shape}")
    h, w = frame.shape[:2]
    ch, cw = shafts_level(h, w, max(min(int(desc.halvings), 4), 0))
    # (every output between `guard` floats of a value the library never writes: the entry fills its float counts and no more)
    arrays = [np.full(n + 2 * guard, -7.5, dtype=np.float32) for n in (frame.size, ch * cw * 3, ch * cw * 3)]
    out, src, march = arrays
    _check_accum(entry(*head, frame.ctypes.data, zbuf.ctypes.data, h, w, C.byref(desc), out[guard:].ctypes.data,
                       src[guard:].ctypes.data if fields else None, march[guard:].ctypes.data if fields else None), name)
    touched = sum(int((a[:guard] != -7.5).sum() + (a[len(a) - guard:] != -7.5).sum()) for a in arrays) if guard else 0
    if touched:
        raise AssertionError(f"{name}: {touched} guard floats round the outputs changed")
    result = out[guard:guard + frame.size].reshape(frame.shape)
    if not fields:
        return result
    return result, src[guard:guard + ch * cw * 3].reshape(ch, cw, 3), march[guard:guard + ch * cw * 3].reshape(ch, cw, 3)


def host_light_shafts(frame, zbuf, desc, fields=False, guard=16):
    """``mr_host_light_shafts``: the light shafts' definition on the host, no device.  *frame* ``(Hs, Ws, 3)`` float32, *zbuf*
    ``(Hs, Ws)`` float64, *desc* a ``LightShaftsDesc``; returns the frame with the shafts, and with *fields* ``(frame, S, R)``,
    the march's source and result as ``(H_d, W_d, 3)`` arrays.  Every output is handed over between *guard* floats, which
    must come back untouched.  ``ValueError`` with the library's text for what it refuses."""
    return _shafts_call(load_library().mr_host_light_shafts, "mr_host_light_shafts", (), frame, zbuf, desc, fields, guard)


def debug_light_shafts_post(handle, frame, zbuf, desc, fields=False, guard=16):
    """``mr_debug_light_shafts_post``: the light shafts' kernels on the caller's frame and z-buffer, no frame rendered.
    Returns what ``host_light_shafts`` returns."""
    return _shafts_call(load_library().mr_debug_light_shafts_post, "mr_debug_light_shafts_post", (handle,), frame, zbuf, desc, fields, guard)


def _tone_map_call(entry, name, head, frame, desc, e_prev, tail, n_exposure, guard):
    frame = np.ascontiguousarray(frame, dtype=np.float32)
    if frame.ndim != 3 or frame.shape[2] != 3:
        raise ValueError(f"frame must be (H, W, 3), got {frame.shape}")
    h, w = frame.shape[:2]
    # (every output between `guard` words of a value the library never writes: the entry fills its counts and no more)
    out = np.full(frame.size + 2 * guard, -7.5, dtype=np.float32)
    hist = np.full(256 + 2 * guard, 0xfeedbeef, dtype=np.uint32)
    exposure = np.full(n_exposure + 2 * guard, -7.5, dtype=np.float32)
    _check_accum(entry(*head, frame.ctypes.data, h, w, C.byref(desc), int(e_prev is not None), 0.0 if e_prev is None else float(e_prev), *tail,
                       out[guard:].ctypes.data, hist[guard:].ctypes.data, exposure[guard:].ctypes.data), name)
    touched = sum(int((a[:guard] != fill).sum() + (a[len(a) - guard:] != fill).sum())
                  for a, fill in ((out, -7.5), (hist, 0xfeedbeef), (exposure, -7.5))) if guard else 0
    if touched:
        raise AssertionError(f"{name}: {touched} guard words round the outputs changed")
    return out[guard:guard + frame.size].reshape(frame.shape), hist[guard:guard + 256].copy(), exposure[guard:guard + n_exposure].copy()


def host_tone_map(frame, desc, e_prev=None, guard=16):
    """``mr_host_tone_map``: the tone mapping's definition on the host, no device.  *frame* ``(Hs, Ws, 3)`` float32, *desc* a
    ``ToneMapDesc``, *e_prev* the scene's previous exposure or ``None``; returns ``(frame, histogram, exposure)``: the
    tone-mapped frame, the 256 uint32 counts and ``e`` as a float32.  Every output is handed over between *guard* words,
    which must come back untouched.  ``ValueError`` with the library's text for what it refuses."""
    out, hist, e = _tone_map_call(load_library().mr_host_tone_map, "mr_host_tone_map", (), frame, desc, e_prev, (), 1, guard)
    return out, hist, e[0]


def debug_tone_map_post(handle, frame, desc, e_prev=None, grid_cap=0, form=-1, guard=16, times=False):
    """``mr_debug_tone_map_post``: the tone mapping's kernels on the caller's frame, no frame rendered; *grid_cap* caps
    ``k_lum_hist``'s grid (0: the library's default), *form* is its form (0, 1; -1: the default).  Returns ``(frame,
    histogram, exposure, state)``: what ``host_tone_map`` returns and the state cell a scene would adopt; with *times* a
    fifth item, the device milliseconds of the three kernels as a dict (``DeviceRenderer.TONE_MAP_TIME_NAMES``)."""
    ms = np.zeros(3, dtype=np.float32)
    entry = load_library().mr_debug_tone_map_post
    out, hist, e = _tone_map_call(lambda *a: entry(*a, ms.ctypes.data if times else None), "mr_debug_tone_map_post", (handle,), frame, desc, e_prev,
                                  (int(grid_cap), int(form)), 2, guard)
    if times:
        return out, hist, e[0], e[1], dict(zip(DeviceRenderer.TONE_MAP_TIME_NAMES, (float(v) for v in ms)))
    return out, hist, e[0], e[1]


def _taa_arrays(frame, velocity, history):
    frame = np.ascontiguousarray(frame, dtype=np.float32)
    velocity = np.ascontiguousarray(velocity, dtype=np.float32)
    history = None if history is None else np.ascontiguousarray(history, dtype=np.float32)
    if frame.ndim != 3 or frame.shape[2] != 3 or velocity.shape != frame.shape[:2] + (2,) or (history is not None and history.shape != frame.shape):
        raise ValueError(f"frame and history must be (H, W, 3) and velocity (H, W, 2), got {frame.shape}, "
                         f"{None if history is None else history.shape} and {velocity.shape}")
    return frame, velocity, history


def host_taa(frame, velocity, history, blend):
    """``mr_host_taa``: the temporal anti-aliasing's definition on the host, no device.  *frame* ``(Hs, Ws, 3)`` float32,
    *velocity* ``(Hs, Ws, 2)`` float32, *history* like *frame* or ``None`` (no history); returns the blended frame, which is
    also the new history.  ``ValueError`` with the library's text for what it refuses."""
    frame, velocity, history = _taa_arrays(frame, velocity, history)
    out = np.empty_like(frame)
    _check_accum(load_library().mr_host_taa(frame.ctypes.data, velocity.ctypes.data, None if history is None else history.ctypes.data,
                                            frame.shape[0], frame.shape[1], float(blend), out.ctypes.data), "mr_host_taa")
    return out


def debug_taa_post(handle, frame, velocity, history, blend, shape=0):
    """``mr_debug_taa_post``: k_taa on the caller's arrays, no frame rendered; *shape* 0 .. 2 is its workgroup.  Returns
    ``(the float frame, the new history, guard bytes the kernel changed)``."""
    frame, velocity, history = _taa_arrays(frame, velocity, history)
    out, hist = np.empty_like(frame), np.empty_like(frame)
    guard = C.c_int32(-1)
    _check_accum(load_library().mr_debug_taa_post(handle, frame.ctypes.data, velocity.ctypes.data,
                                                  None if history is None else history.ctypes.data, frame.shape[0], frame.shape[1],
                                                  float(blend), int(shape), out.ctypes.data, hist.ctypes.data, C.byref(guard)),
                 "mr_debug_taa_post")
    return out, hist, int(guard.value)


def _face_arrays(verts_now, verts_prev, faces, s_now, s_prev):
    verts_now = np.ascontiguousarray(verts_now, dtype=np.float64)
    verts_prev = np.ascontiguousarray(verts_prev, dtype=np.float64)
    faces = np.ascontiguousarray(faces, dtype=np.int32)
    if verts_now.ndim != 2 or verts_now.shape[1] != 4 or verts_prev.shape != verts_now.shape:
        raise ValueError(f"the vertices must be two (n, 4) arrays, got {verts_now.shape} and {verts_prev.shape}")
    if faces.ndim != 2 or faces.shape[1] != 12:
        raise ValueError(f"faces must be (n, 12) int32 records, got {faces.shape}")
    s_now = np.ascontiguousarray(s_now, dtype=np.float64)
    s_prev = np.ascontiguousarray(s_prev, dtype=np.float64)
    if s_now.shape != (4, 3) or s_prev.shape != (4, 3):
        raise ValueError(f"s_now and s_prev must be (4, 3), got {s_now.shape} and {s_prev.shape}")
    return verts_now, verts_prev, faces, s_now, s_prev


def face_records(corners):
    """The 12-int32 face records of ``(n, 3)`` vertex indices: corners at 0, 4 and 8, the rest zero."""
    corners = np.asarray(corners, dtype=np.int32).reshape(-1, 3)
    faces = np.zeros((len(corners), 12), dtype=np.int32)
    faces[:, 0], faces[:, 4], faces[:, 8] = corners[:, 0], corners[:, 1], corners[:, 2]
    return faces


def hom_offsets(face_off, deforming, n_faces):
    """``(hom_off, n_records)`` as the library lays the flagged models' records out: one model after the other, -1 for a
    model that is not flagged (or has no face)."""
    face_off = np.asarray(face_off, dtype=np.int64).ravel()
    ends = np.append(face_off[1:], int(n_faces))
    hom_off = np.full(len(face_off), -1, dtype=np.int32)
    records = 0
    for m, flagged in enumerate(np.asarray(deforming).ravel()):
        if flagged and ends[m] > face_off[m]:
            hom_off[m] = records
            records += int(ends[m] - face_off[m])
    return hom_off, records


def host_face_homographies(verts_now, verts_prev, faces, s_now, s_prev):
    """``mr_host_face_homographies``: H of every face on the host, float64 ``(n_faces, 3, 3)``.  ``ValueError`` with the
    library's text for what it refuses."""
    verts_now, verts_prev, faces, s_now, s_prev = _face_arrays(verts_now, verts_prev, faces, s_now, s_prev)
    out = np.empty((len(faces), 3, 3), dtype=np.float64)
    _check_accum(load_library().mr_host_face_homographies(verts_now.ctypes.data, verts_prev.ctypes.data, len(verts_now), faces.ctypes.data,
                                                          len(faces), s_now.ctypes.data, s_prev.ctypes.data, out.ctypes.data),
                 "mr_host_face_homographies")
    return out


def host_velocity_faces(winner, face_off, hom_off, h, velocity):
    """``mr_host_velocity_faces``: a copy of *velocity* ``(Hs, Ws, 2)`` with U of the flagged models' samples overwritten
    from the records *h* ``(n_records, 3, 3)``."""
    winner = np.ascontiguousarray(winner, dtype=np.int32)
    face_off = np.ascontiguousarray(face_off, dtype=np.int32).ravel()
    hom_off = np.ascontiguousarray(hom_off, dtype=np.int32).ravel()
    h = np.ascontiguousarray(h, dtype=np.float64).reshape(-1, 9)
    out = np.array(velocity, dtype=np.float32, order="C")
    if winner.ndim != 2 or out.shape != winner.shape + (2,) or len(hom_off) != len(face_off):
        raise ValueError(f"winner must be (H, W), velocity (H, W, 2) and hom_off as long as face_off, got {winner.shape}, {out.shape}, "
                         f"{len(hom_off)} and {len(face_off)}")
    _check_accum(load_library().mr_host_velocity_faces(winner.ctypes.data, face_off.ctypes.data, hom_off.ctypes.data, len(face_off),
                                                       h.ctypes.data, len(h), winner.shape[0], winner.shape[1], out.ctypes.data),
                 "mr_host_velocity_faces")
    return out


def debug_motion_faces_post(handle, verts_now, verts_prev, faces, face_off, deforming, s_now, s_prev, winner, velocity):
    """``mr_debug_motion_faces_post``: k_face_homography and k_velocity_faces on the caller's arrays, no frame rendered.
    Returns ``(H float64 (n_records, 3, 3), U float32 (Hs, Ws, 2), guard bytes the kernels changed)``."""
    verts_now, verts_prev, faces, s_now, s_prev = _face_arrays(verts_now, verts_prev, faces, s_now, s_prev)
    winner = np.ascontiguousarray(winner, dtype=np.int32)
    face_off = np.ascontiguousarray(face_off, dtype=np.int32).ravel()
    deforming = np.ascontiguousarray(deforming, dtype=np.int32).ravel()
    out = np.array(velocity, dtype=np.float32, order="C")
    if winner.ndim != 2 or out.shape != winner.shape + (2,) or len(deforming) != len(face_off):
        raise ValueError(f"winner must be (H, W), velocity (H, W, 2) and deforming as long as face_off, got {winner.shape}, {out.shape}, "
                         f"{len(deforming)} and {len(face_off)}")
    h = np.full((max(len(faces), 1), 3, 3), np.nan)
    guard = C.c_int32(-1)
    _check_accum(load_library().mr_debug_motion_faces_post(
        handle, verts_now.ctypes.data, verts_prev.ctypes.data, len(verts_now), faces.ctypes.data, len(faces), face_off.ctypes.data,
        deforming.ctypes.data, len(face_off), s_now.ctypes.data, s_prev.ctypes.data, winner.ctypes.data, winner.shape[0], winner.shape[1],
        out.ctypes.data, h.ctypes.data, C.byref(guard)), "mr_debug_motion_faces_post")
    return h[:hom_offsets(face_off, deforming, len(faces))[1]], out, int(guard.value)


FACE_POS_DTYPES = {True: np.dtype([("v", np.float32, (3, 4)), ("material", np.int32), ("flags", np.uint32), ("pad", np.uint32, (2,))]),
                   False: np.dtype([("v", np.float64, (3, 4)), ("material", np.int32), ("flags", np.uint32), ("pad", np.uint32, (2,))])}
FACE_ATTR_DTYPE = np.dtype([("uv", np.float32, (3, 2)), ("n", np.float32, (3, 3)), ("pad", np.float32)])
FF_HAS_NORMALS, FF_HAS_UV = 4, 8
LAYERS_SENTINEL = 0xa5


def _layers_arrays(winner, face_pos, face_attr, face_off):
    winner = np.ascontiguousarray(winner, dtype=np.int32)
    face_off = np.ascontiguousarray(face_off, dtype=np.int32).ravel()
    face_pos, face_attr = np.ascontiguousarray(face_pos), np.ascontiguousarray(face_attr)
    if winner.ndim != 2:
        raise ValueError(f"winner must be (H, W), got {winner.shape}")
    if face_pos.dtype not in FACE_POS_DTYPES.values() or face_attr.dtype != FACE_ATTR_DTYPE or face_pos.shape != face_attr.shape or face_pos.ndim != 1:
        raise ValueError("face_pos and face_attr must be record arrays of FACE_POS_DTYPES and FACE_ATTR_DTYPE, one record a face")
    return winner, face_pos, face_attr, face_off, int(face_pos.dtype == FACE_POS_DTYPES[True])


def _layers_outputs(shape, fill_byte=None):
    """One array a layer, on the sample grid *shape*, and the table of their addresses."""
    from ._pack import LAYER_CHANNELS, LAYER_DTYPES
    arrays = []
    for dtype, channels in zip(LAYER_DTYPES, LAYER_CHANNELS):
        a = np.zeros(tuple(shape) + ((channels,) if channels > 1 else ()), dtype=dtype)
        if fill_byte is not None:
            a.view(np.uint8)[...] = fill_byte
        arrays.append(a)
    return arrays, (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def host_layers(winner, face_pos, face_attr, face_off, desc):
    """``mr_host_layers``: the data layers' definition on the host, no device.  *winner* ``(Hs, Ws)`` int32, *face_pos* and
    *face_attr* record arrays (``FACE_POS_DTYPES``, ``FACE_ATTR_DTYPE``), *face_off* the models' first faces, *desc* a
    ``LayersDesc`` whose ``n_models`` is ``len(face_off)``.  Returns ``(layers, degenerate)``: a dict name -> array of the
    layers the mask names, and the number of degenerate samples.  ``ValueError`` with the library's text for what it refuses."""
    from ._pack import LAYER_NAMES
    winner, face_pos, face_attr, face_off, pos32 = _layers_arrays(winner, face_pos, face_attr, face_off)
    arrays, table = _layers_outputs(winner.shape)
    degenerate = C.c_int64(-1)
    _check_accum(load_library().mr_host_layers(winner.ctypes.data, winner.shape[0], winner.shape[1], face_pos.ctypes.data, pos32, face_attr.ctypes.data,
                                               len(face_pos), face_off.ctypes.data, C.byref(desc), table, C.byref(degenerate)), "mr_host_layers")
    return {name: a for i, (name, a) in enumerate(zip(LAYER_NAMES, arrays)) if desc.mask >> i & 1}, int(degenerate.value)


def debug_layers_post(handle, winner, face_pos, face_attr, face_off, desc, times=False):
    """``mr_debug_layers_post``: ``k_layers`` on the caller's arrays, no frame rendered.  Returns ``(layers, guard)``: a dict
    name -> array of ALL nine layers -- one the mask does not name comes back as the sentinel byte ``LAYERS_SENTINEL`` -- and
    the guard bytes the kernel changed; with *times* a third item, the kernel's device milliseconds."""
    from ._pack import LAYER_NAMES
    winner, face_pos, face_attr, face_off, pos32 = _layers_arrays(winner, face_pos, face_attr, face_off)
    arrays, table = _layers_outputs(winner.shape, fill_byte=0x3c)
    guard, ms = C.c_int32(-1), C.c_float(0)
    _check_accum(load_library().mr_debug_layers_post(handle, winner.ctypes.data, winner.shape[0], winner.shape[1], face_pos.ctypes.data, pos32,
                                                     face_attr.ctypes.data, len(face_pos), face_off.ctypes.data, C.byref(desc), table,
                                                     C.byref(guard), C.byref(ms) if times else None), "mr_debug_layers_post")
    out = dict(zip(LAYER_NAMES, arrays))
    return (out, int(guard.value), float(ms.value)) if times else (out, int(guard.value))


def stripe_out_rows(height, stripe_count):
    """Rows of a device's output buffer in the striped layout (``mr_frame_desc.stripe_count``)."""
    tile_rows = -(-int(height) // 16)
    return -(-tile_rows // int(stripe_count)) * 16


def fill_frame_desc(pf, row_band=None, keep_float=False, light_timing=False, face_status=False, counters=False,
                    keep_buffers=False, stripe=None, no_timing=False, overlay=False):
    d = FrameDesc()
    d.width, d.height, d.system = pf.width, pf.height, pf.system
    d.backface_culling, d.light_type = int(pf.backface_culling), pf.light_type
    d.flags = ((FRAME_SHADOWS if pf.shadows else 0) | (FRAME_KEEP_FLOAT if keep_float else 0)
               | (FRAME_LIGHT_TIMING if light_timing else 0) | (FRAME_FACE_STATUS if face_status else 0)
               | (FRAME_COUNTERS if counters else 0) | (FRAME_KEEP_BUFFERS if keep_buffers else 0)
               | (FRAME_NO_TIMING if no_timing else 0) | (FRAME_OVERLAY if overlay else 0))
    # a supersampled frame (pf is its sample grid): row_band counts OUTPUT rows, the descriptor sample rows
    ss = int(getattr(pf, "supersample", 1))
    d.flags |= _SUPERSAMPLE_FLAGS[ss]
    d.row_begin, d.row_end = (0, pf.height) if row_band is None else (int(row_band[0]) * ss, int(row_band[1]) * ss)
    if stripe is not None:                      # (index, count): interleaved tile rows, see mi355rast.h
        d.stripe_index, d.stripe_count = int(stripe[0]), int(stripe[1])
    for name in ("mvp", "viewport", "debug_mvp", "frustum_planes", "camera_pos", "light_pos", "light_dir",
                 "light_color", "light_ambient"):
        src = np.ascontiguousarray(getattr(pf, name), dtype=np.float64)
        C.memmove(getattr(d, name), src.ctypes.data, src.nbytes)
    d.z_near, d.z_far = pf.z_near, pf.z_far
    d.specular_strength = pf.specular_strength
    d.att_constant, d.att_linear, d.att_quadratic = pf.att_constant, pf.att_linear, pf.att_quadratic
    d.spot_edge0, d.spot_edge1 = pf.spot_edge0, pf.spot_edge1
    for i in range(3):
        d.background[i] = float(pf.background[i])
    # the finalised background exactly as the reference computes it (float32 ** 0.8 * 255 -> uint8)
    bg = (np.asarray(pf.background, dtype=np.float32) ** 0.8 * 255).astype(np.uint8)
    d.background_u8 = int(bg[0]) | int(bg[1]) << 8 | int(bg[2]) << 16 | 1 << 24
    if pf.sky_tri is not None:
        d.flags |= FRAME_SKYBOX
        for i, v in enumerate(np.asarray(pf.sky_tri, dtype=np.int32).ravel()):
            d.sky_tri[i] = int(v)
        for i, v in enumerate(np.asarray(pf.sky_rays, dtype=np.float64).ravel()):
            d.sky_rays[i] = v
    return d


class _PinnedPool:
    """Page-locked output buffers for ``mr_render``, recycled when the NumPy array that wraps one is
    garbage collected: a render loop that drops each frame before asking for the next allocates once."""

    def __init__(self, lib, keep=4):
        self.lib, self.keep = lib, keep
        self.free = {}                       # bytes -> [pointers]

    def array(self, shape):
        import weakref
        nbytes = int(np.prod(shape))
        stock = self.free.setdefault(nbytes, [])
        ptr = stock.pop() if stock else self.lib.mr_host_alloc(nbytes)
        if not ptr:
            return np.empty(shape, dtype=np.uint8)           # pageable memory still works, just slower
        raw = (C.c_uint8 * nbytes).from_address(ptr)
        arr = np.frombuffer(raw, dtype=np.uint8).reshape(shape)
        weakref.finalize(raw, self._release, nbytes, ptr)       # raw lives as long as any view of arr does
        return arr

    def _release(self, nbytes, ptr):
        stock = self.free.setdefault(nbytes, [])
        if len(stock) < self.keep:
            stock.append(ptr)
        else:
            self.lib.mr_host_free(ptr)

    def close(self):
        for stock in self.free.values():
            while stock:
                self.lib.mr_host_free(stock.pop())


class DeviceRenderer:
    """Owns one ``mr_scene`` handle and keeps it in step with a Python ``Scene``."""

    def __init__(self, device=None):
        self.lib = load_library()
        _check(self.lib.mr_init(-1 if device is None else int(device)), "mr_init")
        self.handle = self.lib.mr_scene_create()
        if not self.handle:
            raise RuntimeError("mr_scene_create failed: " + self.lib.mr_last_error().decode())
        self._signature = None
        self._pose_keys = []                 # per model: (bytes of the pose, bytes of the normal matrix or None) the library holds, or None
        self._skin_keys = {}                 # model index -> [serial of the skin, its bone count, bytes of the bones or None] the library holds
        self._morph_keys = {}                # model index -> [serial of the morph, bytes of the weights or None] the library holds
        self._auto_keys = {}                 # model index -> True where the library holds the auto_normals flag
        self._sky_key = None
        self._last_stats = {}
        self._frame = None
        self._packed = (None, None)          # (key, PackedFrame) of the last frame's per-frame constants
        self._pinned = _PinnedPool(self.lib)

    # -- scene upload ---------------------------------------------------------------------
    @staticmethod
    def _fingerprint(arr):
        """Cheap identity of an array's CONTENT: where it lives, its layout, and a checksum of ~64 WHOLE rows
        spread evenly over the array (a few microseconds).  Catches replacement and wholesale in-place edits,
        including an edit of a single column (every row changes, so every sampled row does; sampling flat
        elements at a stride that shares a factor with the row width would skip whole columns); a poke at a
        few single elements needs ``Model.invalidate()``."""
        if arr is None:
            return None
        a = np.asarray(arr)
        rows = a.reshape(a.shape[0], -1) if a.ndim > 1 else a.reshape(-1, 1)
        step = max(1, rows.shape[0] // 64)
        return (a.__array_interface__["data"][0], a.shape, a.dtype.str, zlib.crc32(np.ascontiguousarray(rows[::step])))

    @classmethod
    def _scene_signature(cls, scene):
        from .materials import Material
        return (Material.revision,) + tuple(
            (id(m), m._revision, cls._fingerprint(m.vertices), cls._fingerprint(m._faces), cls._fingerprint(m.uv),
             cls._fingerprint(m.normals), bool(m.clip), bool(m.depth_test), tuple(m.material_group))
            for m in scene.models)

    def sync_scene(self, scene):
        """The library's scene in step with the Python one: everything again when a model, texture or material changed
        (``_scene_signature``), and the models' poses, which are no part of that signature, beside it."""
        for model in scene.models:
            active_skin(model)                   # (a skin that no longer fits its vertices: ValueError before any device work)
            active_morph(model)                  # (... or a morph)
        sig = self._scene_signature(scene)
        if sig != self._signature:
            self._upload_scene(scene)
            self._signature = sig
            self._pose_keys = [None] * len(scene.models)        # (mr_scene_clear dropped the poses)
            self._skin_keys = {}                                 # (... and the skins)
            self._morph_keys = {}                                # (... and the morphs)
            self._auto_keys = {}                                 # (... and the auto_normals flags)
        self.sync_poses(scene)

    def sync_poses(self, scene):
        """``mr_scene_set_model_pose`` for every model whose ``pose`` is not the one the library holds, and
        ``mr_scene_set_model_pose_normals`` after it where the normal matrix (``Model.pose_normals``) is not; then the
        same for the skins: a model is keyed by (pose bytes, G bytes) and (serial of its skin, bones bytes), and each of
        ``mr_scene_set_model_skin`` / ``mr_scene_set_model_bones`` is called when its part changed.  A skin goes to the
        library when its model first has bones: a scene without bones makes no call.  The morphs likewise: (serial of the
        morph, weight bytes), ``mr_scene_set_model_morph`` / ``mr_scene_set_model_morph_weights``, the tables handed over
        when the model first has weights.  ``Model.auto_normals`` goes over (``mr_scene_set_model_auto_normals``) when
        it changes for a model it has an effect on -- moved, with normals: a scene without such a model makes no call."""
        keys = self._pose_keys
        for index, model in enumerate(scene.models):
            self._sync_auto_normals(index, model)
            self._sync_morph(index, model)
            self._sync_skin(index, model)
            pose = getattr(model, "pose", None)
            g = None if pose is None else pose_normal_matrix(model)
            key = None if pose is None else (pose.tobytes(), None if g is None else g.tobytes())
            if key == keys[index]:
                continue
            _check(self.lib.mr_scene_set_model_pose(self.handle, index, None if pose is None else pose.ctypes.data),
                   "mr_scene_set_model_pose")
            held = None if keys[index] is None else keys[index][1]
            if key is not None and key[1] != held:            # (the library lets go of the matrix with the pose)
                _check(self.lib.mr_scene_set_model_pose_normals(self.handle, index, None if g is None else g.ctypes.data),
                       "mr_scene_set_model_pose_normals")
            keys[index] = key

    def _sync_auto_normals(self, index, model):
        held = self.__dict__.setdefault("_auto_keys", {})
        on = auto_normals_active(model)
        if on != held.get(index, False):
            _check(self.lib.mr_scene_set_model_auto_normals(self.handle, index, int(on)), "mr_scene_set_model_auto_normals")
            held[index] = on

    def _sync_morph(self, index, model):
        keys = self.__dict__.setdefault("_morph_keys", {})
        held = keys.get(index)                   # [serial of the morph, bytes of the weights or None]
        morph = active_morph(model)
        if morph is None:
            if held is not None and held[1] is not None:       # morph_weights = None, or the morph is gone: the rest shape
                _check(self.lib.mr_scene_set_model_morph_weights(self.handle, index, None, 0), "mr_scene_set_model_morph_weights")
                held[1] = None
            return
        if held is None:
            held = keys[index] = [None, None]
        if held[0] != model._morph_serial:
            first, vindex, delta = morph_csr(morph.targets)
            nfirst, nindex, ndelta = (None, None, None) if morph.normal_targets is None else morph_csr(morph.normal_targets)
            ptr = lambda a: None if a is None else a.ctypes.data
            _check(self.lib.mr_scene_set_model_morph(self.handle, index, len(morph.targets), ptr(first), ptr(vindex), ptr(delta),
                                                     ptr(nfirst), ptr(nindex), ptr(ndelta)), "mr_scene_set_model_morph")
            held[:] = [model._morph_serial, None]
        weights = model.morph_weights
        key = weights.tobytes()
        if held[1] != key:
            _check(self.lib.mr_scene_set_model_morph_weights(self.handle, index, weights.ctypes.data, len(weights)),
                   "mr_scene_set_model_morph_weights")
            held[1] = key

    def _sync_skin(self, index, model):
        keys = self.__dict__.setdefault("_skin_keys", {})
        held = keys.get(index)                   # [serial of the skin, its bone count, bytes of the bones or None]
        skin = active_skin(model)
        if skin is None:
            if held is not None and held[2] is not None:       # bones = None, or the skin is gone: the rest position
                _check(self.lib.mr_scene_set_model_bones(self.handle, index, None, 0), "mr_scene_set_model_bones")
                held[2] = None
            return
        if held is None:
            held = keys[index] = [None, 0, None]
        bones = model.bones
        if held[:2] != [model._skin_serial, len(bones)]:       # (another bone count: the library takes the skin again with it)
            owners = normal_owners(model) if skin.normals and model.normals is not None else None
            _check(self.lib.mr_scene_set_model_skin(self.handle, index, skin.joints.ctypes.data, skin.weights.ctypes.data,
                                                    len(bones), None if owners is None else owners.ctypes.data),
                   "mr_scene_set_model_skin")
            held[:] = [model._skin_serial, len(bones), None]
        key = bones.tobytes()
        if held[2] != key:
            _check(self.lib.mr_scene_set_model_bones(self.handle, index, bones.ctypes.data, len(bones)), "mr_scene_set_model_bones")
            held[2] = key

    def _upload_scene(self, scene):
        _check(self.lib.mr_scene_clear(self.handle), "mr_scene_clear")
        textures, seen, uploaded = [], {}, 0
        for model in scene.models:
            pm = pack_model(model, textures, seen)
            for tex in textures[uploaded:]:
                _check(self.lib.mr_scene_add_texture(self.handle, tex.ctypes.data, tex.shape[0], tex.shape[1]),
                       "mr_scene_add_texture")
            uploaded = len(textures)
            mats = (MaterialDesc * len(pm.materials))()
            for j, m in enumerate(pm.materials):
                for i in range(3):
                    mats[j].kd[i], mats[j].ks255[i] = m.kd[i], m.ks255[i]
                mats[j].ns = m.ns
                mats[j].tex_kd, mats[j].tex_norm, mats[j].tex_ks = m.tex_kd, m.tex_norm, m.tex_ks
                mats[j].norm_tangent = int(m.norm_tangent)
            d = ModelDesc()
            d.vertices = pm.vertices.ctypes.data
            d.uv = pm.uv.ctypes.data if pm.uv is not None else None
            d.normals = pm.normals.ctypes.data if pm.normals is not None else None
            d.faces = pm.faces.ctypes.data
            d.materials = mats
            d.edge_ids = pm.edge_ids.ctypes.data if pm.edge_ids is not None else None
            d.n_vertices = len(pm.vertices)
            d.n_uv = 0 if pm.uv is None else len(pm.uv)
            d.n_normals = 0 if pm.normals is None else len(pm.normals)
            d.n_faces, d.n_materials = len(pm.faces), len(pm.materials)
            d.vertices_are_f32, d.clip, d.depth_test = int(pm.vertices_are_f32), int(pm.clip), int(pm.depth_test)
            _check(self.lib.mr_scene_add_model(self.handle, C.byref(d)), "mr_scene_add_model")

    def sync_skybox(self, scene):
        sky = scene.skybox if hasattr(scene.skybox, "texels") else None
        key = None if sky is None else id(sky.texels)
        if key == self._sky_key:
            return
        if sky is None:
            _check(self.lib.mr_scene_set_skybox(self.handle, None, 0), "mr_scene_set_skybox")
        else:
            tex = np.ascontiguousarray(sky.texels, dtype=np.uint8)
            _check(self.lib.mr_scene_set_skybox(self.handle, tex.ctypes.data, tex.shape[1]), "mr_scene_set_skybox")
        self._sky_key = key

    def sync_overlay(self, scene):
        """Debug-frustum overlay (obj/core.py:638): the statement lists depend on the two cameras and the
        resolution only (a camera's MVP is cached for life), so they are built and uploaded once."""
        cam = scene.camera
        dbg = scene.debug_camera if scene.debug_camera is not None else cam
        # (the lines go through camera.viewport: its offsets and depth range may be reassigned on a camera that stays)
        key = lambda: (id(cam), id(dbg), id(cam.__dict__.get("MVP")), id(dbg.__dict__.get("MVP")), tuple(scene.resolution),
                       int(scene.system), int(scene.subsystem), getattr(scene, "supersample", 1),
                       cam.x_offset, cam.y_offset, float(cam.near), float(cam.far))
        if getattr(self, "_overlay_key", None) == key() or getattr(self, "_overlay_pinned", False):
            return
        # the key holds ids: keep the objects alive while it is cached, so that no other camera or matrix can
        # be given a recycled address and pass for them
        from .frustums import frustum_corners
        # the two inverses / vector products of the recipe stay with NumPy (obj/frustums.py:52-60); everything after
        # them -- clipping, projection, DDA, dashes, the per-pixel lists and their upload -- is one call into the library
        corners, inside = frustum_corners(cam, dbg)
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        corners, planes, mvp = f64(corners), f64(cam.frustum_planes), f64(cam.MVP)
        # (a supersampled frame draws the lines on its sample grid, like the reference at that resolution)
        from ._pack import sample_grid
        _, height, width, viewport = sample_grid(scene)
        viewport = f64(viewport)
        _check(self.lib.mr_scene_set_overlay_cameras(self.handle, corners.ctypes.data, planes.ctypes.data, mvp.ctypes.data,
                                                     viewport.ctypes.data, float(cam.near), float(cam.far), int(inside),
                                                     height, width), "mr_scene_set_overlay_cameras")
        self._overlay_key = key()                    # the MVPs exist (and are cached) now
        self._overlay_refs = (cam, dbg, cam.__dict__.get("MVP"), dbg.__dict__.get("MVP"))

    def set_overlay_lists(self, ops, pin=True):
        """``mr_scene_set_overlay`` with explicit statement lists (a ``frustums.OverlayOps``); ``sync_overlay`` builds
        the same inside the library.  While *pin*ned, frames drawn with the overlay keep these lists instead of
        rebuilding them from the scene's cameras (``pin=False`` hands the overlay back to the cameras)."""
        d = OverlayDesc()
        d.n_segments, d.n_points, d.height, d.width = len(ops.seg_first), ops.n_points, ops.height, ops.width
        d.seg_first, d.seg_count = ops.seg_first.ctypes.data, ops.seg_count.ctypes.data
        d.target, d.z = ops.target.ctypes.data, ops.z.ctypes.data
        _check(self.lib.mr_scene_set_overlay(self.handle, C.byref(d) if ops.n_points else None), "mr_scene_set_overlay")
        self._overlay_key = None
        self._overlay_pinned = ops is not None and pin

    @staticmethod
    def _ao_values(scene):
        """The scene's ``AmbientOcclusion`` by value (``None`` without one), for ``_frame_key``."""
        ao = getattr(scene, "ambient_occlusion", None)
        return None if ao is None else (ao.radius, ao.strength, ao.depth_range, ao.bias)

    def _sync_desc(self, scene, tag, entry, values, fill):
        """What ``sync_ambient_occlusion`` and ``sync_depth_of_field`` do.  *values* is the scene's object by value, ``None``
        without one; *fill* builds the description from the scene and the view; *entry* names the library's setter.  The
        caches are ``_<tag>_key`` (the bytes of the description last handed over) and ``_<tag>_packed`` (what it was built
        from), read with ``getattr``: they work on a renderer whose ``__init__`` never ran."""
        key_name, packed_name = "_%s_key" % tag, "_%s_packed" % tag
        setter = getattr(self.lib, entry)
        if values(scene) is None:
            if getattr(self, key_name, None) is not None:
                _check_accum(setter(self.handle, None), entry)
                setattr(self, key_name, None)
                setattr(self, packed_name, None)
            return
        # (called behind packed_frame: while its entry lives, camera, resolution and supersample are the same)
        packed = (getattr(self, "_pack_serial", 0), values(scene))
        if getattr(self, packed_name, None) == packed:
            return
        desc = fill(scene)
        key = None if desc is None else bytes(desc)           # (None: this view has no use for the pass -- off for this frame)
        if getattr(self, key_name, None) != key:
            _check_accum(setter(self.handle, None if desc is None else C.byref(desc)), entry)
            setattr(self, key_name, key)
        setattr(self, packed_name, packed)

    def sync_ambient_occlusion(self, scene):
        """``mr_scene_set_ambient_occlusion`` for the frames enqueued from now on, whenever the description -- the
        scene's ``AmbientOcclusion`` and the view's depth map and footprint -- is not the one last handed over.  A scene
        that never had one makes no call."""
        self._sync_desc(scene, "ao", "mr_scene_set_ambient_occlusion", self._ao_values,
                        lambda sc: fill_ao_desc(sc.ambient_occlusion, *ao_constants(sc)))

    @staticmethod
    def _dof_values(scene):
        """The scene's ``DepthOfField`` by value (``None`` without one), for ``_frame_key``."""
        dof = getattr(scene, "depth_of_field", None)
        return None if dof is None else (dof.focus, dof.lens_radius)

    def sync_depth_of_field(self, scene):
        """``mr_scene_set_depth_of_field`` for the frames enqueued from now on, whenever the description -- the scene's
        ``DepthOfField`` and the view's depth map, focus and ``kf`` -- is not the one last handed over.  A scene that
        never had one makes no call."""
        self._sync_desc(scene, "dof", "mr_scene_set_depth_of_field", self._dof_values, lambda sc: fill_dof_desc(*dof_constants(sc)))

    @staticmethod
    def _bloom_values(scene):
        """The scene's ``Bloom`` by value (``None`` without one), for ``_frame_key``."""
        bloom = getattr(scene, "bloom", None)
        return None if bloom is None else (bloom.threshold, bloom.intensity, bloom.levels)

    def sync_bloom(self, scene):
        """``mr_scene_set_bloom`` for the frames enqueued from now on, whenever the description -- the scene's ``Bloom``
        and the levels its ``supersample`` adds -- is not the one last handed over.  A scene that never had one makes no
        call."""
        self._sync_desc(scene, "bloom", "mr_scene_set_bloom", self._bloom_values, lambda sc: fill_bloom_desc(*bloom_constants(sc)))

    @staticmethod
    def _light_shafts_values(scene):
        """The scene's ``LightShafts`` by value and what it takes from its light (``None`` without one), for ``_frame_key``.
        ``ValueError`` for a ``light`` index the scene does not have."""
        shafts = getattr(scene, "light_shafts", None)
        if shafts is None:
            return None
        lights = list(scene.lights)
        if shafts.light >= len(lights):
            raise ValueError(f"light shafts: light {shafts.light} does not exist: the scene has {len(lights)}")
        light = lights[shafts.light]
        vec = lambda a: tuple(np.asarray(a, dtype=np.float64).ravel().tolist())
        return (tuple(getattr(shafts, name) for name in shafts.__slots__), id(light), vec(light.position), vec(light.center), str(light.light_type))

    def sync_light_shafts(self, scene):
        """``mr_scene_set_light_shafts`` for the frames enqueued from now on, whenever the description -- the scene's
        ``LightShafts``, its light's place on this view's sample grid, the levels its ``supersample`` adds -- is not the
        one last handed over; a view whose light lies behind the camera hands over NULL.  A scene that never had one
        makes no call."""
        def fill(sc):
            constants = light_shafts_constants(sc)
            return None if constants is None else fill_light_shafts_desc(*constants)
        self._sync_desc(scene, "shafts", "mr_scene_set_light_shafts", self._light_shafts_values, fill)

    @staticmethod
    def _tone_map_values(scene):
        """The scene's ``ToneMap`` by value (``None`` without one), for ``_frame_key``."""
        tm = getattr(scene, "tone_map", None)
        return None if tm is None else tuple(getattr(tm, name) for name in tm.__slots__)

    def sync_tone_map(self, scene, accumulating=False):
        """``mr_scene_set_tone_map`` for the frames enqueued from now on, whenever the description is not the one last handed
        over, and ``mr_scene_reset_exposure`` after ``reset_motion()``.  An adaptive ``ToneMap`` takes one frame of the scene
        at a time and no sub-frame of an accumulation.  A scene that never had one makes no call."""
        tm = getattr(scene, "tone_map", None)
        if tm is not None and tm.adaptive:
            if accumulating:
                raise ValueError("an adaptive tone_map (speed < 1) is not available inside accumulate() / render_mean(): its "
                                 "sub-frames have no previous frame (speed=1 or a fixed exposure is)")
            if scene.__dict__.get("_pending"):
                raise ValueError("an adaptive tone_map (speed < 1) takes one frame of the scene at a time: another frame is "
                                 "pending, take its result() first (every frame reads the exposure the frame before it left)")
        forget = scene.__dict__.pop("_tone_forget", False)
        self._sync_desc(scene, "tone", "mr_scene_set_tone_map", self._tone_map_values, lambda sc: fill_tone_map_desc(*tone_map_constants(sc)))
        if forget and getattr(self, "_tone_key", None) is not None:
            _check_accum(self.lib.mr_scene_reset_exposure(self.handle), "mr_scene_reset_exposure")

    @staticmethod
    def _layers_values(scene):
        """The scene's ``Layers`` by value (``None`` without one), for ``_frame_key``."""
        layers = getattr(scene, "layers", None)
        return None if layers is None else (layers.names, len(scene.models))

    def sync_layers(self, scene, accumulating=False):
        """``mr_scene_set_layers`` for the frames enqueued from now on, whenever the description -- the scene's ``Layers``,
        the view's ``layer_matrix`` with the frame's sub-sample offset, the number of models -- is not the one last handed
        over.  A scene that never had one makes no call."""
        if getattr(scene, "layers", None) is not None and accumulating:
            raise ValueError("layers is not available inside accumulate() / render_mean(): a sum of frames has no one winner a sample")
        self._sync_desc(scene, "layers", "mr_scene_set_layers", self._layers_values,
                        lambda sc: fill_layers_desc(layer_matrix(sc), layer_mask(sc.layers.names), len(sc.models)))

    def _sync_post(self, scene, accumulating=False):
        """The passes behind the tile kernel of the frame being issued, in the order they run: the nine descriptions in step
        with *scene*."""
        self.sync_layers(scene, accumulating)
        self.sync_ambient_occlusion(scene)
        self.sync_temporal_aa(scene)
        self.sync_depth_of_field(scene)
        self.sync_motion_blur(scene)
        self.sync_motion_faces(scene)
        self.sync_light_shafts(scene)
        self.sync_bloom(scene)
        self.sync_tone_map(scene, accumulating)

    @staticmethod
    def _motion_values(scene):
        """The motion of the frame being issued by value (``None`` without ``motion_blur``), for ``_frame_key``."""
        return None if getattr(scene, "motion_blur", None) is None else scene.__dict__.get("_motion_frame")

    @staticmethod
    def _taa_values(scene):
        """The temporal anti-aliasing of the frame being issued by value (``None`` without ``temporal_aa``), for ``_frame_key``."""
        return None if getattr(scene, "temporal_aa", None) is None else scene.__dict__.get("_taa_frame")

    def issue_motion(self, scene, partial=False, accumulating=False):
        """A frame of *scene* is being issued: with ``motion_blur`` or ``temporal_aa`` set, the matrices that lead from it to
        the previous frame's state (``_pack.motion_matrices``) become the scene's ``_motion_frame`` / ``_taa_frame`` -- by
        value, for ``_frame_key``, ``sync_motion_blur`` and ``sync_temporal_aa``, both from the same tables -- and its own
        state becomes the previous one.  With ``temporal_aa`` the frame also takes its place k in the jitter's sequence
        (``_pack.taa_jitter``), which becomes the scene's ``_sample_jitter`` until the frame's descriptor is filled; the
        history is forgotten -- k = 0, and ``sync_temporal_aa`` calls ``mr_scene_reset_history`` -- after ``reset_motion()`` (which every assignment of
        ``motion_blur`` or ``temporal_aa`` calls), with another model list and with a sample grid of another size.  A frame
        rendered again after an overflow (``PendingFrame.result``) takes the matrices and the jitter of its first attempt
        and leaves the previous state alone."""
        mb, taa = getattr(scene, "motion_blur", None), getattr(scene, "temporal_aa", None)
        if mb is None:
            scene.__dict__.pop("_motion_frame", None)
        if taa is None:
            scene.__dict__.pop("_taa_frame", None)
        if mb is None and taa is None:
            return
        if partial and mb is not None:
            raise ValueError("motion blur takes whole frames (no row band, no stripes): its taps cross the bands")
        if partial:
            raise ValueError("temporal AA takes whole frames (no row band, no stripes): its taps cross the bands")
        if accumulating and mb is not None:
            raise ValueError("motion_blur is not available inside accumulate() / render_mean(): the accumulation is the "
                             "other way to blur motion, and its sub-frames have no previous frame")
        if accumulating:
            raise ValueError("temporal_aa is not available inside accumulate() / render_mean(): the accumulation is the "
                             "other way to spread samples over frames, and its sub-frames have no history")
        if taa is not None and scene.__dict__.get("_pending"):
            raise ValueError("temporal_aa takes one frame of the scene at a time: another frame is pending, take its "
                             "result() first (every frame reads the history the frame before it left)")
        replay, taa_replay = scene.__dict__.get("_motion_replay"), scene.__dict__.get("_taa_replay")
        if replay is not None or taa_replay is not None:
            if mb is not None and replay is not None:
                scene.__dict__["_motion_frame"] = replay
                scene.__dict__["_motion_faces_frame"] = scene.__dict__.get("_motion_faces_replay")
            if taa is not None and taa_replay is not None:
                scene.__dict__["_taa_frame"] = taa_replay
                scene.__dict__["_sample_jitter"] = taa_replay[4]
            return
        previous = scene.__dict__.get("_motion_prev")
        if taa is not None:
            grid = tuple(sample_grid(scene)[1:3])
            if grid != scene.__dict__.get("_taa_grid"):          # (resolution or supersample: the previous S is another grid's too)
                previous = None
            scene.__dict__["_taa_grid"] = grid
        depth_map, matrices, background, class_of, state = motion_matrices(scene, previous)
        if mb is not None:
            scene.__dict__["_motion_frame"] = (mb.shutter, tuple(depth_map), matrices.tobytes(), background.tobytes(), class_of.tobytes())
            scene.__dict__["_motion_faces_frame"] = None
            if mb.deformation:             # (the per-face velocity of the models that bend: _pack.motion_vertices)
                s_now, s_prev, deforming, prev_serial = motion_vertices(scene, previous, state)
                scene.__dict__["_motion_faces_frame"] = (s_now.tobytes(), s_prev.tobytes(), deforming.tobytes(), int(prev_serial))
        if taa is not None:
            if scene.__dict__.pop("_taa_forget", False) or previous is None or not state.same_models(previous):
                scene.__dict__["_taa_reset"] = True            # (sync_temporal_aa tells the library)
                scene.__dict__["_taa_k"] = 0
            k = scene.__dict__.get("_taa_k", 0)
            jitter = taa_jitter(k, taa.jitter)
            scene.__dict__["_taa_k"] = k + 1
            scene.__dict__["_taa_frame"] = (taa.blend, matrices.tobytes(), background.tobytes(), class_of.tobytes(), jitter)
            scene.__dict__["_sample_jitter"] = jitter
        scene.__dict__["_motion_prev"] = state

    def sync_temporal_aa(self, scene):
        """``mr_scene_set_temporal_aa`` for the frames enqueued from now on, whenever the frame's description
        (``issue_motion``) is not the one last handed over.  A scene that never had one makes no call."""
        frame = self._taa_values(scene)
        if scene.__dict__.pop("_taa_reset", False) and getattr(self, "_taa_key", None) is not None:
            _check_accum(self.lib.mr_scene_reset_history(self.handle), "mr_scene_reset_history")
        if frame is None:
            if getattr(self, "_taa_key", None) is not None:
                _check_accum(self.lib.mr_scene_set_temporal_aa(self.handle, None), "mr_scene_set_temporal_aa")
                self._taa_key = None
            return
        key = frame[:4]
        if getattr(self, "_taa_key", None) == key:
            return
        blend, matrices, background, class_of = key
        desc = fill_taa_desc(blend, np.frombuffer(matrices, dtype=np.float64), np.frombuffer(background, dtype=np.float64),
                             np.frombuffer(class_of, dtype=np.int32))
        _check_accum(self.lib.mr_scene_set_temporal_aa(self.handle, C.byref(desc)), "mr_scene_set_temporal_aa")
        self._taa_key = key

    def sync_motion_faces(self, scene):
        """``mr_scene_track_vertices`` and ``mr_scene_set_motion_faces`` for the frames enqueued from now on, behind
        ``sync_motion_blur``: tracking goes on with the first frame of a ``MotionBlur(deformation=True)`` and the frame's
        description (``issue_motion``) goes over whenever it is not the one last handed over.  A scene that never set the
        flag makes no call."""
        frame = None if self._motion_values(scene) is None else scene.__dict__.get("_motion_faces_frame")
        if frame is None:
            if getattr(self, "_motion_faces_key", None) is not None:
                _check_accum(self.lib.mr_scene_set_motion_faces(self.handle, None), "mr_scene_set_motion_faces")
                _check_accum(self.lib.mr_scene_track_vertices(self.handle, 0), "mr_scene_track_vertices")
                self._motion_faces_key = None
            return
        if getattr(self, "_motion_faces_key", None) is None:
            _check_accum(self.lib.mr_scene_track_vertices(self.handle, 1), "mr_scene_track_vertices")
        if getattr(self, "_motion_faces_key", None) == frame:
            return
        s_now, s_prev, deforming, prev_serial = frame
        desc = fill_motion_faces_desc(np.frombuffer(s_now, dtype=np.float64), np.frombuffer(s_prev, dtype=np.float64),
                                      np.frombuffer(deforming, dtype=np.int32), prev_serial)
        _check_accum(self.lib.mr_scene_set_motion_faces(self.handle, C.byref(desc)), "mr_scene_set_motion_faces")
        self._motion_faces_key = frame

    def note_motion_serial(self, scene):
        """Behind the enqueue of a frame with ``MotionBlur(deformation=True)``: the vertex serial of the state it was
        rendered from goes into the state it left (``MotionState.serial``), for the next frame's ``prev_serial``."""
        state = scene.__dict__.get("_motion_prev")
        if state is not None and state.bones is not None and scene.__dict__.get("_motion_replay") is None \
                and getattr(scene, "motion_blur", None) is not None:
            state.serial = int(self.lib.mr_scene_vertices_serial(self.handle))

    def sync_motion_blur(self, scene):
        """``mr_scene_set_motion_blur`` for the frames enqueued from now on, whenever the frame's motion (``issue_motion``)
        is not the one last handed over.  A scene that never had one makes no call."""
        frame = self._motion_values(scene)
        if frame is None:
            if getattr(self, "_motion_key", None) is not None:
                _check_accum(self.lib.mr_scene_set_motion_blur(self.handle, None), "mr_scene_set_motion_blur")
                self._motion_key = None
            return
        key = frame
        if getattr(self, "_motion_key", None) == key:
            return
        shutter, depth_map, matrices, background, class_of = frame
        desc = fill_motion_desc(depth_map, shutter, np.frombuffer(matrices, dtype=np.float64), np.frombuffer(background, dtype=np.float64),
                                np.frombuffer(class_of, dtype=np.int32))
        _check_accum(self.lib.mr_scene_set_motion_blur(self.handle, C.byref(desc)), "mr_scene_set_motion_blur")
        self._motion_key = key

    # -- frames ---------------------------------------------------------------------------
    @staticmethod
    def _frame_key(scene, shadows):
        """Everything ``pack_frame`` reads, cheaply: the camera objects (their MVP is cached for life, as in
        the reference) and the values of the few scalars and 3-vectors a caller may have reassigned."""
        cam, light = scene.camera, scene.light
        dbg = scene.debug_camera if scene.debug_camera is not None else cam

        def vec(x):
            return tuple(np.asarray(x, dtype=np.float64).ravel().tolist())
        # lights 1.. (Scene.add_light): everything pack_light reads of them, like the first light's below
        extras = tuple((id(x), vec(x.position), vec(x.center), vec(x.color), vec(x.ambient), str(x.light_type),
                        float(x.specular_strength), float(x.constant), float(x.linear), float(x.quadratic))
                       for x in list(getattr(scene, "lights", [light]))[1:])
        return (extras, id(cam), id(dbg), id(cam.__dict__.get("MVP")), id(dbg.__dict__.get("MVP")), tuple(scene.resolution),
                int(scene.system), int(scene.subsystem), bool(shadows), bool(cam.backface_culling), float(cam.near),
                float(cam.far), cam.x_offset, cam.y_offset, vec(cam.position), id(light), vec(light.position),
                vec(light.center), vec(light.color), vec(light.ambient), str(light.light_type),
                float(light.specular_strength), float(light.constant), float(light.linear), float(light.quadratic),
                getattr(scene, "supersample", 1), DeviceRenderer._ao_values(scene), DeviceRenderer._dof_values(scene), DeviceRenderer._motion_values(scene), DeviceRenderer._taa_values(scene), DeviceRenderer._bloom_values(scene), DeviceRenderer._light_shafts_values(scene), DeviceRenderer._tone_map_values(scene), DeviceRenderer._layers_values(scene), scene.__dict__.get("_sample_jitter"), id(scene.skybox) if scene.skybox is None or hasattr(scene.skybox, "textures") else vec(scene.skybox))

    def packed_frame(self, scene, shadows):
        """``pack_frame`` with a one-entry cache: a render loop that changes nothing between two frames does
        not rebuild the matrices and planes (150 us of NumPy scalar arithmetic, more than the frame takes)."""
        key = self._frame_key(scene, shadows)
        if self._packed[0] != key or "MVP" not in scene.camera.__dict__:
            self._pack_serial = getattr(self, "_pack_serial", 0) + 1
            self._packed = (None, pack_frame(scene, shadows))
            self._packed = (self._frame_key(scene, shadows), self._packed[1])    # the MVPs exist (and are cached) now
            # the key identifies cameras, light and matrices by id(): hold them while the entry lives, so that
            # CPython cannot hand their addresses to the objects of a later frame
            cam = scene.camera
            dbg = scene.debug_camera if scene.debug_camera is not None else cam
            self._packed_refs = (cam, dbg, cam.__dict__.get("MVP"), dbg.__dict__.get("MVP"), scene.light, scene.skybox,
                                 tuple(getattr(scene, "lights", ())))
        return self._packed[1]

    def sync_lights(self, pf):
        """The scene's extra lights (``mr_scene_set_extra_lights``) for the frames enqueued from now on; handed over
        again only when they changed."""
        n = len(pf.extra_lights)
        key, last = (getattr(self, "_pack_serial", 0), n), getattr(self, "_lights_key", None)
        if last == key or (n == 0 and (last is None or last[1] == 0)):
            self._lights_key = key
            return
        descs = (LightDesc * max(n, 1))(*[fill_light_desc(x) for x in pf.extra_lights])
        _check(self.lib.mr_scene_set_extra_lights(self.handle, descs if n else None, n), "mr_scene_set_extra_lights")
        self._lights_key = key

    def render(self, scene, shadows=True, row_band=None, keep_float=False, face_status=False, counters=True,
               keep_buffers=None, stripe=None, timing=True, overlay=False):
        """``mr_render``: returns the uint8 rows ``(rows, W, 3)`` as a NumPy array.

        ``counters=True`` (``MR_FRAME_COUNTERS``) also keeps the reference-equivalent fragment
        counters in ``last_stats`` and the reference's stencil values at uncovered pixels;
        ``keep_buffers`` (``MR_FRAME_KEEP_BUFFERS``, default: same as *counters*) also writes the
        z-buffer / stencil / winner map to device memory for ``read_z`` and friends -- what the
        parity tests and tools look at.  ``Scene.render`` passes ``False`` for both: only the
        frame is asked for, those buffers never leave the chip, and shadow quads that cannot pass
        the depth test are skipped (``last_stats`` then reports the fragment counters as -1).
        ``stripe=(index, count)`` renders the interleaved tile rows of one device of a
        multi-GPU split; the rows come back in the striped layout (``multigpu.unstripe``).
        ``timing=False`` (``MR_FRAME_NO_TIMING``) records no HIP events: each one costs a few
        microseconds between two kernels; ``last_stats['gpu_ms_*']`` are then 0.
        ``overlay=True`` (``MR_FRAME_OVERLAY``) draws the debug camera's frustum into the frame on the
        device, as the reference's ``render()`` always does (obj/core.py:638)."""
        desc, out = self._prepare(scene, shadows, row_band, keep_float, face_status, counters, keep_buffers, stripe, timing, overlay)
        stats = Stats()
        _check(self.lib.mr_render(self.handle, C.byref(desc), out.ctypes.data, C.byref(stats) if counters else None),
               "mr_render")
        self.note_motion_serial(scene)
        # a frame rendered for the frame's sake fetches its statistics only if somebody looks at them
        self._last_stats = stats.as_dict() if counters else None
        return out

    def _prepare(self, scene, shadows, row_band, keep_float, face_status, counters, keep_buffers, stripe, timing, overlay):
        """Everything ``render`` / ``render_async`` do before the library call: scene, skybox and overlay in step
        with the Python objects, the frame descriptor, a page-locked output array."""
        desc, shape = self._prepare_desc(scene, shadows, row_band, keep_float, face_status, counters, keep_buffers, stripe,
                                         timing, overlay)
        return desc, self._pinned.array(shape)

    @staticmethod
    def _is_partial(scene, row_band, stripe):
        """Whether a frame of *scene* with this row band (output rows) and stripe is part of a frame only."""
        return (stripe is not None and int(stripe[1]) > 1) or (
            row_band is not None and (int(row_band[0]) != 0 or int(row_band[1]) != int(scene.resolution[0])))

    def _prepare_desc(self, scene, shadows, row_band, keep_float, face_status, counters, keep_buffers, stripe, timing, overlay,
                      accumulating=False):
        """``_prepare`` without the output array: the frame descriptor and the shape of the frame's uint8 rows.  The
        sub-sample offset a ``temporal_aa`` gave the frame (``issue_motion``) lives until the descriptor holds it."""
        try:
            return self._prepare_issued(scene, shadows, row_band, keep_float, face_status, counters, keep_buffers, stripe, timing,
                                        overlay, accumulating)
        finally:
            if getattr(scene, "temporal_aa", None) is not None:
                scene.__dict__.pop("_sample_jitter", None)

    def _prepare_issued(self, scene, shadows, row_band, keep_float, face_status, counters, keep_buffers, stripe, timing, overlay,
                        accumulating):
        self.issue_motion(scene, partial=self._is_partial(scene, row_band, stripe), accumulating=accumulating)
        self.sync_scene(scene)
        self.sync_skybox(scene)
        pf = self.packed_frame(scene, shadows)
        if pf.extra_lights and face_status:
            raise ValueError("the per-face status is not available with more than one light")
        if pf.extra_lights and stripe is not None:
            raise ValueError("striped frames are not available with more than one light")
        # (the library renders such a frame and refuses to hand the status out: mr_read_face_status)
        partial = (stripe is not None and int(stripe[1]) > 1) or (
            row_band is not None and (int(row_band[0]) != 0 or int(row_band[1]) * pf.supersample != pf.height))
        if face_status and partial:
            raise ValueError("the per-face status needs the whole frame on one device (no row band, no stripes)")
        self.sync_lights(pf)
        if getattr(scene, "ambient_occlusion", None) is not None and partial:
            raise ValueError("ambient occlusion takes whole frames (no row band, no stripes): its taps cross the bands")
        if getattr(scene, "depth_of_field", None) is not None and partial:
            raise ValueError("depth of field takes whole frames (no row band, no stripes): its taps cross the bands")
        if getattr(scene, "bloom", None) is not None and partial:
            raise ValueError("bloom takes whole frames (no row band, no stripes): its taps cross the bands")
        if getattr(scene, "light_shafts", None) is not None and partial:
            raise ValueError("light shafts takes whole frames (no row band, no stripes): its taps cross the bands")
        if getattr(scene, "tone_map", None) is not None and partial:
            raise ValueError("tone mapping takes whole frames (no row band, no stripes): its exposure is metered from the whole frame")
        if getattr(scene, "layers", None) is not None and partial:
            raise ValueError("data layers takes whole frames (no row band, no stripes): its taps cross the bands")
        self._sync_post(scene, accumulating)
        if overlay:
            self.sync_overlay(scene)
        if keep_buffers is None:
            keep_buffers = counters
        dkey = (getattr(self, "_pack_serial", 0), row_band, keep_float, face_status, counters, keep_buffers, stripe, timing,
                overlay)
        if getattr(self, "_desc_key", None) != dkey:
            self._desc_cached = fill_frame_desc(pf, row_band, keep_float, face_status=face_status, counters=counters,
                                                keep_buffers=keep_buffers, stripe=stripe, no_timing=not timing,
                                                overlay=overlay)
            self._desc_key = dkey
        desc = self._desc_cached
        self._n_faces = sum(len(m._faces) for m in scene.models)
        ss = pf.supersample           # (the output of a supersampled frame: s x s samples per pixel)
        rows = (desc.row_end - desc.row_begin) // ss if stripe is None else stripe_out_rows(pf.height, stripe[1])
        self._frame = (pf.height, pf.width)          # the taps' shape: the sample grid
        return desc, (rows, pf.width // ss, 3)

    def _counts(self, fn, n):
        """An ``mr_debug_*`` entry that fills *n* int32 counters, as a tuple."""
        out = (C.c_int32 * n)()
        _check(fn(self.handle, out), fn.__name__)
        return tuple(int(x) for x in out)

    def _times(self, fn, names):
        """An ``mr_debug_*_times`` entry: device milliseconds, one per name."""
        buf = (C.c_float * len(names))()
        _check(fn(self.handle, buf), fn.__name__)
        return dict(zip(names, (float(v) for v in buf)))

    # -- the accumulation (Scene.accumulate) ------------------------------------------------
    def accum_begin(self):
        """``mr_accum_begin``: empties the scene's accumulation."""
        _check_accum(self.lib.mr_accum_begin(self.handle), "mr_accum_begin")
        self._accum_shapes = None

    def accum_add(self, scene, weight, shadows=True, overlay=False):
        """``mr_accum_add``: renders *scene* as it is now -- synchronised exactly as for ``render`` -- and adds its float
        frame, times *weight*, to the accumulation.  Nothing is copied to the host."""
        desc, shape = self._prepare_desc(scene, shadows, None, True, False, False, False, None, False, overlay, accumulating=True)
        _check_accum(self.lib.mr_accum_add(self.handle, C.byref(desc), float(weight)), "mr_accum_add")
        self._last_stats = None
        if getattr(self, "_accum_shapes", None) is None:
            self._accum_shapes = ((desc.height, desc.width, 3), shape)      # (the sum's, the result's)

    def accum_resolve(self, scale):
        """``mr_accum_resolve``: the sum as it stands, finalised with *scale*: uint8 ``(H, W, 3)``, row 0 = top."""
        if getattr(self, "_accum_shapes", None) is None:
            raise ValueError("mr_accum_resolve: nothing accumulated yet")
        out = self._pinned.array(self._accum_shapes[1])
        _check_accum(self.lib.mr_accum_resolve(self.handle, float(scale), out.ctypes.data), "mr_accum_resolve")
        return out

    def accum_read(self):
        """``mr_accum_read_f32``: the sum as it stands, float32 on the sample grid, rows bottom-up."""
        if getattr(self, "_accum_shapes", None) is None:
            raise ValueError("mr_accum_read_f32: nothing accumulated yet")
        out = np.empty(self._accum_shapes[0], dtype=np.float32)
        _check_accum(self.lib.mr_accum_read_f32(self.handle, out.ctypes.data), "mr_accum_read_f32")
        return out

    def accum_debug(self):
        """``mr_debug_accum``: (sub-frames added, sub-frames rendered again after an overflow, the sample grid's height
        and width)."""
        return self._counts(self.lib.mr_debug_accum, 4)

    ACCUM_TIME_NAMES = ("accum_add", "accum_resolve")

    def accum_times(self):
        """Device milliseconds of the last ``k_accum_add`` and the last ``k_accum_resolve`` (``mr_debug_accum_times``)."""
        return self._times(self.lib.mr_debug_accum_times, self.ACCUM_TIME_NAMES)

    # -- ambient obscurance (Scene.ambient_occlusion) ------------------------------------------
    def ao_debug(self):
        """``mr_debug_ao``: (frames that enqueued ``k_ao``, the last one's sample rows, its sample columns)."""
        return self._counts(self.lib.mr_debug_ao, 3)

    def ao_time(self):
        """Device milliseconds of the last ``k_ao`` (``mr_debug_ao_times``)."""
        return self._times(self.lib.mr_debug_ao_times, ("ao",))["ao"]

    # -- depth of field (Scene.depth_of_field) ---------------------------------------------------
    def dof_debug(self):
        """``mr_debug_dof``: (frames that enqueued ``k_dof``, the last one's sample rows, its sample columns)."""
        return self._counts(self.lib.mr_debug_dof, 3)

    def dof_time(self):
        """Device milliseconds of the last ``k_dof`` (``mr_debug_dof_times``)."""
        return self._times(self.lib.mr_debug_dof_times, ("dof",))["dof"]

    # -- motion blur (Scene.motion_blur) ---------------------------------------------------------
    def read_velocity(self):
        """``mr_read_velocity``: the last frame's velocity buffer U, float32 ``(Hs, Ws, 2)`` on the sample grid, rows
        bottom-up: the displacement of every sample, in samples, since the previous frame."""
        return self._tap(self.lib.mr_read_velocity, np.float32, (2,))

    def motion_debug(self):
        """``mr_debug_motion``: (frames that enqueued ``k_velocity`` and ``k_mblur``, the last one's sample rows, its columns)."""
        return self._counts(self.lib.mr_debug_motion, 3)

    MOTION_TIME_NAMES = ("velocity", "mblur")

    def motion_times(self):
        """Device milliseconds of the last ``k_velocity`` and the last ``k_mblur`` (``mr_debug_motion_times``)."""
        return self._times(self.lib.mr_debug_motion_times, self.MOTION_TIME_NAMES)

    # -- bloom (Scene.bloom) -----------------------------------------------------------------------
    def bloom_debug(self):
        """``mr_debug_bloom``: (frames that enqueued the pass, the last one's sample rows, its sample columns, its levels)."""
        return self._counts(self.lib.mr_debug_bloom, 4)

    BLOOM_TIME_NAMES = ("down", "up", "composite")

    def bloom_times(self):
        """Device milliseconds of the last bloom's down chain, up chain and composite (``mr_debug_bloom_times``)."""
        return self._times(self.lib.mr_debug_bloom_times, self.BLOOM_TIME_NAMES)

    # -- light shafts (Scene.light_shafts) -----------------------------------------------------------
    def light_shafts_debug(self):
        """``mr_debug_light_shafts``: (frames that enqueued the pass, the last one's sample rows, its sample columns, its halvings)."""
        return self._counts(self.lib.mr_debug_light_shafts, 4)

    LIGHT_SHAFTS_TIME_NAMES = ("source", "march", "composite")

    def light_shafts_times(self):
        """Device milliseconds of the last frame's ``k_shaft_source``, ``k_shaft_march`` and ``k_shaft_composite``
        (``mr_debug_light_shafts_times``)."""
        return self._times(self.lib.mr_debug_light_shafts_times, self.LIGHT_SHAFTS_TIME_NAMES)

    # -- data layers (Scene.layers) ---------------------------------------------------------------
    def read_layers(self):
        """``mr_read_layers`` for every layer the last frame computed: a dict name -> array on the sample grid ``(Hs, Ws[, c])``,
        rows bottom-up.  ``ValueError`` with the library's text where the last frame ran without the pass."""
        from ._pack import LAYER_CHANNELS, LAYER_DTYPES, LAYER_NAMES
        mask = self.layers_debug()[3]
        h, w = self._frame
        out = {}
        for i, name in enumerate(LAYER_NAMES):
            if mask >> i & 1 or not out and i == len(LAYER_NAMES) - 1:      # (no layer at all: the library says why)
                a = np.empty((h, w) + ((LAYER_CHANNELS[i],) if LAYER_CHANNELS[i] > 1 else ()), dtype=LAYER_DTYPES[i])
                _check_accum(self.lib.mr_read_layers(self.handle, i, a.ctypes.data), "mr_read_layers")
                out[name] = a
        return out

    def layers_debug(self):
        """``mr_debug_layers``: (frames that enqueued ``k_layers``, the last one's sample rows, its sample columns, its mask)."""
        return self._counts(self.lib.mr_debug_layers, 4)

    def layers_time(self):
        """Device milliseconds of the last ``k_layers`` (``mr_debug_layers_times``)."""
        return self._times(self.lib.mr_debug_layers_times, ("layers",))["layers"]

    def read_face_records(self):
        """``mr_debug_read_face_records``: the scene's static face records as the device holds them now, ``(face_pos,
        face_attr)`` as record arrays (``FACE_POS_DTYPES``, ``FACE_ATTR_DTYPE``): what ``host_layers`` takes."""
        info = (C.c_int32 * 2)()
        _check_accum(self.lib.mr_debug_read_face_records(self.handle, None, None, info), "mr_debug_read_face_records")
        pos = np.zeros(info[0], dtype=FACE_POS_DTYPES[bool(info[1])])
        attr = np.zeros(info[0], dtype=FACE_ATTR_DTYPE)
        _check_accum(self.lib.mr_debug_read_face_records(self.handle, pos.ctypes.data, attr.ctypes.data, info), "mr_debug_read_face_records")
        return pos, attr

    # -- tone mapping (Scene.tone_map) ------------------------------------------------------------
    def read_exposure(self):
        """``mr_read_exposure``: the exposure ``e`` of the last frame, which ran the pass, as a float32.  ``ValueError`` with
        the library's text where it did not."""
        out = np.zeros(1, dtype=np.float32)
        _check_accum(self.lib.mr_read_exposure(self.handle, out.ctypes.data), "mr_read_exposure")
        return out[0]

    def read_luminance_histogram(self):
        """``mr_read_luminance_histogram``: the 256 uint32 counts the last frame's exposure was metered from (bin 0, black,
        is metered out and reads 0).  ``ValueError`` with the library's text where nothing was metered."""
        out = np.zeros(256, dtype=np.uint32)
        _check_accum(self.lib.mr_read_luminance_histogram(self.handle, out.ctypes.data), "mr_read_luminance_histogram")
        return out

    def tone_map_debug(self):
        """``mr_debug_tone_map``: (frames that enqueued the pass, the last one's sample rows, its sample columns, the
        workgroups of its ``k_lum_hist`` -- 0 with a fixed exposure --, exposures handed over, 1 while the scene holds a
        previous exposure)."""
        return self._counts(self.lib.mr_debug_tone_map, 6)

    TONE_MAP_TIME_NAMES = ("lum_hist", "exposure", "tone_apply")

    def tone_map_times(self):
        """Device milliseconds of the last tone-mapped frame's ``k_lum_hist``, ``k_exposure`` and ``k_tone_apply``
        (``mr_debug_tone_map_times``)."""
        return self._times(self.lib.mr_debug_tone_map_times, self.TONE_MAP_TIME_NAMES)

    # -- temporal anti-aliasing (Scene.temporal_aa) ----------------------------------------------
    def read_history(self):
        """``mr_read_history``: the history as the scene holds it now -- the last complete temporal-AA frame as ``k_taa`` left
        it -- float32 ``(Hs, Ws, 3)`` on the sample grid, rows bottom-up.  ``ValueError`` with the library's text when
        there is none."""
        _, h, w = self.taa_debug()[:3]             # (the grid of the last frame with the pass: the history's, where there is one)
        out = np.empty((max(h, 1), max(w, 1), 3), dtype=np.float32)
        _check_accum(self.lib.mr_read_history(self.handle, out.ctypes.data), "mr_read_history")
        return out

    def taa_debug(self):
        """``mr_debug_taa``: (frames that enqueued ``k_taa``, the last one's sample rows, its columns, ``k_velocity`` launches
        made in front of ``k_taa``, histories handed over, 1 while the scene holds a history)."""
        return self._counts(self.lib.mr_debug_taa, 6)

    TAA_TIME_NAMES = ("velocity", "taa")

    def taa_times(self):
        """Device milliseconds of the last temporal-AA frame's ``k_velocity`` and ``k_taa`` (``mr_debug_taa_times``)."""
        return self._times(self.lib.mr_debug_taa_times, self.TAA_TIME_NAMES)

    def read_prev_vertices(self, n_verts):
        """``mr_debug_read_prev_vertices``: the library's snapshot of the vertices, float64 ``(n_verts, 4)``."""
        out = np.empty((int(n_verts), 4), dtype=np.float64)
        _check_accum(self.lib.mr_debug_read_prev_vertices(self.handle, out.ctypes.data), "mr_debug_read_prev_vertices")
        return out

    def vertices_serial(self):
        """``mr_scene_vertices_serial``: how many states the device's vertices have held."""
        return int(self.lib.mr_scene_vertices_serial(self.handle))

    def motion_faces_debug(self):
        """``mr_debug_motion_faces``: (frames that ran the per-face pass, frames that skipped it, the last pass's records,
        snapshots of the vertices taken)."""
        return self._counts(self.lib.mr_debug_motion_faces, 4)

    MOTION_FACES_TIME_NAMES = ("face_homography", "velocity_faces")

    def motion_faces_times(self):
        """Device milliseconds of the last ``k_face_homography`` and the last ``k_velocity_faces``."""
        return self._times(self.lib.mr_debug_motion_faces_times, self.MOTION_FACES_TIME_NAMES)

    ASYNC_LANES = 4

    def render_async(self, scene, lane, shadows=True, overlay=False):
        """``mr_render_async``: the frame-only render of ``Scene.render`` enqueued on *lane*; returns the (page-locked)
        array the frame will land in.  ``render_wait(lane)`` blocks until it has."""
        desc, out = self._prepare(scene, shadows, None, False, False, False, False, None, False, overlay)
        _check(self.lib.mr_render_async(self.handle, C.byref(desc), out.ctypes.data, int(lane)), "mr_render_async")
        self.note_motion_serial(scene)
        self._last_stats = None
        return out

    def render_wait(self, lane):
        """True when the lane's frame is complete in its array; False when it overflowed a work list (the lists
        have been grown: render the frame again)."""
        rc = self.lib.mr_render_wait(self.handle, int(lane), None)
        if rc == MR_E_OVERFLOW:
            return False
        _check(rc, "mr_render_wait")
        return True

    @property
    def last_stats(self):
        if self._last_stats is None and self.handle:
            st = Stats()
            _check(self.lib.mr_get_stats(self.handle, C.byref(st)), "mr_get_stats")
            self._last_stats = st.as_dict()
        return self._last_stats

    @last_stats.setter
    def last_stats(self, value):
        self._last_stats = value

    def render_device(self, scene, d_out_ptr, stream_ptr=0, shadows=True, row_band=None, light_timing=False,
                      counters=False, stripe=None, no_timing=False, overlay=False):
        """``mr_render_device``: enqueue a frame whose uint8 band lands at device pointer *d_out_ptr*.  With *overlay*
        a device that renders the whole frame draws the debug frustum; one that renders part of it appends the state of
        the touched pixels it owns to its rows (``overlay_state_bytes``, ``overlay_apply``)."""
        if getattr(scene, "temporal_aa", None) is not None:
            raise ValueError("temporal_aa frames are rendered by render() / render_async(): their return hands the history "
                             "over, and a frame enqueued on a caller's stream has none")
        tm = getattr(scene, "tone_map", None)
        if tm is not None and tm.adaptive:
            raise ValueError("frames of an adaptive tone_map (speed < 1) are rendered by render() / render_async(): their return "
                             "hands the exposure over, and a frame enqueued on a caller's stream has none")
        if getattr(scene, "layers", None) is not None:
            raise ValueError("layers frames are rendered by render() / render_async(): their return says which frame "
                             "read_layers() reads, and a frame enqueued on a caller's stream has none")
        self.issue_motion(scene, partial=self._is_partial(scene, row_band, stripe))
        self.sync_scene(scene)
        self.sync_skybox(scene)
        pf = self.packed_frame(scene, shadows)
        if pf.extra_lights and stripe is not None:
            raise ValueError("striped frames are not available with more than one light")
        self.sync_lights(pf)
        self._sync_post(scene)
        if overlay:
            self.sync_overlay(scene)
        desc = fill_frame_desc(pf, row_band, False, light_timing, counters=counters, stripe=stripe, no_timing=no_timing,
                               overlay=overlay)
        _check(self.lib.mr_render_device(self.handle, C.byref(desc), C.c_void_p(d_out_ptr),
                                         C.c_void_p(stream_ptr)), "mr_render_device")
        self.note_motion_serial(scene)
        self._frame = (pf.height, pf.width)
        self._desc = desc
        return desc

    @staticmethod
    def with_timing(desc, mode):
        """Copy of a frame descriptor with its event marks set to *mode*: "all" stages, "light" (frame +
        tile kernel) or "none"."""
        out = FrameDesc.from_buffer_copy(desc)
        out.flags &= ~(FRAME_LIGHT_TIMING | FRAME_NO_TIMING)
        out.flags |= {"all": 0, "light": FRAME_LIGHT_TIMING, "none": FRAME_NO_TIMING}[mode]
        return out

    def enqueue(self, desc, d_out_ptr, stream_ptr=0):
        """Re-issue a prepared frame descriptor (no Python-side packing in the timed loop)."""
        _check(self.lib.mr_render_device(self.handle, C.byref(desc), C.c_void_p(d_out_ptr),
                                         C.c_void_p(stream_ptr)), "mr_render_device")

    def overlay_state_bytes(self):
        """Bytes a device of a split frame appends to its rows for the overlay (``mr_overlay_state_bytes``)."""
        return int(_check(self.lib.mr_overlay_state_bytes(self.handle), "mr_overlay_state_bytes"))

    def overlay_apply(self, d_parts_ptr, part_stride, state_offset, world, striped, system, d_frame_ptr, stream_ptr=0):
        """``mr_overlay_apply``: replay the overlay on the frame assembled from *world* parts."""
        _check(self.lib.mr_overlay_apply(self.handle, C.c_void_p(d_parts_ptr), int(part_stride), int(state_offset), int(world),
                                         int(bool(striped)), int(system), C.c_void_p(d_frame_ptr), C.c_void_p(stream_ptr)),
               "mr_overlay_apply")

    def set_list_capacities(self, small_pairs=0, big_pairs=0, quads=0, work=0):
        """Where the per-tile work lists start (they grow on overflow); a tuning / test hook."""
        _check(self.lib.mr_scene_set_list_capacities(self.handle, small_pairs, big_pairs, quads, work),
               "mr_scene_set_list_capacities")

    def overflowed(self):
        """True when a frame enqueued with ``render_device`` overflowed a work list (the lists have then
        been grown and the frame must be enqueued again); synchronises the device."""
        st = Stats()
        rc = self.lib.mr_get_stats(self.handle, C.byref(st))
        if rc == MR_E_OVERFLOW:
            return True
        _check(rc, "mr_get_stats")
        self.last_stats = st.as_dict()
        return False

    def stats(self):
        st = Stats()
        _check(self.lib.mr_get_stats(self.handle, C.byref(st)), "mr_get_stats")
        self.last_stats = st.as_dict()
        return self.last_stats

    KERNEL_TIME_NAMES = ("vertex_mfma", "setup", "bin_work", "tile", "frame")

    def kernel_times(self, n_frames):
        """Average per-stage device milliseconds over the last *n_frames* frames (syncs)."""
        buf = (C.c_float * 5)()
        n = _check(self.lib.mr_get_kernel_times(self.handle, int(n_frames), buf, 5), "mr_get_kernel_times")
        return dict(zip(self.KERNEL_TIME_NAMES, (float(v) for v in buf))), n

    def stream_kernel_times(self, stream_ptr, n_frames):
        """The same over the marked frames of one stream; returns (dict, frames averaged)."""
        buf = (C.c_float * 5)()
        n = _check(self.lib.mr_get_stream_kernel_times(self.handle, C.c_void_p(stream_ptr), int(n_frames), buf, 5),
                   "mr_get_stream_kernel_times")
        return dict(zip(self.KERNEL_TIME_NAMES, (float(v) for v in buf))), n

    # -- debug taps -----------------------------------------------------------------------
    def _tap(self, fn, dtype, extra=()):
        h, w = self._frame
        out = np.empty((h, w) + tuple(extra), dtype=dtype)
        _check(fn(self.handle, out.ctypes.data), fn.__name__)
        return out

    def read_z(self):
        return self._tap(self.lib.mr_read_z, np.float64)

    def read_stencil(self, light=0):
        """The stencil buffer of light *light* of the last frame (0: ``scene.light``)."""
        h, w = self._frame
        out = np.empty((h, w), dtype=np.int16)
        _check(self.lib.mr_read_stencil_light(self.handle, int(light), out.ctypes.data), "mr_read_stencil_light")
        return out

    def read_winner(self):
        return self._tap(self.lib.mr_read_winner, np.int32)

    def read_frame_f32(self):
        return self._tap(self.lib.mr_read_frame_f32, np.float32, (3,))

    def read_tile_records(self):
        """Per-tile diagnostics of the tile kernel: (n_tiles, 12) uint32, see mi355rast.h."""
        n = _check(self.lib.mr_debug_read_tile_records(self.handle, (C.c_uint32 * TILE_RECORD_WORDS)(), 0),
                   "mr_debug_read_tile_records")
        out = np.empty((max(n, 1), TILE_RECORD_WORDS), dtype=np.uint32)
        _check(self.lib.mr_debug_read_tile_records(self.handle, out.ctypes.data, n), "mr_debug_read_tile_records")
        return out[:n]

    def clusters_culled(self):
        """Clusters of 64 faces the last frame's set-up dropped whole (counted only under MR_CLUSTER_CULL=count)."""
        return int(_check(self.lib.mr_debug_clusters_culled(self.handle), "mr_debug_clusters_culled"))

    def quad_walks(self):
        """``mr_debug_quad_walks`` of the last (counted, single-light) frame: ((quad, row) span items, (quad, strip)
        walks, those of the strip walks with a polygon of more than four vertices, those with a non-finite edge value)."""
        out = (C.c_uint32 * 4)()
        _check(self.lib.mr_debug_quad_walks(self.handle, out), "mr_debug_quad_walks")
        return tuple(int(x) for x in out)

    def pair_log(self):
        """``mr_debug_pair_log`` of the last (counted) frame: (covered samples of small pairs that the winners' sweep
        answered from the lanes' logs, samples it walked again)."""
        out = (C.c_uint32 * 2)()
        _check(self.lib.mr_debug_pair_log(self.handle, out), "mr_debug_pair_log")
        return tuple(int(x) for x in out)

    def big_tri_rejects(self):
        """``mr_debug_big_tri_rejects`` of the last (counted) frame: (large triangle, tile) pairs ``k_bin_work`` left out of
        the tile lists because the triangle can cover no sample of the tile (``MR_BIG_TRI_REJECT=0``: none)."""
        return int(_check(self.lib.mr_debug_big_tri_rejects(self.handle), "mr_debug_big_tri_rejects"))

    def sil_cache(self):
        """Silhouette cache: (path of the last frame with shadows: 0 fused / 1 captured / 2 cached / -1 none, entries it
        read from the cache, captures started so far, usable buffers); see mi355rast.h."""
        return self._counts(self.lib.mr_debug_sil_cache, 4)

    def force_full(self, on=True):
        """``mr_debug_force_full``: every later frame of the scene takes the general kernels (k_setup_full, k_tile_full);
        ``False`` returns to the rule (frame-only kernels unless the frame is counted, asks for the per-face status or
        the scene has a ``depth_test=False`` model)."""
        _check(self.lib.mr_debug_force_full(self.handle, 1 if on else 0), "mr_debug_force_full")

    def frame_path(self):
        """``mr_debug_frame_path`` of the last frame: dict of bools ``full`` (general kernels, else frame-only), ``split``,
        ``ss``, ``ml`` (the tile kernel's instantiation) and ``ordered`` (heaviest-first order)."""
        out = (C.c_int32 * 5)()
        _check(self.lib.mr_debug_frame_path(self.handle, out), "mr_debug_frame_path")
        return dict(zip(("full", "split", "ss", "ml", "ordered"), (bool(x) for x in out)))

    def pose_counters(self):
        """``mr_debug_pose``: (full commits of the scene so far, pose passes so far, posed models, vertices the last
        pass wrote)."""
        return self._counts(self.lib.mr_debug_pose, 4)

    def skin_counters(self):
        """``mr_debug_skin``: (models that have bones, bone matrices the last pose pass uploaded, vertices and normals it
        skinned)."""
        return self._counts(self.lib.mr_debug_skin, 4)

    def morph_counters(self):
        """``mr_debug_morph``: (models that have morph weights, targets the last pose pass used, vertices and normals it
        morphed, entries -- padding included -- of the contribution lists on the device)."""
        return self._counts(self.lib.mr_debug_morph, 5)

    def auto_normals_counters(self):
        """``mr_debug_auto_normals``: (models whose normals the last pose pass rebuilt, normals it wrote, entries --
        padding included -- of the face lists on the device, normals among those written that kept their authored value)."""
        return self._counts(self.lib.mr_debug_auto_normals, 4)

    AUTO_NORMALS_TIME_NAMES = ("auto_normals",)

    def auto_normals_times(self):
        """Device milliseconds of ``k_auto_normals`` in the last pose pass (``mr_debug_auto_normals_times``)."""
        return self._times(self.lib.mr_debug_auto_normals_times, self.AUTO_NORMALS_TIME_NAMES)

    MORPH_TIME_NAMES = ("morph_vertices", "morph_normals")

    def morph_times(self):
        """Device milliseconds of the two morph kernels of the last pose pass (``mr_debug_morph_times``)."""
        return self._times(self.lib.mr_debug_morph_times, self.MORPH_TIME_NAMES)

    SKIN_TIME_NAMES = ("skin_vertices", "skin_normals")

    def skin_times(self):
        """Device milliseconds of the two skin kernels of the last pose pass that had a skin to apply
        (``mr_debug_skin_times``)."""
        return self._times(self.lib.mr_debug_skin_times, self.SKIN_TIME_NAMES)

    POSE_TIME_NAMES = ("pose_vertices", "face_normals", "edge_normals", "face_static", "clusters")

    def pose_times(self):
        """Device milliseconds of the five kernels of the last pose pass (``mr_debug_pose_times``)."""
        return self._times(self.lib.mr_debug_pose_times, self.POSE_TIME_NAMES)

    POSE_NORMALS_TIME_NAMES = ("pose_normals", "pose_texels")

    def pose_normals_times(self):
        """Device milliseconds of the two kernels of the last pose pass that had normal matrices to apply
        (``mr_debug_pose_normals_times``)."""
        return self._times(self.lib.mr_debug_pose_normals_times, self.POSE_NORMALS_TIME_NAMES)

    def read_clusters(self):
        """The per-cluster records of the scene (``mr_debug_read_clusters``): a structured array with ``lo``, ``hi``,
        ``axis`` (3 float32 each), ``cos_half``, ``sin_half``."""
        dtype = np.dtype([("lo", np.float32, 3), ("hi", np.float32, 3), ("axis", np.float32, 3), ("cos_half", np.float32),
                          ("sin_half", np.float32), ("pad", np.uint32, 5)])
        n = _check(self.lib.mr_debug_read_clusters(self.handle, (C.c_uint32 * 16)(), 0), "mr_debug_read_clusters")
        out = np.zeros(max(n, 1), dtype=dtype)
        _check(self.lib.mr_debug_read_clusters(self.handle, out.ctypes.data, n), "mr_debug_read_clusters")
        return out[:n]

    def read_tile_order(self):
        """The order in which the last frame's tile kernel took its tiles: (n_tiles,) uint32."""
        n = _check(self.lib.mr_debug_read_tile_order(self.handle, (C.c_uint32 * 1)(), 0), "mr_debug_read_tile_order")
        out = np.empty(max(n, 1), dtype=np.uint32)
        _check(self.lib.mr_debug_read_tile_order(self.handle, out.ctypes.data, n), "mr_debug_read_tile_order")
        return out[:n]

    def read_face_status(self):
        """One ``Errors`` value (0 = rendered) per face, models concatenated in scene order."""
        out = np.empty(max(self._n_faces, 1), dtype=np.uint8)
        _check(self.lib.mr_read_face_status(self.handle, out.ctypes.data), "mr_read_face_status")
        return out[:self._n_faces]

    def read_silhouette(self, light=0):
        """Silhouette edges of light *light* of the last frame as (model, a, b) rows (0: ``scene.light``)."""
        n = _check(self.lib.mr_read_silhouette_light(self.handle, int(light), None, 0), "mr_read_silhouette_light")
        out = np.empty((max(n, 1), 3), dtype=np.int32)
        _check(self.lib.mr_read_silhouette_light(self.handle, int(light), out.ctypes.data, n), "mr_read_silhouette_light")
        return out[:n]

    def close(self):
        if self.handle:
            self.lib.mr_scene_destroy(self.handle)
            self.handle = None
            self._pinned.close()

    def __del__(self):  # best effort
        try:
            self.close()
        except Exception:
            pass
