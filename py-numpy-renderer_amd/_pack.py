"""Scene -> flat arrays.

Turns the ``Scene`` object graph into the plain arrays and scalars the C ABI takes
(``include/mi355rast.h``): per-frame constants in float64 and, per model, the vertex /
uv / normal / index arrays with every index made non-negative and every material group
resolved to a small record.  Pure host bookkeeping; no rasterisation happens here.
"""
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from .lightning import Lightning

_DEFAULT_BACKGROUND = (64 / 255, 0.5, 198 / 255)       # obj/core.py:600


@dataclass
class PackedMaterial:
    kd: np.ndarray
    ks255: np.ndarray
    ns: float
    tex_kd: int = -1
    tex_norm: int = -1
    tex_ks: int = -1
    norm_tangent: bool = False


@dataclass
class PackedModel:
    vertices: np.ndarray            # float64 (V, 4)
    uv: Optional[np.ndarray]        # float32 (T, 3)
    normals: Optional[np.ndarray]   # float32 (N, 3)
    faces: np.ndarray               # int32 (F, 3, 4), all >= 0
    materials: List[PackedMaterial]
    vertices_are_f32: bool
    clip: bool
    depth_test: bool
    # (F, 3) int32: the vertex column of Model._faces as loaded (negative = relative).  The reference's
    # silhouette set identifies an edge by these raw values (obj/triangular.py:286-302); None when they
    # equal faces[..., 0]
    edge_ids: Optional[np.ndarray] = None


@dataclass
class PackedLight:
    """One light as the C ABI takes it (``mr_light_desc``; for ``scene.light`` the same fields of ``mr_frame_desc``)."""
    light_type: int
    light_pos: np.ndarray
    light_dir: np.ndarray
    light_color: np.ndarray
    light_ambient: np.ndarray
    specular_strength: float
    att_constant: float
    att_linear: float
    att_quadratic: float
    spot_edge0: float
    spot_edge1: float


MAX_LIGHTS = 4


@dataclass
class PackedFrame:
    width: int
    height: int
    system: int
    backface_culling: bool
    light_type: int
    shadows: bool
    mvp: np.ndarray
    viewport: np.ndarray
    debug_mvp: np.ndarray
    frustum_planes: np.ndarray
    z_near: float
    z_far: float
    camera_pos: np.ndarray
    light_pos: np.ndarray
    light_dir: np.ndarray
    light_color: np.ndarray
    light_ambient: np.ndarray
    specular_strength: float
    att_constant: float
    att_linear: float
    att_quadratic: float
    spot_edge0: float
    spot_edge1: float
    background: np.ndarray
    sky_tri: Optional[np.ndarray] = None      # (2, 3, 2) int32, cubemap skybox only
    sky_rays: Optional[np.ndarray] = None     # (2, 3, 3) float64
    # samples per output pixel and axis (Scene.supersample).  width / height / viewport / sky_* above are then the
    # sample grid's: the frame of a twin scene at (s H, s W) with its camera's offsets times s
    supersample: int = 1
    # lights 1.. of the frame (Scene.add_light), scene.light being light 0: the fields above
    extra_lights: tuple = ()


@dataclass
class PackedScene:
    frame: PackedFrame
    models: List[PackedModel]
    textures: List[np.ndarray] = field(default_factory=list)   # float32 (h, w, 3), C order


def _vec3(x):
    v = np.asarray(x, dtype=np.float64).ravel()
    if v.size == 1:
        v = np.repeat(v, 3)
    if v.size != 3:
        raise ValueError(f"expected a 3-vector, got shape {np.shape(x)}")
    return np.ascontiguousarray(v)


def _wrap(idx, n, what):
    """Python-style negative indices -> non-negative, bounds-checked."""
    idx = np.where(idx < 0, idx + n, idx)
    if idx.size and (idx.min() < 0 or idx.max() >= n):
        raise IndexError(f"{what} index out of range for {n} entries")
    return idx


SUPERSAMPLE_FACTORS = (1, 2, 4)


def check_supersample(value):
    """``Scene.supersample``: 1, 2 or 4 samples per output pixel and axis (s divides the 16 x 16 tile, and s * s is a
    power of two: a block of equal colours resolves to exactly that colour)."""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or int(value) not in SUPERSAMPLE_FACTORS:
        raise ValueError(f"supersample must be one of {SUPERSAMPLE_FACTORS}, got {value!r}")
    return int(value)


def check_accum_factor(value, what):
    """A sub-frame's weight or the scale of ``Accumulation.result``: a real number that is finite and > 0 once it is a
    float32 -- what the device multiplies with.  Returned as a Python float (the value as given)."""
    if isinstance(value, (bool, str, bytes)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"{what} must be a real number, got {value!r}")
    with np.errstate(over="ignore"):
        as_f32 = np.float32(value)
    if not np.isfinite(as_f32) or not as_f32 > 0:
        raise ValueError(f"{what} must be finite and > 0 as float32, got {value!r}")
    return float(value)


def default_accum_scale(weight_sum):
    """``float32(1 / sum of the weights as given)``, the division in float64."""
    return float(np.float32(1.0 / float(weight_sum)))


def _ao_number(value, what, lowest_allowed):
    """One parameter of an ``AmbientOcclusion`` as a Python float: a real number that is finite and > 0 (``>= 0`` with
    *lowest_allowed*) once it is a float32 -- what the device computes with."""
    if isinstance(value, (bool, str, bytes)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise TypeError(f"ambient occlusion: {what} must be a real number, got {value!r}")
    with np.errstate(over="ignore"):
        as_f32 = np.float32(value)
    if not np.isfinite(as_f32) or as_f32 < 0 or (as_f32 == 0 and not lowest_allowed):
        raise ValueError(f"ambient occlusion: {what} must be finite and {'>= 0' if lowest_allowed else '> 0'} as float32, got {value!r}")
    return float(value)


def check_ambient_occlusion(radius, strength, depth_range, bias):
    """The parameters of an ``AmbientOcclusion`` as Python floats ``(radius, strength, depth_range, bias)``, the defaults
    filled in: ``depth_range = 3 * radius``, ``bias = depth_range / 32``."""
    radius = _ao_number(radius, "radius", False)
    strength = _ao_number(strength, "strength", False)
    if np.float32(strength) > 8:
        raise ValueError(f"ambient occlusion: strength must be <= 8, got {strength!r}")
    depth_range = _ao_number(3.0 * radius if depth_range is None else depth_range, "depth_range", False)
    bias = _ao_number(depth_range / 32.0 if bias is None else bias, "bias", True)
    if not np.isfinite(np.float32(1.0 / radius)):
        raise ValueError(f"ambient occlusion: radius must be finite and > 0 as float32, got {radius!r}")
    return radius, strength, depth_range, bias


def depth_map(scene, camera):
    """``(m0, m1, m2, m3)`` float64 with ``z_e = (m0 * Z + m1) / (m2 * Z + m3)``: the eye depth, > 0 in front of the
    camera, of a z-buffer value Z of a frame of *scene* seen through *camera*.  The inverse of the chain the reference
    applies to a point ``z_e`` on the view axis (row vectors, P the projection, V the viewport, n / f near / far)::

        z_c = z_e * P[2,2] + P[3,2]      w_c = z_e * P[2,3] + P[3,3]      ndc = z_c / w_c
        scr = ndc * V[2,2] + V[3,2]      Z = 2 n f / ((f + n) - scr * (f - n))

    Every step is a Moebius map ``(a x + b) / (c x + d)``, so the chain is the product of three 2x2 matrices and its
    inverse their adjugate (scaled by its largest entry, which changes no quotient).  The sign: ``z_e`` is negative in
    front of a right-handed camera and positive in front of a left-handed one; a perspective camera shows the points with
    ``w_c > 0``, so the depth is ``z_e * sign(P[2,3])``; for an orthographic one (``w_c`` constant) it is the sign under
    which the middle of [n, f] lands nearer to the middle of the ndc range.  The matrices are *camera*'s own
    (``projection`` at the scene's aspect ratio, ``viewport``'s z row, which a supersampled grid shares)."""
    P = np.asarray(camera.projection, dtype=np.float64)
    V = np.asarray(camera.viewport, dtype=np.float64)
    n, f = float(camera.near), float(camera.far)
    project = np.array([[P[2, 2], P[3, 2]], [P[2, 3], P[3, 3]]])
    to_screen = np.array([[V[2, 2], V[3, 2]], [0.0, 1.0]])
    linearize = np.array([[0.0, 2 * n * f], [-(f - n), f + n]])
    (a, b), (c, d) = linearize @ to_screen @ project
    sign = depth_sign(camera)
    m = np.array([sign * d, -sign * b, -c, a], dtype=np.float64)
    largest = np.abs(m).max()
    if not np.isfinite(m).all() or largest == 0:
        raise ValueError("ambient occlusion: the camera's projection gives no finite depth map")
    return tuple(float(x) for x in m / largest)


def ao_constants(scene, camera=None):
    """What ``mr_ao_desc`` carries for a frame of *scene* (``ambient_occlusion`` set) through *camera* (default: the
    scene's): ``(depth_map, k, perspective)`` with ``k = float32(radius * 0.5 * Hs * |P[1,1]|)`` evaluated in float64,
    Hs the sample grid's height."""
    camera = scene.camera if camera is None else camera
    ao = scene.ambient_occlusion
    P = np.asarray(camera.projection, dtype=np.float64)
    s = check_supersample(getattr(scene, "supersample", 1))
    rows = s * int(scene.resolution[0])
    k = float(np.float32(ao.radius * 0.5 * rows * abs(float(P[1, 1]))))
    return depth_map(scene, camera), k, int(P[2, 3] != 0)


def check_depth_of_field(focus, lens_radius):
    """The parameters of a ``DepthOfField`` as ``(focus, lens_radius)``: Python floats that are finite and > 0 as
    float32; ``focus`` may be ``None`` (the eye depth of the camera's ``center``, per view)."""
    def number(value, what):
        if isinstance(value, (bool, str, bytes)) or not isinstance(value, (int, float, np.integer, np.floating)):
            raise TypeError(f"depth of field: {what} must be a real number, got {value!r}")
        with np.errstate(over="ignore"):
            as_f32 = np.float32(value)
        if not np.isfinite(as_f32) or as_f32 <= 0:
            raise ValueError(f"depth of field: {what} must be finite and > 0 as float32, got {value!r}")
        return float(value)
    return (None if focus is None else number(focus, "focus")), number(lens_radius, "lens_radius")


def dof_constants(scene, camera=None):
    """What ``mr_dof_desc`` carries for a frame of *scene* (``depth_of_field`` set) through *camera* (default: the
    scene's): ``(depth_map, kf, perspective, focus)`` with ``focus`` the ``DepthOfField``'s own or, for ``None``, the eye
    depth of the camera's ``center``, ``|center - position|``, and ``kf = float32(lens_radius * 0.5 * Hs * |P[1,1]| /
    focus)`` evaluated in float64, Hs the sample grid's height."""
    camera = scene.camera if camera is None else camera
    dof = scene.depth_of_field
    focus = dof.focus
    if focus is None:
        focus = float(np.linalg.norm(np.asarray(camera.center, dtype=np.float64).ravel()[:3]
                                     - np.asarray(camera.position, dtype=np.float64).ravel()[:3]))
    P = np.asarray(camera.projection, dtype=np.float64)
    s = check_supersample(getattr(scene, "supersample", 1))
    rows = s * int(scene.resolution[0])
    with np.errstate(all="ignore"):
        kf = float(np.float32(np.float64(dof.lens_radius) * 0.5 * rows * abs(float(P[1, 1])) / np.float64(focus)))
    if not (np.isfinite(np.float32(focus)) and np.float32(focus) > 0 and np.isfinite(kf) and kf > 0):
        raise ValueError(f"depth of field: focus {focus!r} and lens_radius {dof.lens_radius!r} give no finite circle of "
                         f"confusion > 0 for this view (kf = {kf!r})")
    return depth_map(scene, camera), kf, int(P[2, 3] != 0), float(focus)


def check_bloom(threshold, intensity, levels):
    """The parameters of a ``Bloom`` as ``(threshold, intensity, levels)``: *threshold* a Python float that is finite and in
    [0, 1) as float32, *intensity* one that is finite and > 0 as float32, *levels* an int in 1 .. 6."""
    def number(value, what):
        if isinstance(value, (bool, str, bytes)) or not isinstance(value, (int, float, np.integer, np.floating)):
            raise TypeError(f"bloom: {what} must be a real number, got {value!r}")
        with np.errstate(over="ignore"):
            return np.float32(value)
    t, g = number(threshold, "threshold"), number(intensity, "intensity")
    if not np.isfinite(t) or not (0 <= t < 1):
        raise ValueError(f"bloom: threshold must lie in [0, 1) as float32, got {threshold!r}")
    if not np.isfinite(g) or g <= 0:
        raise ValueError(f"bloom: intensity must be finite and > 0 as float32, got {intensity!r}")
    if isinstance(levels, (bool, np.bool_)) or not isinstance(levels, (int, np.integer)):
        raise TypeError(f"bloom: levels must be an int, got {levels!r}")
    if not 1 <= levels <= 6:
        raise ValueError(f"bloom: levels must lie in 1 .. 6, got {levels!r}")
    return float(threshold), float(intensity), int(levels)


def bloom_constants(scene):
    """What ``mr_bloom_desc`` carries for a frame of *scene* (``bloom`` set): ``(threshold, gain, levels)`` with ``gain =
    float32(intensity / levels)`` evaluated in float64 -- the glow is a sum of ``levels`` terms, so its strength does not
    grow with its width -- and ``levels + log2(supersample)`` levels on the sample grid: the glow is as wide in output
    pixels at any ``supersample``."""
    bloom = scene.bloom
    s = check_supersample(getattr(scene, "supersample", 1))
    gain = float(np.float32(np.float64(bloom.intensity) / np.float64(bloom.levels)))
    if not (np.isfinite(gain) and gain > 0):
        raise ValueError(f"bloom: intensity {bloom.intensity!r} over {bloom.levels} levels gives no gain > 0 as float32")
    return bloom.threshold, gain, bloom.levels + {1: 0, 2: 1, 4: 2}[s]


def check_light_shafts(light, intensity, density, decay, samples, threshold, halvings):
    """The parameters of a ``LightShafts`` as ``(light, intensity, density, decay, samples, threshold, halvings)``: *light* an
    int >= 0 (an index into ``scene.lights``, looked up when a frame is issued), *intensity* and *density* Python floats
    that are finite and > 0 as float32, *decay* one in (0, 1] as float32, *samples* an int in 1 .. 128, *threshold* a float
    in [0, 1) as float32, *halvings* 1 or 2."""
    def number(value, what):
        if isinstance(value, (bool, str, bytes)) or not isinstance(value, (int, float, np.integer, np.floating)):
            raise TypeError(f"light shafts: {what} must be a real number, got {value!r}")
        with np.errstate(over="ignore"):
            return np.float32(value)

    def integer(value, what, lo, hi):
        if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
            raise TypeError(f"light shafts: {what} must be an int, got {value!r}")
        if not lo <= value <= hi:
            raise ValueError(f"light shafts: {what} must lie in {lo} .. {hi}, got {value!r}")
        return int(value)

    light = integer(light, "light", 0, 2 ** 31 - 1)
    for value, what in ((intensity, "intensity"), (density, "density")):
        v = number(value, what)
        if not np.isfinite(v) or v <= 0:
            raise ValueError(f"light shafts: {what} must be finite and > 0 as float32, got {value!r}")
    d = number(decay, "decay")
    if not np.isfinite(d) or not (0 < d <= 1):
        raise ValueError(f"light shafts: decay must lie in (0, 1] as float32, got {decay!r}")
    samples = integer(samples, "samples", 1, 128)
    t = number(threshold, "threshold")
    if not np.isfinite(t) or not (0 <= t < 1):
        raise ValueError(f"light shafts: threshold must lie in [0, 1) as float32, got {threshold!r}")
    halvings = integer(halvings, "halvings", 1, 2)
    return light, float(intensity), float(density), float(decay), samples, float(threshold), halvings


def light_shafts_weights(decay, samples):
    """The march's weights: ``w_0 = 1``, ``w_{i+1} = w_i * decay`` in float64 -- a running product, no ``pow``: every host
    sends the same table -- divided by their sum and rounded to float32.  They sum to 1: more samples is not more light."""
    w = np.empty(int(samples), dtype=np.float64)
    value = np.float64(1.0)
    for i in range(int(samples)):
        w[i] = value
        value = value * np.float64(decay)
    return (w / w.sum()).astype(np.float32)


def light_shafts_position(scene, light):
    """Where *light* stands on the un-jittered sample grid of *scene*'s frame: ``(x_u, y_u, w)`` float64, the row vector of
    its ``position`` -- for a directional light of the point at infinity it shines from, ``(position - center, 0)`` --
    through ``S = MVP @ viewport``, the matrix ``MotionState`` uses: the rays stand still under ``temporal_aa``."""
    kind = light.light_type.value if hasattr(light.light_type, "value") else int(light.light_type)
    position = np.asarray(light.position, dtype=np.float64).ravel()[:3]
    if kind == 0:
        point = np.append(position - np.asarray(light.center, dtype=np.float64).ravel()[:3], 0.0)
    else:
        point = np.append(position, 1.0)
    viewport = sample_grid(scene)[3]
    S = np.asarray(scene.camera.MVP, dtype=np.float64) @ np.asarray(viewport, dtype=np.float64)
    x, y, _, w = (float(v) for v in point @ S)
    return x, y, w


def light_shafts_constants(scene):
    """What ``mr_light_shafts_desc`` carries for a frame of *scene* (``light_shafts`` set): ``(light_x, light_y, threshold,
    gain, step, samples, levels, weights)``, or ``None`` where the light has no place on the screen -- it lies in or behind
    the camera's plane (``w <= 0``), or something is not finite -- and the frame runs without the pass.  ``levels =
    halvings + log2(supersample)``: the march runs at the same share of the OUTPUT resolution at any ``supersample``.  The
    light on that level is ``((x_u / w + 0.5) / 2^levels - 0.5, ...)`` rounded to float32, ``step = float32(density /
    samples)``, ``gain = float32(intensity)``.  ``ValueError`` for a ``light`` index the scene does not have."""
    shafts = scene.light_shafts
    lights = list(scene.lights)
    if shafts.light >= len(lights):
        raise ValueError(f"light shafts: light {shafts.light} does not exist: the scene has {len(lights)}")
    s = check_supersample(getattr(scene, "supersample", 1))
    levels = shafts.halvings + {1: 0, 2: 1, 4: 2}[s]
    with np.errstate(all="ignore"):
        x, y, w = light_shafts_position(scene, lights[shafts.light])
        if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(w)) or w <= 0:
            return None
        lx = np.float32((x / w + 0.5) / 2.0 ** levels - 0.5)
        ly = np.float32((y / w + 0.5) / 2.0 ** levels - 0.5)
        step = np.float32(np.float64(shafts.density) / np.float64(shafts.samples))
    if not (np.isfinite(lx) and np.isfinite(ly) and np.isfinite(step) and step > 0):
        return None
    return (float(lx), float(ly), shafts.threshold, float(np.float32(shafts.intensity)), float(step), shafts.samples, levels,
            light_shafts_weights(shafts.decay, shafts.samples))


TONE_OPERATORS = ("linear", "reinhard", "aces")


def permille(fraction):
    """A trim as the device takes it: ``round(1000 * fraction)``, halves away from zero, evaluated in float64."""
    return int(np.floor(1000.0 * float(fraction) + 0.5))


def tone_map_table():
    """``EXP2[f] = float32(2 ** (f / 256))`` for f in 0 .. 255, computed in float64: the table the kernels, the mirror and the
    reference read -- no ``exp2`` runs on the device."""
    return np.exp2(np.arange(256, dtype=np.float64) / 256.0).astype(np.float32)


def check_tone_map(operator, exposure, key, low, high, speed, white, min_exposure, max_exposure):
    """The parameters of a ``ToneMap``, in that order: *operator* one of ``TONE_OPERATORS``; *exposure* ``None`` (metered) or
    a real number that is finite and > 0 as float32; *key*, *white*, *min_exposure* and *max_exposure* finite and > 0 as
    float32 with ``min_exposure <= max_exposure``; *speed* in (0, 1] as float32; *low* and *high* fractions whose permille
    satisfy ``0 <= low < high <= 1000``."""
    def number(value, what):
        if isinstance(value, (bool, str, bytes)) or not isinstance(value, (int, float, np.integer, np.floating)):
            raise TypeError(f"tone_map: {what} must be a real number, got {value!r}")
        with np.errstate(over="ignore"):
            return np.float32(value)

    def positive(value, what):
        v = number(value, what)
        if not np.isfinite(v) or v <= 0:
            raise ValueError(f"tone_map: {what} must be finite and > 0 as float32, got {value!r}")
        return float(value)
    if not isinstance(operator, str):
        raise TypeError(f"tone_map: operator must be a str, got {operator!r}")
    if operator not in TONE_OPERATORS:
        raise ValueError(f"tone_map: operator must be one of {TONE_OPERATORS}, got {operator!r}")
    if exposure is not None:
        exposure = positive(exposure, "exposure")
    key, white = positive(key, "key"), positive(white, "white")
    min_exposure, max_exposure = positive(min_exposure, "min_exposure"), positive(max_exposure, "max_exposure")
    if np.float32(min_exposure) > np.float32(max_exposure):
        raise ValueError(f"tone_map: min_exposure {min_exposure!r} exceeds max_exposure {max_exposure!r}")
    s = number(speed, "speed")
    if not np.isfinite(s) or not (0 < s <= 1):
        raise ValueError(f"tone_map: speed must lie in (0, 1] as float32, got {speed!r}")
    lo, hi = number(low, "low"), number(high, "high")
    if not (np.isfinite(lo) and np.isfinite(hi)) or not (0 <= permille(low) < permille(high) <= 1000):
        raise ValueError(f"tone_map: the trims must satisfy 0 <= low < high <= 1 in permille, got {low!r}, {high!r}")
    return operator, exposure, key, float(low), float(high), float(speed), white, min_exposure, max_exposure


def tone_map_constants(scene):
    """What ``mr_tone_map_desc`` carries for a frame of *scene* (``tone_map`` set): ``(op, fixed, exposure, key, white, speed,
    min_exposure, max_exposure, low_pm, high_pm, table)``; a metered description carries exposure 1."""
    tm = scene.tone_map
    return (TONE_OPERATORS.index(tm.operator), int(tm.exposure is not None), 1.0 if tm.exposure is None else tm.exposure, tm.key, tm.white,
            tm.speed, tm.min_exposure, tm.max_exposure, permille(tm.low), permille(tm.high), tone_map_table())


LAYER_NAMES = ("model", "face", "material", "barycentric", "depth", "position", "face_normal", "normal", "uv")
LAYER_DTYPES = (np.int32, np.int32, np.int32, np.float32, np.float32, np.float32, np.float32, np.float32, np.float32)
LAYER_CHANNELS = (1, 1, 1, 3, 1, 3, 3, 3, 2)


def check_layers(names):
    """The names of a ``Layers``: a non-empty tuple (or list) of distinct strings out of ``LAYER_NAMES``; returned as a tuple
    in the order given."""
    if isinstance(names, (str, bytes)) or not isinstance(names, (tuple, list)):
        raise TypeError(f"layers: the names must be a tuple of str, got {names!r}")
    names = tuple(names)
    if not names:
        raise ValueError("layers: at least one layer must be named")
    for name in names:
        if not isinstance(name, str):
            raise TypeError(f"layers: a name must be a str, got {name!r}")
        if name not in LAYER_NAMES:
            raise ValueError(f"layers: unknown layer {name!r}: the layers are {LAYER_NAMES}")
    if len(set(names)) != len(names):
        raise ValueError(f"layers: a layer is named twice in {names!r}")
    return names


def layer_mask(names):
    """The bit mask ``mr_layers_desc`` carries for these names: bit i is ``LAYER_NAMES[i]``."""
    return sum(1 << LAYER_NAMES.index(name) for name in names)


def depth_sign(camera):
    """+1 or -1: the sign under which the view-space z of a point in front of *camera* is its eye depth -- ``depth_map``'s
    rule (its docstring has the reasons)."""
    P = np.asarray(camera.projection, dtype=np.float64)
    n, f = float(camera.near), float(camera.far)
    if P[2, 3] != 0:
        return 1.0 if P[2, 3] > 0 else -1.0
    mid = 0.5 * (n + f)
    ndc = lambda z: abs((z * P[2, 2] + P[3, 2]) / P[3, 3])
    return 1.0 if ndc(mid) <= ndc(-mid) else -1.0


def layer_matrix(scene):
    """``S`` of ``mr_layers_desc`` for a frame of *scene*, float64 ``(4, 4)``, row vectors: columns 0, 1, 2 are x, y and w of
    ``MVP . viewport`` on the sample grid as ``pack_frame`` hands it to the frame -- ``sample_grid(scene, jittered=True)``,
    the sub-sample offset of a ``temporal_aa`` included -- and column 3 is the view matrix's z column times ``depth_sign``:
    a world point's eye depth, > 0 in front of the camera, for orthographic cameras too."""
    cam = scene.camera
    viewport = np.asarray(sample_grid(scene, jittered=True)[3], dtype=np.float64)
    full = np.asarray(cam.MVP, dtype=np.float64) @ viewport
    S = np.empty((4, 4), dtype=np.float64)
    S[:, :3] = full[:, (0, 1, 3)]
    S[:, 3] = depth_sign(cam) * np.asarray(cam.lookat, dtype=np.float64)[:, 2]
    if not np.isfinite(S).all():
        raise ValueError("layers: the camera's matrices are not finite")
    return S


def check_motion_blur(shutter):
    """The parameter of a ``MotionBlur``: a Python float that lies in (0, 1] as float32."""
    if isinstance(shutter, (bool, str, bytes)) or not isinstance(shutter, (int, float, np.integer, np.floating)):
        raise TypeError(f"motion blur: shutter must be a real number, got {shutter!r}")
    with np.errstate(over="ignore"):
        as_f32 = np.float32(shutter)
    if not np.isfinite(as_f32) or not (0 < as_f32 <= 1):
        raise ValueError(f"motion blur: shutter must lie in (0, 1] as float32, got {shutter!r}")
    return float(shutter)


def check_motion_deformation(value):
    """The flag of ``MotionBlur(deformation=...)``: a ``bool``, nothing else."""
    if not isinstance(value, (bool, np.bool_)):
        raise TypeError(f"motion blur: deformation must be a bool, got {value!r}")
    return bool(value)


def check_temporal_aa(blend, jitter):
    """The parameters of a ``TemporalAA``: *blend* a Python float that lies in (0, 1] as float32, *jitter* an int in
    0 .. 64 (the length of the sub-sample sequence; 0: no jitter)."""
    if isinstance(blend, (bool, str, bytes)) or not isinstance(blend, (int, float, np.integer, np.floating)):
        raise TypeError(f"temporal AA: blend must be a real number, got {blend!r}")
    with np.errstate(over="ignore"):
        as_f32 = np.float32(blend)
    if not np.isfinite(as_f32) or not (0 < as_f32 <= 1):
        raise ValueError(f"temporal AA: blend must lie in (0, 1] as float32, got {blend!r}")
    if isinstance(jitter, (bool, np.bool_)) or not isinstance(jitter, (int, np.integer)):
        raise TypeError(f"temporal AA: jitter must be an int, got {jitter!r}")
    if not 0 <= jitter <= 64:
        raise ValueError(f"temporal AA: jitter must lie in 0 .. 64, got {jitter!r}")
    return float(blend), int(jitter)


def _halton(i, base):
    """The radical inverse of *i* >= 0 in *base*: Halton's sequence, float64, digit by digit from the lowest."""
    f, r = 1.0, 0.0
    while i > 0:
        f /= base
        r += f * (i % base)
        i //= base
    return r


def taa_jitter(k, n):
    """The sub-sample offset ``(jx, jy)`` of temporal-AA frame *k* (counted since the history was last forgotten) of a
    sequence of *n*, in sample-grid units, float64: ``(0.0, 0.0)`` for ``k % n == 0`` or ``n == 0``, otherwise
    ``(halton(k % n, 2) - 0.5, halton(k % n, 3) - 0.5)`` -- in [-0.5, 0.5), period *n*."""
    k, n = int(k), int(n)
    if n == 0 or k % n == 0:
        return 0.0, 0.0
    return _halton(k % n, 2) - 0.5, _halton(k % n, 3) - 0.5


def sample_jitter(scene):
    """The scene's ``_sample_jitter`` -- the private mechanism that carries a sub-sample offset into ``pack_frame`` -- as a
    pair of floats, or ``None`` (absent or ``None``: off).  ``TemporalAA`` sets it while it issues a frame."""
    jitter = getattr(scene, "__dict__", {}).get("_sample_jitter")
    if jitter is None:
        return None
    jx, jy = (float(v) for v in jitter)
    if not (np.isfinite(jx) and np.isfinite(jy)):
        raise ValueError(f"_sample_jitter must be two finite numbers, got {jitter!r}")
    return jx, jy


class MotionState:
    """What a frame leaves for the next one's velocity: ``S = view . projection . viewport`` of its camera on the sample
    grid (one homogeneous 4x4, world to un-divided screen, float64), the scene's models (the objects themselves: another
    list is another scene) and a copy of every model's ``pose`` (``None``: the identity).  With
    ``MotionBlur(deformation=True)`` also what bends a model: a copy of every model's ``bones`` and ``morph_weights``, the
    serials of its ``skin`` and ``morph`` (their identity), and ``serial``, the library's vertex serial once the frame has
    been enqueued (``None`` until then: ``DeviceRenderer.note_motion_serial``)."""

    __slots__ = ("S", "models", "poses", "bones", "weights", "skins", "morphs", "serial")

    def __init__(self, scene):
        viewport = sample_grid(scene)[3]
        self.S = np.asarray(scene.camera.MVP, dtype=np.float64) @ np.asarray(viewport, dtype=np.float64)
        self.models = tuple(scene.models)
        self.poses = tuple(None if m.pose is None else np.array(m.pose, dtype=np.float64) for m in self.models)
        self.bones = self.weights = self.skins = self.morphs = self.serial = None
        if getattr(getattr(scene, "motion_blur", None), "deformation", False):
            self.bones = tuple(None if m.bones is None else np.array(m.bones, dtype=np.float64) for m in self.models)
            self.weights = tuple(None if m.morph_weights is None else np.array(m.morph_weights, dtype=np.float64) for m in self.models)
            self.skins = tuple((m.skin is not None, m._skin_serial) for m in self.models)
            self.morphs = tuple((m.morph is not None, m._morph_serial) for m in self.models)

    def same_models(self, other):
        return len(self.models) == len(other.models) and all(a is b for a, b in zip(self.models, other.models))


def motion_vertices(scene, previous, now=None):
    """What ``mr_motion_faces_desc`` carries for a frame of *scene* (``MotionBlur(deformation=True)``) that follows the frame
    which left *previous* (a ``MotionState``; ``None``, one of another model list or one without the deformation's part:
    no previous frame, nothing flagged): ``(Sn, Sp, deforming, prev_serial)`` -- ``Sn`` and ``Sp`` float64 ``(4, 3)``, the
    (x, y, w) columns of this frame's and the previous frame's ``S``; ``deforming`` int32 ``(len(scene.models),)``, 1 for a
    model whose ``bones`` or ``morph_weights`` differ by value, or whose ``skin`` or ``morph`` is another object, than at
    the previous frame; ``prev_serial`` the vertex serial that frame noted (-1: none).  A flagged model keeps its class
    in ``motion_matrices``: its samples are overwritten behind ``k_velocity``.  *now* is this frame's own ``MotionState`` where
    the caller holds it already (``motion_matrices`` returns it): nothing is copied twice."""
    if now is None:
        now = MotionState(scene)
    flags = np.zeros(len(now.models), dtype=np.int32)
    if previous is None or previous.bones is None or now.bones is None or not now.same_models(previous):
        return now.S[:, (0, 1, 3)].copy(), now.S[:, (0, 1, 3)].copy(), flags, -1

    def differ(a, b):
        return (a is None) != (b is None) or (a is not None and not np.array_equal(a, b))

    for i in range(len(flags)):
        flags[i] = int(differ(now.bones[i], previous.bones[i]) or differ(now.weights[i], previous.weights[i])
                       or now.skins[i] != previous.skins[i] or now.morphs[i] != previous.morphs[i])
    serial = -1 if previous.serial is None else int(previous.serial)
    return (np.ascontiguousarray(now.S[:, (0, 1, 3)]), np.ascontiguousarray(previous.S[:, (0, 1, 3)]), flags, serial)


def motion_matrices(scene, previous):
    """What ``mr_motion_desc`` carries for a frame of *scene* (``motion_blur`` set) that follows the frame which left
    *previous* (a ``MotionState``; ``None``, or one of another model list: no previous frame, identity motion):
    ``(depth_map, T, B, class_of_model, state)`` -- ``T`` float64 ``(n_classes, 4, 3)``, ``B`` float64 ``(3, 3)``,
    ``class_of_model`` int32 ``(len(scene.models),)`` and ``state``, this frame's own ``MotionState``.

    Row vectors, as upstream.  A sample (x, y) of this frame with z-buffer value Z has the screen row vector ``(x, y,
    scr_z, 1)``, ``scr_z = ((f + n) - 2 n f / Z) / (f - n)`` (upstream's ``linearize_z`` undone), which is ``1 / Z`` times
    ``(x Z, y Z, Z, 1) . Lz`` with the constant matrix ``Lz`` below.  With ``S`` as in ``MotionState``, a model moved by
    ``M`` (its ``pose``) takes that vector to the previous frame's un-divided screen through ``K = inv(S_now) . inv(M_now)
    . M_prev . S_prev``; class 0 -- the camera only: every model whose pose is the previous frame's -- drops the ``M``
    factors.  ``T = Lz . K[:, (x, y, w)]``, scaled by its largest entry (a positive factor: the kernel tells front from
    back by the sign of ``u_2 * Z``).  A model whose current pose is singular, or whose ``T`` is not finite, stays in class
    0: it moves with the camera alone.  Bones and morph weights contribute nothing.

    ``B`` serves the samples no face covers.  Under a perspective camera they lie at infinity: ``(x, y, s, 1) .
    inv(S_now)`` has w = 0 for ``s = -(x A[0,3] + y A[1,3] + A[3,3]) / A[2,3]``, ``A = inv(S_now)``, which is linear in
    ``(x, y, 1)``; under an orthographic one, which sees no point at infinity, they lie on the far plane, ``s = f - n``.
    ``B = rows(x, y, 1 -> x, y, s, 1) . K_0[:, (x, y, w)]``, scaled likewise."""
    cam = scene.camera
    now = MotionState(scene)
    if previous is None or not now.same_models(previous):
        previous = now
    n, f = float(cam.near), float(cam.far)
    lz = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, (f + n) / (f - n), 1.0],
                   [0.0, 0.0, -2.0 * n * f / (f - n), 0.0]])
    try:
        inv_now = np.linalg.inv(now.S)
    except np.linalg.LinAlgError:
        raise ValueError("motion blur: the camera's matrices cannot be inverted") from None

    def scaled(m):
        with np.errstate(all="ignore"):
            largest = np.abs(m).max()
            return m / largest if np.isfinite(largest) and largest > 0 else np.full_like(m, np.nan)

    # (a camera that stayed where it was is the identity exactly, not to within the inverse's rounding)
    k0 = np.eye(4) if previous is now or np.array_equal(previous.S, now.S) else inv_now @ previous.S
    matrices = [scaled((lz @ k0)[:, (0, 1, 3)])]
    if not np.isfinite(matrices[0]).all():
        raise ValueError("motion blur: the camera's matrices give no finite motion")
    class_of = np.zeros(len(now.models), dtype=np.int32)
    eye = np.eye(4)
    for i, (m_now, m_prev) in enumerate(zip(now.poses, previous.poses)):
        if (m_now is None and m_prev is None) or (m_now is not None and m_prev is not None and np.array_equal(m_now, m_prev)):
            continue
        try:
            inv_m = eye if m_now is None else np.linalg.inv(m_now)
        except np.linalg.LinAlgError:
            continue
        with np.errstate(all="ignore"):
            t = scaled((lz @ (inv_now @ inv_m @ (eye if m_prev is None else m_prev) @ previous.S))[:, (0, 1, 3)])
        if not np.isfinite(t).all():
            continue
        class_of[i] = len(matrices)
        matrices.append(t)
    P = np.asarray(cam.projection, dtype=np.float64)
    a = inv_now
    if P[2, 3] != 0 and a[2, 3] != 0:
        rows = np.array([[1.0, 0.0, -a[0, 3] / a[2, 3], 0.0], [0.0, 1.0, -a[1, 3] / a[2, 3], 0.0], [0.0, 0.0, -a[3, 3] / a[2, 3], 1.0]])
    else:
        rows = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, f - n, 1.0]])
    background = scaled((rows @ k0)[:, (0, 1, 3)])
    if not np.isfinite(background).all():
        raise ValueError("motion blur: the camera's matrices give no finite motion")
    return depth_map(scene, cam), np.ascontiguousarray(matrices, dtype=np.float64), np.ascontiguousarray(background), class_of, now


def sample_grid(scene, jittered=False):
    """(s, sample-grid height, sample-grid width, sample-grid viewport) of a scene's frame.  With *jittered* -- what
    ``pack_frame`` hands to the frame, and nothing else -- the scene's ``_sample_jitter`` (``sample_jitter``), in
    sample-grid units, is added to x and y of the viewport's translation row: the velocity, the overlay's lines and the
    camera's offsets know nothing of it."""
    cam = scene.camera
    s = check_supersample(getattr(scene, "supersample", 1))
    height, width = (int(v) for v in scene.resolution)
    if s == 1:
        viewport = cam.viewport
    else:
        from .transformation import ViewPort
        height, width = s * height, s * width
        viewport = ViewPort((height, width), cam.far, cam.near, x_offset=cam.x_offset * s, y_offset=cam.y_offset * s)
    jitter = sample_jitter(scene) if jittered else None
    if jitter is not None:
        viewport = np.array(viewport, dtype=np.float64)
        viewport[3, 0] += jitter[0]
        viewport[3, 1] += jitter[1]
    return s, height, width, viewport


def check_pose(value):
    """``Model.pose``: ``None``, or a finite 4x4 matrix, returned as a read-only float64 copy.  ``TypeError`` for what
    is no array of numbers, ``ValueError`` for a wrong shape or an entry that is not finite."""
    if value is None:
        return None
    if isinstance(value, (str, bytes)):
        raise TypeError(f"pose must be None or a 4x4 matrix, got {type(value).__name__}")
    try:
        m = np.array(value, dtype=np.float64)
    except TypeError as exc:
        raise TypeError(f"pose must be None or a 4x4 matrix of numbers: {exc}") from None
    except ValueError as exc:
        raise ValueError(f"pose must be None or a 4x4 matrix of numbers: {exc}") from None
    if m.shape != (4, 4):
        raise ValueError(f"pose must be 4x4, got shape {m.shape}")
    if not np.isfinite(m).all():
        raise ValueError("pose must be finite")
    m = np.ascontiguousarray(m)
    m.setflags(write=False)
    return m


def _numbers(value, what, dtype=np.float64):
    """*value* as an array of numbers, with the ``TypeError`` / ``ValueError`` split of ``check_pose``."""
    if isinstance(value, (str, bytes)):
        raise TypeError(f"{what} must be an array of numbers, got {type(value).__name__}")
    try:
        return np.array(value, dtype=dtype)
    except TypeError as exc:
        raise TypeError(f"{what} must be an array of numbers: {exc}") from None
    except ValueError as exc:
        raise ValueError(f"{what} must be an array of numbers: {exc}") from None


def check_skin(joints, weights, normals=False):
    """The parts of a ``Skin``: *joints* ``(n, 4)`` integral and not negative, returned as a read-only ``int32`` copy;
    *weights* the same shape and finite, as a read-only ``float64`` copy; *normals* as ``check_pose_normals`` takes it.
    ``TypeError`` for what is no array of numbers, ``ValueError`` for a wrong shape or a wrong value."""
    j = _numbers(joints, "skin joints")
    w = _numbers(weights, "skin weights")
    if j.ndim != 2 or j.shape[1] != 4:
        raise ValueError(f"skin joints must be (n, 4), got shape {j.shape}")
    if w.shape != j.shape:
        raise ValueError(f"skin weights must have the joints' shape {j.shape}, got {w.shape}")
    if not np.isfinite(w).all():
        raise ValueError("skin weights must be finite")
    if not np.isfinite(j).all() or (j != np.floor(j)).any():
        raise ValueError("skin joints must be integers")
    if (j < 0).any():
        raise ValueError("skin joints must not be negative")
    if j.size and j.max() > np.iinfo(np.int32).max:
        raise ValueError("skin joints must fit 32 bits")
    if not isinstance(normals, (bool, np.bool_)) and not (isinstance(normals, (int, np.integer)) and int(normals) in (0, 1)):
        raise TypeError(f"Skin(normals=...) must be True or False, got {normals!r}")
    j, w = np.ascontiguousarray(j.astype(np.int32)), np.ascontiguousarray(w)
    j.setflags(write=False)
    w.setflags(write=False)
    return j, w, bool(normals)


def check_bones(value):
    """``Model.bones``: ``None``, or a finite ``(b, 4, 4)`` array with b >= 1, returned as a read-only float64 copy."""
    if value is None:
        return None
    b = _numbers(value, "bones")
    if b.ndim != 3 or b.shape[1:] != (4, 4) or b.shape[0] < 1:
        raise ValueError(f"bones must be (b, 4, 4) with b >= 1, got shape {b.shape}")
    if not np.isfinite(b).all():
        raise ValueError("bones must be finite")
    b = np.ascontiguousarray(b)
    b.setflags(write=False)
    return b


def check_skin_pair(skin, bones):
    """What only the pair can break: every joint names one of the bones."""
    if skin is not None and bones is not None and skin.joints.size and int(skin.joints.max()) >= len(bones):
        raise ValueError(f"skin joints reach bone {int(skin.joints.max())}, bones has {len(bones)}")


def active_skin(model):
    """The model's ``Skin`` when it has ``bones`` too and so moves, else ``None``; ``ValueError`` for a skin whose row
    count is not the vertices' (``vertices`` was replaced after the skin was set)."""
    skin, bones = getattr(model, "skin", None), getattr(model, "bones", None)
    if skin is None or bones is None:
        return None
    if len(skin.joints) != len(model.vertices):
        raise ValueError(f"the model's skin has {len(skin.joints)} rows, its vertices {len(model.vertices)}")
    return skin


def _morph_entry(entry, what):
    """One morph target as ``(indices, deltas)``: read-only ``int32`` ``(n_k,)`` and ``float64`` ``(n_k, 3)`` copies.
    *entry* is a pair of that form or a dense ``(n, 3)`` array, which means ``(arange(n), array)``."""
    pair = None
    if isinstance(entry, (tuple, list)) and len(entry) == 2:
        first, second = _numbers(entry[0], f"{what} indices"), _numbers(entry[1], f"{what} deltas")
        if first.ndim == 1 and second.ndim == 2:
            pair = (first, second)
    if pair is None:
        dense = _numbers(entry, what)
        if dense.ndim != 2 or dense.shape[1] != 3:
            raise ValueError(f"{what} must be (indices, deltas) or a dense (n, 3) array, got shape {dense.shape}")
        pair = (np.arange(len(dense), dtype=np.float64), dense)
    i, d = pair
    if d.shape != (len(i), 3):
        raise ValueError(f"{what} deltas must be ({len(i)}, 3), got shape {d.shape}")
    if not np.isfinite(d).all():
        raise ValueError(f"{what} deltas must be finite")
    if not np.isfinite(i).all() or (i != np.floor(i)).any():
        raise ValueError(f"{what} indices must be integers")
    if (i < 0).any():
        raise ValueError(f"{what} indices must not be negative")
    if i.size and i.max() > np.iinfo(np.int32).max:
        raise ValueError(f"{what} indices must fit 32 bits")
    i, d = np.ascontiguousarray(i.astype(np.int32)), np.ascontiguousarray(d)
    if len(np.unique(i)) != len(i):
        raise ValueError(f"{what} names an index twice")
    i.setflags(write=False)
    d.setflags(write=False)
    return i, d


def _morph_entries(value, what):
    if isinstance(value, (str, bytes)) or not hasattr(value, "__len__") or not hasattr(value, "__iter__"):
        raise TypeError(f"{what} must be a sequence of targets, got {type(value).__name__}")
    return list(value)


def check_morph(targets, normal_targets=None):
    """The parts of a ``Morph``: *targets* a sequence of t >= 1 entries, each a pair ``(indices, deltas)`` -- ``(n_k,)``
    integral, not negative and without duplicates; ``(n_k, 3)`` finite -- or a dense ``(n, 3)`` array; *normal_targets*
    ``None`` or t entries of the same forms, ``None`` among them for a target that moves no normal.  Returns two tuples of
    ``(int32 indices, float64 deltas)`` pairs, read-only copies (the second ``None`` without *normal_targets*).
    ``TypeError`` for what is no sequence of arrays of numbers, ``ValueError`` for a wrong shape or a wrong value."""
    entries = _morph_entries(targets, "morph targets")
    if len(entries) < 1:
        raise ValueError("a morph needs at least one target")
    out = tuple(_morph_entry(e, f"morph target {k}") for k, e in enumerate(entries))
    if normal_targets is None:
        return out, None
    entries = _morph_entries(normal_targets, "morph normal_targets")
    if len(entries) != len(out):
        raise ValueError(f"normal_targets must have one entry per target ({len(out)}), got {len(entries)}")
    none = (np.zeros(0, dtype=np.int32), np.zeros((0, 3), dtype=np.float64))
    for arr in none:
        arr.setflags(write=False)
    return out, tuple(none if e is None else _morph_entry(e, f"morph normal target {k}") for k, e in enumerate(entries))


def morph_csr(pairs):
    """The tables of ``check_morph`` as the C ABI takes them, CSR by target: ``(first (t + 1,) int32, index int32,
    delta (N, 3) float64)``."""
    first = np.zeros(len(pairs) + 1, dtype=np.int64)
    first[1:] = np.cumsum([len(i) for i, _ in pairs])
    if first[-1] > np.iinfo(np.int32).max:
        raise ValueError("the morph's targets list more than 2^31 - 1 entries")
    index = np.ascontiguousarray(np.concatenate([i for i, _ in pairs]), dtype=np.int32)
    delta = np.ascontiguousarray(np.concatenate([d for _, d in pairs]), dtype=np.float64)
    return np.ascontiguousarray(first, dtype=np.int32), index, delta


def check_morph_weights(value):
    """``Model.morph_weights``: ``None``, or a finite ``(t,)`` array with t >= 1, returned as a read-only float64 copy."""
    if value is None:
        return None
    w = _numbers(value, "morph weights")
    if w.ndim != 1 or w.shape[0] < 1:
        raise ValueError(f"morph weights must be (t,) with t >= 1, got shape {w.shape}")
    if not np.isfinite(w).all():
        raise ValueError("morph weights must be finite")
    w = np.ascontiguousarray(w)
    w.setflags(write=False)
    return w


def check_morph_pair(morph, weights):
    """What only the pair can break: one weight per target."""
    if morph is not None and weights is not None and len(weights) != len(morph.targets):
        raise ValueError(f"the morph has {len(morph.targets)} targets, morph_weights {len(weights)} entries")


def check_morph_fits(morph, model):
    """Every index of *morph* names a vertex (a normal) of *model*; normal targets need a model that has normals."""
    n = len(model.vertices)
    reach = max((int(i.max()) for i, _ in morph.targets if i.size), default=-1)
    if reach >= n:
        raise ValueError(f"the morph reaches vertex {reach}, the model has {n} vertices")
    if morph.normal_targets is not None:
        if model.normals is None:
            raise ValueError("normal_targets need a model that has normals")
        reach = max((int(i.max()) for i, _ in morph.normal_targets if i.size), default=-1)
        if reach >= len(model.normals):
            raise ValueError(f"the morph reaches normal {reach}, the model has {len(model.normals)} normals")


def active_morph(model):
    """The model's ``Morph`` when it has ``morph_weights`` too and so moves, else ``None``; ``ValueError`` for a morph
    whose indices no longer fit the model (``vertices`` or ``normals`` was replaced after the morph was set)."""
    morph, weights = getattr(model, "morph", None), getattr(model, "morph_weights", None)
    if morph is None or weights is None:
        return None
    check_morph_fits(morph, model)
    check_morph_pair(morph, weights)
    return morph


_native_morph = None         # mr_host_morph_chain of the HIP library, or False


def _fast_morph():
    """The library's host helper, if the library is built (it loads without a GPU); else the loop below."""
    global _native_morph
    if _native_morph is None:
        try:
            from ._native import load_library
            _native_morph = load_library().mr_host_morph_chain
        except Exception:           # not built / not loadable here: the pure-Python chain gives the same bits
            _native_morph = False
    return _native_morph


def _morph_chain(base, pairs, weights, native):
    """``acc = base[i][c]``, then ``acc = fma(w[k], d_k[i][c], acc)`` for every target k that lists i, k ascending, for
    the first three columns of the float64 array *base*; further columns pass through."""
    base = np.ascontiguousarray(base, dtype=np.float64)
    out = base.copy()
    fast = _fast_morph() if native is None or native else False
    if fast:
        first, index, delta = morph_csr(pairs)
        rc = fast(base.ctypes.data, len(base), base.shape[1], len(pairs), first.ctypes.data, index.ctypes.data, delta.ctypes.data,
                  weights.ctypes.data, out.ctypes.data)
        if rc != 0:
            raise ValueError("mr_host_morph_chain refused the morph's tables")
        return out
    from ._fp import fma
    for k, (index, delta) in enumerate(pairs):
        w = float(weights[k])
        for i, d in zip(index.tolist(), delta.tolist()):
            for c in range(3):
                out[i, c] = fma(w, d[c], float(out[i, c]))
    return out


def morphed_vertices(model, native=None):
    """The float64 vertices ``V_m`` of a model that has ``morph`` and ``morph_weights``: vertex i starts from
    ``float64(vertices[i])`` and takes ``fma(w[k], d_k[i][c], .)`` for every target k that lists it, k ascending, in its
    first three components; ``None`` for a model without the pair.  *native*: ``False`` forces the pure-Python chain, the
    yardstick of the library's ``mr_host_morph_chain``."""
    morph = active_morph(model)
    if morph is None:
        return None
    return _morph_chain(np.asarray(model.vertices).astype(np.float64), morph.targets, model.morph_weights, native)


def morphed_normals(model, native=None):
    """The float32 normals ``N_m`` of a model whose normals follow its morph (``normal_targets``, ``morph_weights`` set,
    ``normals`` not ``None``): the chain of ``morphed_vertices`` from ``float64(float32(normals))`` over the normal
    targets, rounded to float32 once, the shape kept.  ``None`` for every other model."""
    morph = active_morph(model)
    if morph is None or morph.normal_targets is None or model.normals is None:
        return None
    normals = np.ascontiguousarray(model.normals, dtype=np.float32)
    out = normals.copy()
    out[:, :3] = _morph_chain(normals[:, :3].astype(np.float64), morph.normal_targets, model.morph_weights, native).astype(np.float32)
    return out


def normal_owners(model):
    """(len(normals),) int32: for every vertex normal the (non-negative) vertex index at the first (face, corner) of
    ``_faces`` in row-major order whose normal column names it; -1 for a normal no corner references."""
    faces = np.asarray(model._faces)
    n_normals, n_verts = len(model.normals), len(model.vertices)
    vertex = _wrap(faces[..., 0].astype(np.int64), n_verts, "vertex").ravel()
    normal = _wrap(faces[..., 2].astype(np.int64), n_normals, "normal").ravel()
    owners = np.full(n_normals, -1, dtype=np.int32)
    which, first = np.unique(normal, return_index=True)
    owners[which] = vertex[first]
    return owners


def blend_matrices(skin, bones, rows):
    """S of the vertices *rows* (pure Python): ``S[i][r][c] = dot_chain(W[i], (B[J[i][k]][r][c] for k in 0..3))``."""
    from ._fp import dot_chain
    out = np.empty((len(rows), 4, 4), dtype=np.float64)
    for n, i in enumerate(rows):
        picked = bones[skin.joints[i]]
        for r in range(4):
            for c in range(4):
                out[n, r, c] = dot_chain(skin.weights[i], picked[:, r, c])
    return out


_native_skin = None          # (mr_host_skin_chain, mr_host_skin_chain3) of the HIP library, or False


def _fast_skin():
    """The library's host helpers, if the library is built (it loads without a GPU); else the loops below."""
    global _native_skin
    if _native_skin is None:
        try:
            from ._native import load_library
            lib = load_library()
            _native_skin = (lib.mr_host_skin_chain, lib.mr_host_skin_chain3)
        except Exception:           # not built / not loadable here: the pure-Python chains give the same bits
            _native_skin = False
    return _native_skin


def skinned_vertices(model, native=None):
    """The float64 vertices of a model that has ``skin`` and ``bones``: ``V'[i] = matmul_chain(float64(vertices[i]), S_i)``
    with S_i the vertex's blend matrix (``blend_matrices``); ``None`` for a model without the pair.  *native*: ``False``
    forces the pure-Python chains, the yardstick of the library's ``mr_host_skin_chain``."""
    skin = active_skin(model)
    if skin is None:
        return None
    verts = morphed_vertices(model, native)          # (morph first, then skin)
    if verts is None:
        verts = np.ascontiguousarray(np.asarray(model.vertices).astype(np.float64))
    bones = model.bones
    check_skin_pair(skin, bones)
    out = np.empty_like(verts)
    fast = _fast_skin() if native is None or native else False
    if fast:
        fast[0](verts.ctypes.data, skin.joints.ctypes.data, skin.weights.ctypes.data, bones.ctypes.data, len(verts), out.ctypes.data)
        return out
    from ._fp import dot_chain
    blend = blend_matrices(skin, bones, range(len(verts)))
    for i in range(len(verts)):
        for c in range(4):
            out[i, c] = dot_chain(verts[i], blend[i, :, c])
    return out


def skinned_normals(model, native=None):
    """The float64 normals ``n'`` of a model whose normals follow its skin (``Skin(..., normals=True)``, ``bones`` set,
    ``normals`` not ``None``): ``n'[q] = matmul_chain(float64(float32(normals[q])), S_owner[:3, :3])`` with the owner of
    ``normal_owners``, the widened normal itself where nothing owns it.  Not rounded, not re-normalised.  ``None`` for
    every other model."""
    skin = active_skin(model)
    if skin is None or not skin.normals or model.normals is None:
        return None
    followed = morphed_normals(model, native)        # (float32: the morph's normals are rounded before the skin takes them)
    vectors = np.ascontiguousarray(np.ascontiguousarray(model.normals if followed is None else followed, dtype=np.float32)[:, :3].astype(np.float64))
    owners = normal_owners(model)
    bones = model.bones
    check_skin_pair(skin, bones)
    out = vectors.copy()
    fast = _fast_skin() if native is None or native else False
    if fast:
        fast[1](vectors.ctypes.data, owners.ctypes.data, skin.joints.ctypes.data, skin.weights.ctypes.data, bones.ctypes.data,
                len(vectors), out.ctypes.data)
        return out
    from ._fp import dot_chain
    owned = np.flatnonzero(owners >= 0)
    blend = blend_matrices(skin, bones, owners[owned])
    for n, q in enumerate(owned):
        for c in range(3):
            out[q, c] = dot_chain(vectors[q], blend[n, :3, c])
    return out


def posed_vertices(model):
    """The vertices a model renders with: ``model.vertices``; with ``morph`` and ``morph_weights`` the float64 array
    ``morphed_vertices(model)``; with ``skin`` and ``bones`` the float64 array ``skinned_vertices(model)`` of that; with a pose ``matmul_chain`` of either (widened to float64) and the pose -- skin first,
    then pose (``Model.skin``, ``Model.pose``)."""
    pose = getattr(model, "pose", None)
    verts = skinned_vertices(model)
    if verts is None:
        verts = morphed_vertices(model)
    if verts is None:
        verts = np.asarray(model.vertices)
    if pose is None:
        return verts
    from ._fp import matmul_chain
    return matmul_chain(verts.astype(np.float64), pose)


def check_pose_normals(value):
    """``Model.pose_normals``: ``True`` / ``False`` (``bool``, ``np.bool_``) or the integers 0 / 1, returned as a
    ``bool``; ``TypeError`` for anything else."""
    return _check_flag(value, "pose_normals")


def _check_flag(value, name):
    if isinstance(value, (bool, np.bool_)):
        return bool(value)
    if isinstance(value, (int, np.integer)) and int(value) in (0, 1):
        return bool(value)
    raise TypeError(f"{name} must be True or False, got {value!r}")


def normal_matrix(pose):
    """The 3x3 float64 matrix G that takes a posed model's normals along: the inverse transpose of ``pose[:3, :3]`` in
    the row-vector convention (``n' = n @ G``), formed as the cofactor matrix divided by the determinant.  Plain float64
    operations in the order written here, no LAPACK: ``C[i][j] = a[i+1][j+1] * a[i+2][j+2] - a[i+1][j+2] * a[i+2][j+1]``
    (indices mod 3), ``det = (a[0][0] * C[0][0] + a[0][1] * C[0][1]) + a[0][2] * C[0][2]``, ``G[i][j] = C[i][j] / det``.
    ``ValueError`` when the determinant is 0 or an entry of G is not finite."""
    a = [[float(x) for x in row[:3]] for row in np.asarray(pose, dtype=np.float64)[:3]]
    c = [[a[(i + 1) % 3][(j + 1) % 3] * a[(i + 2) % 3][(j + 2) % 3] - a[(i + 1) % 3][(j + 2) % 3] * a[(i + 2) % 3][(j + 1) % 3]
          for j in range(3)] for i in range(3)]
    det = (a[0][0] * c[0][0] + a[0][1] * c[0][1]) + a[0][2] * c[0][2]
    if det == 0 or det != det:
        raise ValueError("pose_normals needs an invertible pose")
    g = np.array([[c[i][j] / det for j in range(3)] for i in range(3)], dtype=np.float64)
    if not np.isfinite(g).all():
        raise ValueError("pose_normals needs an invertible pose")
    g.setflags(write=False)
    return g


def pose_normal_matrix(model):
    """G of a model whose normals follow its pose (``pose`` set and ``pose_normals`` on), else ``None``."""
    pose = getattr(model, "pose", None)
    if pose is None or not getattr(model, "pose_normals", False):
        return None
    g = model.__dict__.get("_normal_matrix")
    return g if g is not None else normal_matrix(pose)


def _chain_f32(vectors, g):
    """``float32(matmul_chain(float64(float32(vectors)), g))`` of an (..., 3) array: rounded once, not re-normalised."""
    from ._fp import matmul_chain
    v = np.ascontiguousarray(vectors, dtype=np.float32)
    return matmul_chain(v.reshape(-1, 3).astype(np.float64), g).astype(np.float32).reshape(v.shape)


def posed_normals(model):
    """The vertex normals a model renders with: ``model.normals``, or with ``pose_normals`` and a pose the float32 array
    ``float32(matmul_chain(float64(float32(normals)), G))``, ``G = normal_matrix(pose)``.  Normals that follow a skin
    (``skinned_normals``) take the place of the widened normals: ``float32(n')``, or ``float32(matmul_chain(n', G))``.
    With ``auto_normals`` on a moved model none of this applies: the normals are ``auto_normals(model)``, those of the
    final geometry."""
    g = pose_normal_matrix(model)
    if model.normals is None:
        return model.normals
    rebuilt = auto_normals(model)                    # (``Model.auto_normals``: the normals of the final geometry, nothing applied first)
    if rebuilt is not None:
        return rebuilt
    followed = skinned_normals(model)
    if followed is not None:
        from ._fp import matmul_chain
        shape = np.asarray(model.normals).shape
        return (followed if g is None else matmul_chain(followed, g)).astype(np.float32).reshape(shape)
    morphed = morphed_normals(model)                 # (the morph's normals take the place of ``normals`` themselves)
    normals = model.normals if morphed is None else morphed
    if g is None:
        return normals
    return _chain_f32(normals, g)


def check_auto_normals(value):
    """``Model.auto_normals``: ``True`` / ``False`` (``bool``, ``np.bool_``) or the integers 0 / 1, returned as a
    ``bool``; ``TypeError`` for anything else (the rules of ``check_pose_normals``)."""
    return _check_flag(value, "auto_normals")


def auto_normals_active(model):
    """Whether ``Model.auto_normals`` has an effect: the flag is on, ``normals`` is not ``None`` and the model is moved
    (it has ``morph_weights`` on a morph, ``bones`` on a skin, or a ``pose``)."""
    if not getattr(model, "auto_normals", False) or model.normals is None:
        return False
    return getattr(model, "pose", None) is not None or active_skin(model) is not None or active_morph(model) is not None


def face_rows(model):
    """``_faces`` as the library keeps face rows: ``(F, 12)`` int32, corner k at ``[4 k .. 4 k + 3]`` with the vertex and
    normal columns wrapped as ``normal_owners`` wraps them; the uv and material columns, which no caller of this reads,
    are 0."""
    faces = np.asarray(model._faces)
    rows = np.zeros((len(faces), 3, 4), dtype=np.int32)
    rows[..., 0] = _wrap(faces[..., 0].astype(np.int64), len(model.vertices), "vertex")
    rows[..., 2] = _wrap(faces[..., 2].astype(np.int64), len(model.normals), "normal")
    return np.ascontiguousarray(rows.reshape(len(faces), 12))


_native_auto = None          # mr_host_auto_normals of the HIP library, or False


def _fast_auto():
    """The library's host helper, if the library is built (it loads without a GPU); else the loop below."""
    global _native_auto
    if _native_auto is None:
        try:
            from ._native import load_library
            _native_auto = load_library().mr_host_auto_normals
        except Exception:           # not built / not loadable here: the pure-Python chain gives the same bits
            _native_auto = False
    return _native_auto


def auto_normals(model, native=None):
    """The float32 normals N of a model whose ``auto_normals`` has an effect (``auto_normals_active``), the shape of
    ``normals`` kept, else ``None``.  With V = ``posed_vertices(model)`` (float64) and ``L(q)`` the faces that have at
    least one corner whose normal column is q, each once, ascending: ``acc`` = the cross product ``(V[b] - V[a]) x
    (V[c] - V[a])`` of ``L(q)[0]`` (a, b, c the vertex columns of corners 0, 1, 2; every operation rounded on its own),
    plus those of the further faces in order, component by component; ``l = sqrt((acc0 * acc0 + acc1 * acc1) + acc2 *
    acc2)``; ``N[q] = float32(acc / l)``.  ``float32(normals[q])`` stays where ``L(q)`` is empty, ``l == 0``, or a
    component of ``acc`` or ``l`` is not finite.  Only columns 0 to 2 change.  *native*: ``False`` forces the pure-Python
    loop over Python floats, the yardstick of the library's ``mr_host_auto_normals``."""
    if not auto_normals_active(model):
        return None
    verts = np.ascontiguousarray(np.asarray(posed_vertices(model)).astype(np.float64))
    normals = np.ascontiguousarray(model.normals, dtype=np.float32)
    rows = face_rows(model)
    out = normals.copy()
    fast = _fast_auto() if native is None or native else False
    if fast:
        flat = np.ascontiguousarray(normals[:, :3])
        res = np.empty_like(flat)
        rc = fast(verts.ctypes.data, len(verts), rows.ctypes.data, len(rows), flat.ctypes.data, len(flat), res.ctypes.data)
        if rc != 0:
            raise ValueError("mr_host_auto_normals refused the model's faces")
        out[:, :3] = res
        return out
    import math
    lists = [[] for _ in range(len(normals))]
    for f, row in enumerate(rows.tolist()):
        for k in range(3):
            q = row[4 * k + 2]
            if q not in (row[4 * j + 2] for j in range(k)):
                lists[q].append(f)
    v = verts[:, :3].tolist()
    corners = rows[:, [0, 4, 8]].tolist()
    for q, faces in enumerate(lists):
        acc = None
        for f in faces:
            a, b, c = (v[i] for i in corners[f])
            e0 = (b[0] - a[0], b[1] - a[1], b[2] - a[2])
            e1 = (c[0] - a[0], c[1] - a[1], c[2] - a[2])
            cr = (e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0])
            acc = cr if acc is None else (acc[0] + cr[0], acc[1] + cr[1], acc[2] + cr[2])
        if acc is None or not all(math.isfinite(x) for x in acc):
            continue
        sq = (acc[0] * acc[0] + acc[1] * acc[1]) + acc[2] * acc[2]
        if not math.isfinite(sq):                  # (the length would be infinite)
            continue
        l = math.sqrt(sq)
        if l == 0:
            continue
        out[q, :3] = np.array([acc[0] / l, acc[1] / l, acc[2] / l], dtype=np.float64).astype(np.float32)
    return out


def posed_normal_map(texels, g):
    """An object-space normal map under the normal matrix *g*: ``float32(matmul_chain(float64(texels), g))`` texel by
    texel, the shape kept."""
    arr = np.asarray(texels)
    return _chain_f32(arr[..., :3], g)


def pack_light(light) -> PackedLight:
    kind = light.light_type.value if isinstance(light.light_type, Lightning) else int(light.light_type)
    return PackedLight(
        light_type=kind,
        light_pos=_vec3(light.position), light_dir=_vec3(light.direction),
        light_color=_vec3(light.color), light_ambient=_vec3(light.ambient),
        specular_strength=float(light.specular_strength),
        att_constant=float(light.constant), att_linear=float(light.linear),
        att_quadratic=float(light.quadratic),
        spot_edge0=float(np.cos(np.deg2rad(20))), spot_edge1=float(np.cos(np.deg2rad(10))))


def pack_frame(scene, shadows=True) -> PackedFrame:
    cam, light = scene.camera, scene.light
    dbg = scene.debug_camera if scene.debug_camera is not None else cam
    ss, height, width, viewport = sample_grid(scene, jittered=True)
    sky = scene.skybox
    sky_tri = sky_rays = None
    if sky is not None and hasattr(sky, "textures"):
        from .cube_map import sky_frame_constants
        sky_tri, sky_rays = sky_frame_constants(cam, viewport)
        background = np.zeros(3, dtype=np.float32)          # uncovered pixels stay black (frame starts at 0)
    elif sky is not None:
        background = np.asarray(np.array(sky), dtype=np.float32).ravel()
        if background.size != 3:
            raise ValueError("skymap colour must have 3 components")
    else:
        background = np.asarray(_DEFAULT_BACKGROUND, dtype=np.float32)
    first = pack_light(light)
    extras = tuple(pack_light(x) for x in list(getattr(scene, "lights", [light]))[1:])
    if len(extras) > MAX_LIGHTS - 1:
        raise ValueError(f"a scene has at most {MAX_LIGHTS} lights")
    return PackedFrame(
        width=width, height=height, system=int(scene.system),
        backface_culling=bool(cam.backface_culling), light_type=first.light_type, shadows=bool(shadows),
        mvp=np.ascontiguousarray(cam.MVP, dtype=np.float64),
        viewport=np.ascontiguousarray(viewport, dtype=np.float64),
        debug_mvp=np.ascontiguousarray(dbg.MVP, dtype=np.float64),
        frustum_planes=np.ascontiguousarray(cam.frustum_planes, dtype=np.float64),
        z_near=float(cam.near), z_far=float(cam.far),
        camera_pos=_vec3(cam.position),
        light_pos=first.light_pos, light_dir=first.light_dir,
        light_color=first.light_color, light_ambient=first.light_ambient,
        specular_strength=first.specular_strength,
        att_constant=first.att_constant, att_linear=first.att_linear, att_quadratic=first.att_quadratic,
        spot_edge0=first.spot_edge0, spot_edge1=first.spot_edge1,
        background=background, sky_tri=sky_tri, sky_rays=sky_rays, supersample=ss, extra_lights=extras)


def _texture_id(tex, textures, seen):
    key = id(tex)
    if key not in seen:
        arr = np.asarray(tex)
        if arr.ndim != 3 or arr.shape[2] < 3:
            raise ValueError(f"texture must be (h, w, 3), got {arr.shape}")
        seen[key] = len(textures)
        textures.append(np.ascontiguousarray(arr[..., :3], dtype=np.float32))
    return seen[key]


def _posed_map_id(tex, g, model, textures, seen):
    """A texture of its own for *model*'s re-baked copy of the object-space normal map *tex*: another model that
    registered the same array keeps the original, or gets a copy with its own matrix."""
    key = ("posed", id(model), id(tex))
    if key not in seen:
        arr = np.asarray(tex)
        if arr.ndim != 3 or arr.shape[2] < 3:
            raise ValueError(f"texture must be (h, w, 3), got {arr.shape}")
        seen[key] = len(textures)
        textures.append(np.ascontiguousarray(posed_normal_map(arr, g)))
    return seen[key]


def pack_model(model, textures, seen, posed=False) -> PackedModel:
    """*posed*: pack the arrays the model renders with -- ``posed_vertices`` (morph, then skin, then pose) and, with
    ``pose_normals``, a skin or a morph the normals follow, or ``auto_normals``, ``posed_normals``, and with ``pose_normals`` re-baked object-space normal maps -- instead of
    ``model.vertices`` / ``normals`` / the maps as registered: what the oracle needs; the device gets the arrays as they
    are and the matrices and tables beside them (``mr_scene_set_model_pose``, ``mr_scene_set_model_pose_normals``,
    ``mr_scene_set_model_skin``, ``mr_scene_set_model_bones``)."""
    verts = posed_vertices(model) if posed else np.asarray(model.vertices)
    nmat = pose_normal_matrix(model) if posed else None
    if verts.ndim != 2 or verts.shape[1] != 4:
        raise ValueError(f"Model.vertices must be (V, 4), got {verts.shape}")
    faces = np.asarray(model._faces)
    if faces.ndim != 3 or faces.shape[1:] != (3, 4):
        raise ValueError("Model._faces must be (F, 3, 4): every face corner needs v/vt/vn indices "
                         f"(got {faces.shape})")
    uv = None if model.uv is None else np.ascontiguousarray(model.uv, dtype=np.float32)
    normals = None if model.normals is None else np.ascontiguousarray(model.normals, dtype=np.float32)
    morph = active_morph(model) if posed else None
    if posed and normals is not None and (nmat is not None or (active_skin(model) is not None and model.skin.normals)
                                          or (morph is not None and morph.normal_targets is not None)
                                          or auto_normals_active(model)):
        normals = np.ascontiguousarray(posed_normals(model))
    if uv is not None and (uv.ndim != 2 or uv.shape[1] < 2):
        raise ValueError(f"Model.uv must be (T, 3), got {uv.shape}")
    if uv is not None and uv.shape[1] != 3:
        uv = np.ascontiguousarray(np.pad(uv[:, :3], ((0, 0), (0, 3 - min(uv.shape[1], 3)))))

    groups = list(model.material_group)
    mats = []
    for g in range(len(groups)):
        mat = model.face_material(g)
        ks = np.asarray(mat.Ks)
        rec = PackedMaterial(kd=_vec3(mat.Kd), ks255=_vec3(ks * 255), ns=float(mat.Ns))
        if hasattr(mat, "map_Kd"):
            rec.tex_kd = _texture_id(mat.map_Kd, textures, seen)
        if hasattr(mat, "norm"):
            rec.norm_tangent = mat.is_tangent_space("norm")
            if nmat is not None and not rec.norm_tangent:
                rec.tex_norm = _posed_map_id(mat.norm, nmat, model, textures, seen)
            else:
                rec.tex_norm = _texture_id(mat.norm, textures, seen)
        if hasattr(mat, "map_Ks"):
            rec.tex_ks = _texture_id(mat.map_Ks, textures, seen)
        mats.append(rec)
        if (rec.tex_kd >= 0 or rec.tex_norm >= 0 or rec.tex_ks >= 0) and uv is None:
            raise ValueError("model has texture maps but no uv coordinates")
        if rec.norm_tangent and normals is None:
            raise ValueError("tangent-space normal map needs vertex normals")

    out = np.empty(faces.shape, dtype=np.int32)
    out[..., 0] = _wrap(faces[..., 0].astype(np.int64), len(verts), "vertex")
    out[..., 1] = _wrap(faces[..., 1].astype(np.int64), len(uv), "uv") if uv is not None else 0
    out[..., 2] = _wrap(faces[..., 2].astype(np.int64), len(normals), "normal") if normals is not None else 0
    out[..., 3] = _wrap(faces[..., 3].astype(np.int64), len(groups), "material group")
    raw = faces[..., 0].astype(np.int64)
    edge_ids = np.ascontiguousarray(raw, dtype=np.int32) if (raw < 0).any() else None
    return PackedModel(
        vertices=np.ascontiguousarray(verts, dtype=np.float64), uv=uv, normals=normals,
        faces=np.ascontiguousarray(out), materials=mats,
        vertices_are_f32=(verts.dtype == np.float32),
        clip=bool(model.clip), depth_test=bool(model.depth_test), edge_ids=edge_ids)


def pack_scene(scene, shadows=True) -> PackedScene:
    textures, seen = [], {}
    models = [pack_model(m, textures, seen, posed=True) for m in scene.models]
    return PackedScene(frame=pack_frame(scene, shadows), models=models, textures=textures)
