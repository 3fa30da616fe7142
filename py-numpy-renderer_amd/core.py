"""Scene API: ``Model / Camera / Light / Scene`` with ``Scene.render() -> uint8 (H, W, 3)``.

Drop-in for the classes of the reference's ``obj/core.py`` (Model :231, Camera :432,
Light :444, Scene :558): same constructor arguments, same attribute names, same OBJ/MTL
ingest rules.  What differs is where the work happens: ``Scene.render`` packs the scene into
flat arrays (``_pack.py``) and hands it to the HIP library through the C ABI declared in
``include/mi355rast.h``; nothing is rasterised or shaded on the host.
"""
import itertools
import os
from functools import cached_property
from typing import Iterable, List

import numpy as np
from PIL import Image

from . import _fp
from .constants import *  # noqa: F401,F403  (re-exported like the reference's core module)
from .constants import PROJECTION_TYPE, SUBSYSTEM, SYSTEM, mat3x3
from .lightning import Lightning
from .materials import Material
from .transformation import (ViewPort, look_at_rotate_lh, look_at_rotate_rh, looka_at_translate,
                             normalize, perspectives, scale)


def triangulate_int(polygon):
    """Fan triangulation of one parsed ``f`` record (reference: ``obj/core.py:72-74``)."""
    for i in range(1, len(polygon) - 1):
        yield np.array([polygon[0], polygon[i], polygon[i + 1]], dtype=np.int32)


class TextureMaps:
    """``model.textures.register(kind, path, normalize=True, tangent=False)``
    (reference: ``obj/core.py:77-105``)."""

    texture_map = {
        "diffuse": "map_Kd",
        "ambient": "map_Ka",
        "specular": "map_Ks",
        "shininess": "map_Ns",
        "transparency": "map_d",
        "normals": "norm",
    }

    def __init__(self, model):
        self.model = model

    def register(self, attr_name, path, normalize=True, tangent=False):
        key = self.texture_map.get(attr_name)
        if key is None:
            raise ValueError(f"{attr_name} not recognized.\nSupported: {self.texture_map.keys()}")
        texels = self.load_texture(path)
        if normalize:                       # [0,1] -> [-1,1]: meant for normal maps, and the default
            texels = texels * 2 - 1
        tagged = np.dtype(np.float32, metadata={"tangent": tangent})
        setattr(self.model.materials["default"], key, np.array(texels, dtype=tagged))
        self.model._revision += 1

    @staticmethod
    def load_texture(name):
        with Image.open(name) as img:
            return np.asarray(img.convert("RGB")) / 255


_skin_serial = itertools.count(1)      # every assignment of Model.skin gets its own number (the renderer's key)


class Skin:
    """What ``Model.skin`` holds: the static part of linear-blend skinning.  ``joints`` ``(len(vertices), 4)`` integers
    (kept as read-only ``int32``) and ``weights`` of the same shape (read-only ``float64``): vertex i follows the bones
    ``joints[i]`` by ``weights[i]``.  ``normals=True`` makes the vertex normals follow as well.  A ``Skin`` is never
    modified: assign a new one to change it.  ``TypeError`` for what is no array of numbers, ``ValueError`` for a wrong
    shape, weights that are not finite, joints that are not integral or negative."""

    __slots__ = ("joints", "weights", "normals")

    def __init__(self, joints, weights, normals=False):
        from ._pack import check_skin
        j, w, n = check_skin(joints, weights, normals)
        object.__setattr__(self, "joints", j)
        object.__setattr__(self, "weights", w)
        object.__setattr__(self, "normals", n)

    def __setattr__(self, name, value):
        raise AttributeError("a Skin is read-only: assign a new Skin to Model.skin")

    def __repr__(self):
        return f"Skin({len(self.joints)} vertices, normals={self.normals})"


_morph_serial = itertools.count(1)     # ... and every assignment of Model.morph


class Morph:
    """What ``Model.morph`` holds: the static part of morph targets (blend shapes).  ``targets`` is a sequence of t >= 1
    entries, each a pair ``(indices, deltas)`` -- ``(n_k,)`` integers, not negative, no index twice in one target (kept as
    read-only ``int32``), and ``(n_k, 3)`` finite numbers (read-only ``float64``) -- or a dense ``(n, 3)`` array, which
    means ``(arange(n), array)``: target k displaces vertex ``indices[j]`` by ``w[k] * deltas[j]``.  ``normal_targets`` is
    ``None`` or t entries of the same forms (``None`` among them for a target that moves no normal) whose indices count
    ``model.normals``.  A ``Morph`` is never modified: assign a new one to change it.  ``TypeError`` for what is no
    sequence of arrays of numbers, ``ValueError`` for a wrong shape or value."""

    __slots__ = ("targets", "normal_targets")

    def __init__(self, targets, normal_targets=None):
        from ._pack import check_morph
        t, n = check_morph(targets, normal_targets)
        object.__setattr__(self, "targets", t)
        object.__setattr__(self, "normal_targets", n)

    def __setattr__(self, name, value):
        raise AttributeError("a Morph is read-only: assign a new Morph to Model.morph")

    def __repr__(self):
        return f"Morph({len(self.targets)} targets, normal_targets={self.normal_targets is not None})"


class AmbientOcclusion:
    """What ``Scene.ambient_occlusion`` holds: the parameters of screen-space ambient obscurance from the z-buffer
    (``include/mi355rast.h`` has the definition, ``DESIGN.md`` section 6i the reasons).  ``radius`` is a length in world
    units: a sample at eye depth e looks ``radius * 0.5 * Hs * |P[1][1]| / e`` samples far (between 1 and 32; constant for
    an orthographic camera), and a crease that deep is fully obscured.  ``strength`` scales the darkening (0 < strength <=
    8).  ``depth_range`` (default ``3 * radius``) is the largest difference in eye depth a tap may have and still count;
    ``bias`` (default ``depth_range / 32``) is what a pair of taps must exceed before it darkens.  As float32, ``radius``,
    ``strength`` and ``depth_range`` must be finite and > 0 and ``bias`` finite and >= 0 (``ValueError``; ``TypeError`` for
    what is no real number).  An ``AmbientOcclusion`` is never modified: assign a new one to change it."""

    __slots__ = ("radius", "strength", "depth_range", "bias")

    def __init__(self, radius=0.1, strength=1.0, depth_range=None, bias=None):
        from ._pack import check_ambient_occlusion
        for name, value in zip(self.__slots__, check_ambient_occlusion(radius, strength, depth_range, bias)):
            object.__setattr__(self, name, value)

    def __setattr__(self, name, value):
        raise AttributeError("an AmbientOcclusion is read-only: assign a new one to Scene.ambient_occlusion")

    def __repr__(self):
        return (f"AmbientOcclusion(radius={self.radius!r}, strength={self.strength!r}, depth_range={self.depth_range!r}, "
                f"bias={self.bias!r})")


class DepthOfField:
    """What ``Scene.depth_of_field`` holds: a thin lens (``include/mi355rast.h`` has the definition, ``DESIGN.md`` section
    6j the reasons).  ``focus`` is the eye depth of the plane in focus, in world units; ``None`` (the default) means the eye
    depth of the camera's ``center``, ``|center - position|``, taken per view.  ``lens_radius`` is the lens' radius in
    world units: a point at eye depth e spreads over a disc of ``lens_radius * |e - focus| / focus`` world units at its own
    depth, at most 16 samples on the frame.  As float32 both must be finite and > 0 (``ValueError``; ``TypeError`` for what
    is no real number).  A ``DepthOfField`` is never modified: assign a new one to change it."""

    __slots__ = ("focus", "lens_radius")

    def __init__(self, focus=None, lens_radius=0.02):
        from ._pack import check_depth_of_field
        for name, value in zip(self.__slots__, check_depth_of_field(focus, lens_radius)):
            object.__setattr__(self, name, value)

    def __setattr__(self, name, value):
        raise AttributeError("a DepthOfField is read-only: assign a new one to Scene.depth_of_field")

    def __repr__(self):
        return f"DepthOfField(focus={self.focus!r}, lens_radius={self.lens_radius!r})"


class MotionBlur:
    """What ``Scene.motion_blur`` holds: the blur of what moved since the previous frame of the scene, gathered in one pass
    along a per-sample velocity buffer (``include/mi355rast.h`` has the definition, ``DESIGN.md`` section 6k the reasons).
    ``shutter`` is the part of the frame interval the shutter is open, in (0, 1] as float32 (``ValueError``; ``TypeError``
    for what is no real number): a sample that moved by U samples since the previous frame smears over ``shutter * |U|``,
    at most 33 samples.  ``deformation`` (a ``bool``, ``TypeError`` else; off by default, and then every frame is what it
    was without the flag) also gives the samples of a model whose ``bones``, ``morph_weights``, ``skin`` or ``morph`` changed
    since the previous frame the velocity of their face's deformed vertices, one 3 x 3 matrix per face (section 6l), not the
    velocity of the model's pose alone.  A ``MotionBlur`` is never modified: assign a new one to change it."""

    __slots__ = ("shutter", "deformation")

    def __init__(self, shutter=0.5, deformation=False):
        from ._pack import check_motion_blur, check_motion_deformation
        object.__setattr__(self, "shutter", check_motion_blur(shutter))
        object.__setattr__(self, "deformation", check_motion_deformation(deformation))

    def __setattr__(self, name, value):
        raise AttributeError("a MotionBlur is read-only: assign a new one to Scene.motion_blur")

    def __repr__(self):
        return f"MotionBlur(shutter={self.shutter!r}, deformation={self.deformation!r})"


class Bloom:
    """What ``Scene.bloom`` holds: a glow round the samples brighter than a threshold, gathered on the device from a
    resolution pyramid (``include/mi355rast.h`` has the definition, ``DESIGN.md`` section 6n the reasons).  ``threshold`` (a
    float32 in [0, 1), default 0.8) is the brightness -- the largest of a sample's three channels -- above which a sample
    glows, with ``(m - threshold) / m`` of its colour.  ``intensity`` (finite and > 0 as float32, default 0.5) is the
    strength of the glow whatever its width: the device adds ``intensity / levels`` times the sum of ``levels`` blurred
    copies.  ``levels`` (an int in 1 .. 6, default 4) is the width: every level doubles the glow's reach, in output pixels at
    any ``supersample``.  ``ValueError`` outside these ranges, ``TypeError`` for the wrong type.  A ``Bloom`` is never
    modified: assign a new one to change it."""

    __slots__ = ("threshold", "intensity", "levels")

    def __init__(self, threshold=0.8, intensity=0.5, levels=4):
        from ._pack import check_bloom
        for name, value in zip(self.__slots__, check_bloom(threshold, intensity, levels)):
            object.__setattr__(self, name, value)

    def __setattr__(self, name, value):
        raise AttributeError("a Bloom is read-only: assign a new one to Scene.bloom")

    def __repr__(self):
        return f"Bloom(threshold={self.threshold!r}, intensity={self.intensity!r}, levels={self.levels!r})"


class Layers:
    """What ``Scene.layers`` holds: the names of the per-sample data layers every frame also produces on the device, for
    ``Scene.read_layers()`` (``include/mi355rast.h`` has the definition, ``DESIGN.md`` section 6q the reasons).  ``names`` is
    a non-empty tuple of distinct names out of ``"model"``, ``"face"``, ``"material"`` (int32; -1 where no face shows),
    ``"barycentric"``, ``"position"``, ``"face_normal"``, ``"normal"`` (float32 x 3), ``"depth"`` (float32 eye depth, ``+inf``
    where no face shows) and ``"uv"`` (float32 x 2).  Only the named layers are computed, stored and copied.  ``ValueError``
    for an empty tuple, an unknown name or a name given twice, ``TypeError`` for the wrong type.  A ``Layers`` is never
    modified: assign a new one to change it."""

    __slots__ = ("names",)

    def __init__(self, names):
        from ._pack import check_layers
        object.__setattr__(self, "names", check_layers(names))

    def __setattr__(self, name, value):
        raise AttributeError("a Layers is read-only: assign a new one to Scene.layers")

    def __repr__(self):
        return f"Layers({self.names!r})"


class LightShafts:
    """What ``Scene.light_shafts`` holds: crepuscular rays, the bright sky streaming past the models towards a light's place
    on the screen, marched on the device (``include/mi355rast.h`` has the definition, ``DESIGN.md`` section 6o the reasons).
    ``light`` (an int, default 0) is an index into ``scene.lights``; an index that does not exist when a frame is issued
    raises there.  ``intensity`` (finite and > 0 as float32, default 0.5) is the gain of the rays over the frame.
    ``density`` (finite and > 0, default 0.9) is how far towards the light a sample marches: 1 reaches it, more overshoots.
    ``decay`` (in (0, 1], default 0.97) makes tap ``i`` weigh ``decay^i``; the weights are normalised, so more samples is not
    more light.  ``samples`` (an int in 1 .. 128, default 64) is the number of taps.  ``threshold`` (a float32 in [0, 1),
    default 0) is the bloom's bright factor, applied to the sky only.  ``halvings`` (1 or 2, default 2): the march runs at
    1/2 or 1/4 of the output resolution per axis.  ``ValueError`` outside these ranges, ``TypeError`` for the wrong type.
    A ``LightShafts`` is never modified: assign a new one to change it."""

    __slots__ = ("light", "intensity", "density", "decay", "samples", "threshold", "halvings")

    def __init__(self, light=0, intensity=0.5, density=0.9, decay=0.97, samples=64, threshold=0.0, halvings=2):
        from ._pack import check_light_shafts
        for name, value in zip(self.__slots__, check_light_shafts(light, intensity, density, decay, samples, threshold, halvings)):
            object.__setattr__(self, name, value)

    def __setattr__(self, name, value):
        raise AttributeError("a LightShafts is read-only: assign a new one to Scene.light_shafts")

    def __repr__(self):
        return "LightShafts(" + ", ".join(f"{name}={getattr(self, name)!r}" for name in self.__slots__) + ")"


class ToneMap:
    """What ``Scene.tone_map`` holds: the frame's last stage, an exposure and a tone curve applied on the device behind the
    bloom and in front of the debug frustum (``include/mi355rast.h`` has the definition, ``DESIGN.md`` section 6p the
    reasons).  ``operator`` is the curve: ``"linear"`` (x), ``"reinhard"`` (extended, with the ``white`` point that maps to 1)
    or ``"aces"`` (the fitted filmic curve, the default).  ``exposure`` is a fixed factor (finite and > 0 as float32), or
    ``None`` (the default): the exposure is metered from a histogram of the frame's log luminance -- 8 bins a stop -- and
    brings the geometric mean of the samples between the ``low`` and ``high`` fractions (black excluded) to ``key``, clamped
    to ``min_exposure .. max_exposure``.  ``speed`` in (0, 1] is how far a frame's exposure moves from the previous frame's
    towards its own meter: 1 (the default) meters every frame on its own and keeps nothing between frames; below 1 the scene
    adapts over frames, one frame at a time.  ``ValueError`` outside these ranges, ``TypeError`` for the wrong type.  A
    ``ToneMap`` is never modified: assign a new one to change it."""

    __slots__ = ("operator", "exposure", "key", "low", "high", "speed", "white", "min_exposure", "max_exposure")

    def __init__(self, operator="aces", exposure=None, key=0.18, low=0.0, high=1.0, speed=1.0, white=4.0, min_exposure=2.0 ** -6,
                 max_exposure=2.0 ** 6):
        from ._pack import check_tone_map
        checked = check_tone_map(operator, exposure, key, low, high, speed, white, min_exposure, max_exposure)
        for name, value in zip(self.__slots__, checked):
            object.__setattr__(self, name, value)

    def __setattr__(self, name, value):
        raise AttributeError("a ToneMap is read-only: assign a new one to Scene.tone_map")

    @property
    def adaptive(self):
        """Whether the scene carries an exposure from frame to frame: metered with ``speed`` below 1 as float32."""
        return self.exposure is None and np.float32(self.speed) < 1

    def __repr__(self):
        return "ToneMap(" + ", ".join(f"{name}={getattr(self, name)!r}" for name in self.__slots__) + ")"


class TemporalAA:
    """What ``Scene.temporal_aa`` holds: anti-aliasing spread over consecutive frames.  Every frame is rendered once, with a
    sub-sample offset of its sample grid, and its float colours are blended into the history -- the previous frame as this
    pass left it -- fetched where every sample's surface point was (the velocity buffer of ``MotionBlur``).

    ``blend`` (a float32 in (0, 1], default 0.1) is the share of the new frame: ``out = H + blend * (C - H)`` with ``H`` the
    history, clamped to the colours the 3 x 3 samples round the sample show now -- the one rejection of stale history.
    ``jitter`` (an int in 0 .. 64, default 8) is the length of the sub-sample sequence, Halton's in bases 2 and 3 minus a
    half, starting at (0, 0); 0 switches the jitter off.  A ``TemporalAA`` is never modified: assign a new one to change
    it."""

    __slots__ = ("blend", "jitter")

    def __init__(self, blend=0.1, jitter=8):
        from ._pack import check_temporal_aa
        blend, jitter = check_temporal_aa(blend, jitter)
        object.__setattr__(self, "blend", blend)
        object.__setattr__(self, "jitter", jitter)

    def __setattr__(self, name, value):
        raise AttributeError("a TemporalAA is read-only: assign a new one to Scene.temporal_aa")

    def __repr__(self):
        return f"TemporalAA(blend={self.blend!r}, jitter={self.jitter!r})"


class Model:
    """Triangle mesh: ``vertices`` (V,4), ``uv`` (T,3), ``normals`` (N,3) and ``_faces``
    (F,3,4) holding per corner ``[vertex, uv, normal, material-group]`` indices.

    ``pose`` (an addition; ``None`` by default, or a 4x4 matrix in the row-vector convention) moves the model
    between frames without a re-upload.  A model with ``pose = M`` renders as the reference renders the same model
    with its ``vertices`` replaced by the float64 array ``_fp.matmul_chain(float64(vertices), float64(M))`` -- every
    element ``rn(v[0] * M[0][j])`` followed by ``fma`` steps in ascending k.  That is upstream's ``Model @ M`` with the
    product's rounding pinned to the one order this package uses for its 4x4 products.  Like ``Model @ M`` it moves
    ``vertices`` only (vertex normals are not transformed), and its result is float64: a posed float32 model behaves
    as a float64 model (face normals, edge vectors and silhouette normals in float64).  ``vertices`` itself is never
    modified and the pose is absolute, not cumulative: ``pose = None`` gives the un-posed model back.  A scene whose
    models all have ``pose = None`` is exactly the scene without this attribute.

    ``pose_normals`` (an addition; ``False`` by default; ``True`` / ``False`` / 0 / 1, anything else ``TypeError``)
    makes the shading follow the pose.  With ``pose = M`` and ``pose_normals = True`` the model renders as the model above
    with two further replacements, both made with ``G = _pack.normal_matrix(M)``, the inverse transpose of ``M[:3, :3]``
    (cofactors over determinant in plain float64): ``normals`` by ``float32(matmul_chain(float64(float32(normals)), G))``
    and every object-space normal map (``norm`` registered with ``tangent=False``) of its materials by
    ``float32(matmul_chain(float64(texels), G))``, neither re-normalised (the reference normalises per fragment).
    Tangent-space maps follow by themselves (their frame is built from the posed corners and these normals); ``map_Kd``
    and ``map_Ks`` are never touched, and a texture array that another model holds too stays what it was for that model.
    A pose that cannot be inverted raises ``ValueError`` at whichever of the two assignments completes the pair, and
    the attribute keeps its value; without ``pose_normals`` such a pose stays legal.  With ``pose_normals = False`` or
    ``pose = None`` everything is exactly as without this attribute.

    ``skin`` and ``bones`` (additions; both ``None`` by default) deform the model by linear-blend skinning, again
    without a re-upload.  ``skin`` is a ``Skin(joints, weights, normals=False)`` -- the static part, handed to the device
    once -- and ``bones`` a ``(b, 4, 4)`` array in the row-vector convention of ``pose`` (kept as a read-only float64
    copy), the part that changes per frame.  With both set the model renders as the reference renders it with
    ``vertices`` replaced by the float64 array ``V'``: for vertex i with ``J = joints[i]``, ``W = weights[i]``,
    ``S[r][c] = _fp.dot_chain(W, (B[J[0]][r][c], B[J[1]][r][c], B[J[2]][r][c], B[J[3]][r][c]))`` -- ``rn(W0 * x0)``, then
    ``fma`` steps in ascending k -- and ``V'[i] = _fp.matmul_chain(float64(vertices[i]), S)``.  Weights are used as given:
    not normalised, and they need not sum to 1.  With ``pose = M`` as well the vertices are ``matmul_chain(V', M)``: skin
    first, then pose.  ``V'`` is float64, so a skinned float32 model behaves as a float64 one, as a posed one does.
    ``vertices`` is never modified; ``bones = None`` gives the un-skinned model back, and a scene whose models all have
    ``bones = None`` is exactly the scene without these attributes, whatever ``skin`` holds.
    With ``Skin(..., normals=True)`` normal q follows the blend matrix of its owner, the vertex at the first (face,
    corner) of ``_faces`` in row-major order whose normal column is q (a normal no corner references stays):
    ``n' = matmul_chain(float64(float32(normals[q])), S[:3, :3])``, and the model renders with ``float32(n')`` -- with
    ``pose`` and ``pose_normals`` on top with ``float32(matmul_chain(n', G))``.  ``S[:3, :3]`` itself, not its inverse
    transpose: exact in direction for bones that rotate, translate and scale uniformly; a shearing bone tilts normals.
    Tangent-space maps follow by themselves; object-space normal maps do not follow the skin (they keep what
    ``pose_normals`` does to them).  Assignments are checked at once: ``bones`` without a ``skin``, and a joint that
    reaches past the last bone -- at whichever of the two assignments completes the pair -- raise ``ValueError`` and the
    attribute keeps its value; ``skin = None`` drops ``bones`` as well.  A skin whose row count no longer equals
    ``len(vertices)`` raises ``ValueError`` at ``render()``.

    ``morph`` and ``morph_weights`` (additions; both ``None`` by default) deform the model by morph targets (blend
    shapes), again without a re-upload.  ``morph`` is a ``Morph(targets, normal_targets=None)`` -- the static part, handed
    to the device once -- and ``morph_weights`` a ``(t,)`` array (kept as a read-only float64 copy), the part that changes
    per frame.  With both set the model renders as the model whose ``vertices`` is the float64 array ``V_m``: for c in
    0..2 ``acc = float64(vertices[i][c])``, then ``acc = _fp.fma(w[k], d_k[i][c], acc)`` for every target k that lists
    vertex i, k ascending; ``V_m[i][3] = float64(vertices[i][3])``.  With ``normal_targets`` its ``normals`` is the float32
    array ``N_m``: the same chain from ``float64(float32(normals[q][c]))`` over the normal targets, rounded to float32
    once.  Weights are used as given: not clamped, they may be negative or above 1; a target that lists the vertex takes
    its step even with weight 0, so all-zero weights are not promised to equal ``morph_weights = None`` bit for bit
    (``-0.0 + 0 * d`` is ``+0.0``) -- ``None`` is the un-morphed model.  Everything else applies to that model: the order is
    morph, then skin, then pose.  ``V_m`` is float64, so a morphed float32 model behaves as a float64 one.  ``vertices``
    and ``normals`` are never modified.  Object-space normal maps do not follow a morph; tangent-space maps follow by
    themselves.  Assignments are checked at once: an index past ``len(vertices)`` (``len(normals)``), ``normal_targets``
    on a model without normals, ``morph_weights`` without a ``morph``, and a weight count other than t -- at whichever of
    the two assignments completes the pair -- raise ``ValueError`` and the attribute keeps its value; ``morph = None``
    drops ``morph_weights`` as well.  A morph whose indices no longer fit the model raises ``ValueError`` at ``render()``.

    ``auto_normals`` (an addition; ``False`` by default; ``True`` / ``False`` / 0 / 1, anything else ``TypeError``)
    rebuilds the vertex normals of a moved model from its deformed triangles, as any deformer does.  It takes effect
    while the model is moved (it has ``morph_weights``, ``bones`` or a ``pose``) and ``normals`` is not ``None``; a
    model at rest renders its authored normals -- ``pose = np.eye(4)`` rebuilds the normals of a mesh that is otherwise
    at rest.  With V the float64 vertices the model renders with (``_pack.posed_vertices``) and ``L(q)`` the faces that
    have at least one corner whose normal column is q, each once, in ascending order, ``normals[q]`` becomes the float32
    of the sum over ``L(q)`` of ``(V[b] - V[a]) x (V[c] - V[a])`` (a, b, c the vertex columns of corners 0, 1, 2; plain
    float64 operations, added in order) divided by its length (``_pack.auto_normals``); the authored ``float32(normals[q])``
    stays where ``L(q)`` is empty, the length is 0, or the sum or its length is not finite.  The direction is that of
    the face normals of the light-facing test, so a mirroring pose flips the normals with the faces.  For the vertex
    normals it supersedes ``normal_targets``, ``Skin(normals=True)`` and the vector part of ``pose_normals``: none of
    them is applied first.  Object-space normal maps keep their behaviour (re-baked under ``pose`` and ``pose_normals``,
    else untouched); tangent-space maps follow by themselves.  ``normals`` itself is never modified."""

    def __init__(self, vertices, uv, normals, faces, shadowing=False, materials=None,
                 material_group=None, clip=True, depth_test=True):
        self.vertices = vertices
        self.uv = uv
        self.normals = normals
        self._faces = faces
        self.shadowing = shadowing          # kept for signature parity; the reference never reads it
        self.clip = clip
        self.depth_test = depth_test
        self.materials = materials or {"default": Material()}
        self.material_group = material_group or ["default"]
        self.textures = TextureMaps(self)
        self.shape = None
        self.silhouette = set()             # filled by Scene.render with the last frame's edges
        self._revision = 0                  # bumped whenever device copies go stale
        self._pose = None
        self._pose_normals = False
        self._normal_matrix = None          # normal_matrix(pose) while pose_normals is on and a pose is set
        self._skin = None
        self._bones = None
        self._skin_serial = 0
        self._morph = None
        self._morph_weights = None
        self._morph_serial = 0
        self._auto_normals = False

    # -- ingest ---------------------------------------------------------------------------
    @classmethod
    def load_model(cls, name, shadowing=True):
        """Parse a Wavefront OBJ (reference: ``obj/core.py:257-318``).

        ``v`` gets ``w = 1`` appended, 2-component ``vt`` is padded with 0, polygons are
        fan-triangulated, a missing index (``1//3``) becomes -1, positive indices become
        0-based and negative ones are left as they are (NumPy-relative)."""
        verts, uvs, norms, tris = [], [], [], []
        groups = ["default"]
        current = "default"
        materials = {"default": Material()}
        folder = os.path.dirname(name)
        with open(name) as fh:
            for line in fh:
                tag, _, rest = line.partition(" ")
                if tag == "v":
                    xyz = rest.split()
                    verts.append(xyz + [1] if len(xyz) == 3 else xyz)
                elif tag == "vt":
                    st = rest.split()
                    uvs.append(st + [0] if len(st) == 2 else st)
                elif tag == "vn":
                    norms.append(rest.split())
                elif tag == "f":
                    group_id = groups.index(current) + 1
                    corners = [[(ref if ref != "" else -1) for ref in corner.split("/")] + [group_id]
                               for corner in rest.split()]
                    tris.extend(triangulate_int(corners))
                elif tag == "usemtl":
                    current = rest.split()[0]
                    if current not in groups:
                        groups.append(current)
                elif tag == "mtllib":
                    lib = os.path.join(folder, rest.split()[0])
                    if os.path.exists(lib):
                        materials.update(cls.parse_mtl(lib))
        faces = np.array(tris)
        faces = np.where(faces > 0, faces - 1, faces)
        return cls(np.array(verts, dtype=np.float32),
                   np.array(uvs, dtype=np.float32) if uvs else None,
                   np.array(norms, dtype=np.float32) if norms else None,
                   faces, shadowing, materials=materials, material_group=groups)

    @staticmethod
    def parse_mtl(mtllib):
        """``.mtl`` -> {name: Material}; ``map*``/``disp`` keys load the image next to the
        library, ``map_bump`` is stored as a tangent-space ``norm`` (``obj/core.py:321-348``)."""
        library = {}
        folder = os.path.dirname(mtllib)
        material = None
        with open(mtllib) as fh:
            for line in fh:
                if line.startswith("#") or line == "\n":
                    continue
                key, *val = line.split()
                if key == "newmtl":
                    material = library[val[0]] = Material()
                elif key.startswith("map") or key == "disp":
                    path = os.path.join(folder, val[0])
                    if not os.path.exists(path):
                        print(f"{key} {path} is not found. Recommend manually assign texture by descriptor "
                              f"Model.texture.register")
                        continue
                    dtype = np.float32
                    if key == "map_bump":
                        key, dtype = "norm", np.dtype(np.float32, metadata={"tangent": True})
                    setattr(material, key, np.array(TextureMaps.load_texture(path), dtype=dtype))
                else:
                    setattr(material, key, val)
        return library

    @property
    def pose(self):
        """``None`` or the 4x4 float64 pose matrix (read-only: assign a new matrix to move the model); see the class
        docstring."""
        return getattr(self, "_pose", None)

    @pose.setter
    def pose(self, value):
        from ._pack import check_pose, normal_matrix
        pose = check_pose(value)
        # (a pose that cannot carry the normals is refused here, and the last one stays)
        g = normal_matrix(pose) if pose is not None and self.pose_normals else None
        self._pose, self._normal_matrix = pose, g

    @property
    def pose_normals(self):
        """``False`` (the default) or ``True``: the shading normals follow ``pose``; see the class docstring."""
        return getattr(self, "_pose_normals", False)

    @pose_normals.setter
    def pose_normals(self, value):
        from ._pack import check_pose_normals, normal_matrix
        on = check_pose_normals(value)
        g = normal_matrix(self.pose) if on and self.pose is not None else None
        self._pose_normals, self._normal_matrix = on, g

    @property
    def auto_normals(self):
        """``False`` (the default) or ``True``: the vertex normals of the moved model are rebuilt from its deformed
        triangles; see the class docstring."""
        return getattr(self, "_auto_normals", False)

    @auto_normals.setter
    def auto_normals(self, value):
        from ._pack import check_auto_normals
        self._auto_normals = check_auto_normals(value)

    @property
    def skin(self):
        """``None`` or the model's ``Skin`` (joints, weights, whether the normals follow); see the class docstring."""
        return getattr(self, "_skin", None)

    @skin.setter
    def skin(self, value):
        from ._pack import check_skin_pair
        if value is None:
            self._skin, self._bones = None, None          # (no skin, no bones)
            return
        if not isinstance(value, Skin):
            raise TypeError(f"skin must be None or a Skin, got {type(value).__name__}")
        if len(value.joints) != len(self.vertices):
            raise ValueError(f"skin must have one row per vertex ({len(self.vertices)}), got {len(value.joints)}")
        check_skin_pair(value, self.bones)                # (refused here, and the last skin stays)
        self._skin, self._skin_serial = value, next(_skin_serial)

    @property
    def bones(self):
        """``None`` (the rest position) or the ``(b, 4, 4)`` float64 bone matrices (read-only: assign a new array to
        move the model); see the class docstring."""
        return getattr(self, "_bones", None)

    @bones.setter
    def bones(self, value):
        from ._pack import check_bones, check_skin_pair
        bones = check_bones(value)
        if bones is not None and self.skin is None:
            raise ValueError("bones need a skin: assign Model.skin first")
        check_skin_pair(self.skin, bones)
        self._bones = bones

    @property
    def morph(self):
        """``None`` or the model's ``Morph`` (targets, normal targets); see the class docstring."""
        return getattr(self, "_morph", None)

    @morph.setter
    def morph(self, value):
        from ._pack import check_morph_fits, check_morph_pair
        if value is None:
            self._morph, self._morph_weights = None, None      # (no morph, no weights)
            return
        if not isinstance(value, Morph):
            raise TypeError(f"morph must be None or a Morph, got {type(value).__name__}")
        check_morph_fits(value, self)
        check_morph_pair(value, self.morph_weights)        # (refused here, and the last morph stays)
        self._morph, self._morph_serial = value, next(_morph_serial)

    @property
    def morph_weights(self):
        """``None`` (the rest shape) or the ``(t,)`` float64 weights (read-only: assign a new array to move the model);
        see the class docstring."""
        return getattr(self, "_morph_weights", None)

    @morph_weights.setter
    def morph_weights(self, value):
        from ._pack import check_morph_pair, check_morph_weights
        weights = check_morph_weights(value)
        if weights is not None and self.morph is None:
            raise ValueError("morph_weights need a morph: assign Model.morph first")
        check_morph_pair(self.morph, weights)
        self._morph_weights = weights

    def __matmul__(self, other):
        self.vertices = self.vertices @ other
        self._revision += 1
        return self

    def invalidate(self):
        """Tell the renderer that ``vertices`` / ``uv`` / ``normals`` / ``_faces`` were edited IN PLACE.
        Replacing an array, ``Model @ M``, ``textures.register`` and material assignments are noticed
        by themselves, and so are in-place edits that change a sampled checksum of the arrays (scaling,
        ``[:] =``); a change to a few single elements needs this call."""
        self._revision += 1

    def face_material(self, group_index):
        """Material of a face whose first corner carries *group_index* (``obj/core.py:125``)."""
        return self.materials.get(self.material_group[group_index], self.materials["default"])


_PROJECTIONS = {}


class PositionedObject:
    def __init__(self, position, center=np.array([0, 0, 0])):
        self.scene = None
        self.position = position
        self.center = center

    @property
    def direction(self):
        # (asked for once per frame for the light, which rarely moves: the last answer is kept with the bytes it was
        # computed from)
        p, c = np.asarray(self.position), np.asarray(self.center)
        key = (p.tobytes(), c.tobytes(), p.dtype.str, c.dtype.str)
        hit = self.__dict__.get("_direction_memo")
        if hit is None or hit[0] != key:
            hit = self.__dict__["_direction_memo"] = (key, normalize(p - c).ravel())
        return hit[1].copy()

    def direction_to(self, other):
        return normalize(self.direction - other)

    def set_position(self, new_position):
        self.position = new_position
        return self


class TransformationMatrixMixin:
    """View / projection matrices of a positioned object (``obj/core.py:373-429``).

    ``lookat`` and ``MVP`` are cached on first use, as in the reference.  The 4x4 products
    use explicit fma chains (``_fp.matmul_chain``) so the constants handed to the device are
    the same on every host."""

    def __init__(self, x_offset=0, y_offset=0, projection_type=PROJECTION_TYPE.PERSPECTIVE,
                 up=np.array([0, 1, 0]), near=0.001, far=6, fovy=90):
        self.up = up
        self.projection_type = projection_type
        self.near = (np.linalg.norm(self.position)
                     if projection_type == PROJECTION_TYPE.ORTHOGRAPHIC else near)
        self.far = far
        self.fovy = fovy
        self.x_offset = x_offset
        self.y_offset = y_offset
        self.scene = None

    @property
    def projection(self):
        height, width = self.scene.resolution
        build = perspectives[self.scene.subsystem][self.projection_type][self.scene.system]
        # (a camera that moves keeps its lens: the matrix of the last few parameter sets is kept)
        try:
            key = (build, float(self.fovy), width / height, float(self.near), float(self.far))
            hit = _PROJECTIONS.get(key)
        except (TypeError, ValueError):
            return build(self.fovy, width / height, self.near, self.far)
        if hit is None:
            if len(_PROJECTIONS) > 64:
                _PROJECTIONS.clear()
            hit = _PROJECTIONS[key] = build(self.fovy, width / height, self.near, self.far)
        return hit.copy()

    @property
    def rotate(self):
        # argument order (center, position) is the reference's: the camera looks along -forward
        if self.scene.system == SYSTEM.LH:
            return look_at_rotate_lh(self.center, self.position, self.up)
        return look_at_rotate_rh(self.center, self.position, self.up)

    @property
    def translate(self):
        return looka_at_translate(self.position)

    def _constants_native(self):
        """look-at, MVP and the frustum planes in ONE call into the library's host code
        (``mr_host_camera_constants``: the same operations in the same order as the properties below, bit for bit --
        ``tests/test_host_api.py``); False where the library is not built.  A camera that moves is a new object every
        frame, and the NumPy route costs a tenth of a millisecond per camera."""
        fast = _fp.camera_constants()
        if not fast or "lookat" in self.__dict__ or "MVP" in self.__dict__:
            return False
        try:
            vec = lambda v: np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(3))
            eye, center, up, pos = vec(self.center), vec(self.position), vec(self.up), vec(self.position)
            proj = np.ascontiguousarray(self.projection, dtype=np.float64)
        except (TypeError, ValueError, AttributeError, KeyError):      # (e.g. the look-at of an object whose scene is still being built)
            return False
        if proj.shape != (4, 4):
            return False
        lookat, mvp, planes = np.empty((4, 4)), np.empty((4, 4)), np.empty((6, 4))
        fast(eye.ctypes.data, center.ctypes.data, up.ctypes.data, pos.ctypes.data, proj.ctypes.data,
             1 if self.scene.system == SYSTEM.LH else 0, lookat.ctypes.data, mvp.ctypes.data, planes.ctypes.data)
        self.__dict__["lookat"], self.__dict__["MVP"] = lookat, mvp
        self.__dict__["_planes_memo"] = (mvp, planes)
        return True

    @cached_property
    def lookat(self):
        if self._constants_native():
            return self.__dict__["lookat"]
        return _fp.matmul_chain(self.translate, self.rotate)

    @cached_property
    def MVP(self):
        if self._constants_native():
            return self.__dict__["MVP"]
        return _fp.matmul_chain(self.lookat, self.projection)

    @property
    def frustum_planes(self):
        from .plane_intersection import extract_frustum_planes
        mvp = self.MVP
        memo = self.__dict__.get("_planes_memo")
        if memo is not None and memo[0] is mvp:
            return memo[1].copy()
        return extract_frustum_planes(mvp)

    @property
    def viewport(self):
        return ViewPort(self.scene.resolution, self.far, self.near,
                        x_offset=self.x_offset, y_offset=self.y_offset)


class Camera(PositionedObject, TransformationMatrixMixin):
    def __init__(self, position, center, show=False, backface_culling=True, **kwargs):
        PositionedObject.__init__(self, np.array(position), center)
        TransformationMatrixMixin.__init__(self, **kwargs)
        self.show = show
        self.backface_culling = backface_culling


class Light(PositionedObject, TransformationMatrixMixin):
    """Point / directional / spot light with the reference's attenuation model
    ``1 / (constant + d (linear + quadratic d))`` (``obj/core.py:444-524``)."""

    def __init__(self, position, light_type=Lightning.POINT_LIGHTNING, center=(0, 0, 0),
                 color=(1., 1., 1.), ambient_strength=0, diffuse=1, specular_strength=0.5,
                 show=False, constant=1, linear=0.14, quadratic=0.07, **kwargs):
        self.color = np.array(color)
        self.light_type = light_type
        PositionedObject.__init__(self, np.array(position), np.array(center))
        self.ambient = ambient_strength * self.color
        self.show = show
        self.diffuse = diffuse
        self.specular_strength = specular_strength
        self.constant = constant
        self.linear = linear
        self.quadratic = quadratic
        TransformationMatrixMixin.__init__(self, **kwargs)

    @staticmethod
    def reflect(I, N):
        return normalize(I - 2. * (N * I).sum(axis=1)[..., np.newaxis] * N)

    @staticmethod
    def smoothstep(edge0, edge1, x_array):
        t = np.clip((x_array - edge0) / (edge1 - edge0), 0.0, 1.0)
        return t * t * (3 - 2 * t)

    def attenuation(self, fragment_position):
        d = np.linalg.norm(self.position - fragment_position, axis=1)
        return 1.0 / (self.constant + d * (self.linear + self.quadratic * d))[..., np.newaxis]


class Bound:
    """Descriptor tying a camera / light to the scene it is assigned to
    (``obj/core.py:527-555``).  State is kept per scene instance (the reference keeps it on
    the descriptor, so all its scenes share the last assignment)."""

    def __set_name__(self, owner, name):
        self._slot = "_bound_" + name

    def __set__(self, instance, value):
        instance.__dict__[self._slot] = value
        if value is None:
            return
        value.scene = instance
        if getattr(value, "show", False):
            instance.add_model(_gizmo(value))

    def __get__(self, instance, owner):
        if instance is None:
            return self
        return instance.__dict__.get(self._slot)


def _gizmo(value):
    """The little mesh that marks a ``show=True`` camera or light (``obj/core.py:532-552``): a sphere
    for a light, a camera body for a camera, scaled to a tenth and carried to the object's place by the
    inverse of its look-at matrix.  The meshes are loaded from ``obj_loader_test/sphere.obj`` /
    ``obj_loader_test/camera.obj`` relative to the working directory, exactly as upstream does -- which
    does not ship them, so without files of your own there this raises ``FileNotFoundError`` there and here.
    Vertices and normals leave as float64 (float32 @ float64), as upstream's do; the device keeps normals
    in float32 (the rounding is 6e-8 of a unit vector, far inside the float frame's 2e-6)."""
    from .transformation import scale
    is_light = isinstance(value, Light)
    sub = Model.load_model("obj_loader_test/sphere.obj" if is_light else "obj_loader_test/camera.obj",
                           shadowing=False)
    sub.clip = False
    sub = sub @ scale(0.1)
    lookat = value.lookat
    if is_light:            # a light straight above its centre has a singular look-at: upstream falls back to pinv
        try:
            sub = sub @ np.linalg.inv(lookat)
        except np.linalg.LinAlgError:
            sub = sub @ np.linalg.pinv(lookat)
        try:
            sub.normals = -sub.normals @ np.linalg.inv(lookat[mat3x3])
        except np.linalg.LinAlgError:
            sub.normals = -sub.normals @ np.linalg.pinv(lookat[mat3x3])
    else:
        sub = sub @ np.linalg.inv(lookat)
        sub.normals = -sub.normals @ np.linalg.inv(lookat[mat3x3])
    return sub


class PendingFrame:
    """A frame enqueued by ``Scene.render_async``: ``result()`` waits for it and returns the ``uint8 (H, W, 3)`` array."""

    def __init__(self, scene, lane, out, shadows, cameras):
        self._scene, self._lane, self._out, self._shadows, self._cameras = scene, lane, out, shadows, cameras
        self._motion = scene.__dict__.get("_motion_frame")      # the matrices the frame was issued with (motion_blur)
        self._motion_faces = scene.__dict__.get("_motion_faces_frame")      # ... and its per-face description (deformation)
        self._taa = scene.__dict__.get("_taa_frame")            # ... and its blend, matrices and jitter (temporal_aa)
        self._done = False

    def result(self):
        if not self._done:
            scene = self._scene
            ok = scene._backend().render_wait(self._lane)
            scene.__dict__.get("_pending", {}).pop(self._lane, None)
            if not ok:          # a work list overflowed (now grown): render this frame's view again, synchronously
                now = (scene.camera, scene.debug_camera)
                scene.camera, scene.debug_camera = self._cameras
                if scene.motion_blur is not None and self._motion is not None:
                    scene.__dict__["_motion_replay"] = self._motion      # the same matrices as the first attempt
                    scene.__dict__["_motion_faces_replay"] = self._motion_faces
                if scene.temporal_aa is not None and self._taa is not None:
                    scene.__dict__["_taa_replay"] = self._taa            # the same jitter and matrices, the same history
                try:
                    self._out = scene.render(shadows=self._shadows)
                finally:
                    scene.camera, scene.debug_camera = now
                    scene.__dict__.pop("_motion_replay", None)
                    scene.__dict__.pop("_motion_faces_replay", None)
                    scene.__dict__.pop("_taa_replay", None)
            self._done = True
        return self._out


class Accumulation:
    """A weighted sum of the scene's float frames on the device, finalised once (``Scene.accumulate``).

    The sum lives on the sample grid ``(Hs, Ws)`` of its sub-frames -- ``(s*H, s*W)`` for ``Scene.supersample = s`` --
    rows bottom-up like every tap.  With F_k the float32 frame of sub-frame k (after the overlay, after the sum over
    the lights) and w_k its weight as a float32, every operation float32 and rounded on its own::

        A_0 = w_0 * F_0
        A_k = A_{k-1} + (w_k * F_k)
        M   = mean of A over each s x s block      (row by row from the block's bottom-left sample, times 1 / s^2)
        R   = min(M * scale, 1)
        out = uint8(R ** 0.8 * 255), rows flipped  (uint8 (H, W, 3), row 0 = top)

    ``scale`` defaults to ``float32(1 / sum of the weights)``.  Averaging ``render()``'s uint8 frames instead averages
    after the gamma and after the quantisation: wrong, and banded.  No sub-frame leaves the device; ``result()`` copies
    the finished bytes.  A scene has one accumulation at a time: ``close()`` it (or leave its ``with`` block) before
    asking for another.  ``render()`` and ``render_async()`` in between do not disturb it."""

    def __init__(self, scene):
        self._scene, self._open, self._begun = scene, True, False
        self._count, self._weight_sum = 0, 0.0

    @property
    def count(self):
        """Sub-frames added so far."""
        return self._count

    @property
    def weight_sum(self):
        """Sum of the weights as given (float64)."""
        return self._weight_sum

    def _check_open(self):
        if not self._open:
            raise RuntimeError("this accumulation is closed")

    def add(self, weight=1.0, shadows=True):
        """Render the scene AS IT IS NOW -- camera, lights, poses, bones, morph weights, ``supersample``,
        ``draw_debug_frustum`` -- and add the frame times *weight* (finite and > 0 as float32).  The first ``add`` fixes
        the resolution and ``supersample``: a later one that differs raises ``ValueError``.  Returns ``self``."""
        from ._pack import check_accum_factor
        self._check_open()
        weight = check_accum_factor(weight, "weight")
        scene = self._scene
        scene._check_lights()
        backend = scene._backend()
        if not self._begun:
            backend.accum_begin()
            self._begun = True
        backend.accum_add(scene, weight, shadows=shadows, overlay=scene.draw_debug_frustum)
        self._count += 1
        self._weight_sum += weight
        return self

    def result(self, scale=None):
        """The sum as it stands, finalised: ``uint8 (H, W, 3)``, row 0 = top.  The sum stays, so ``add`` may follow
        (progressive refinement).  ``RuntimeError`` before the first ``add``."""
        from ._pack import check_accum_factor, default_accum_scale
        self._check_open()
        scale = default_accum_scale(self._weight_sum) if scale is None and self._count else scale
        if scale is not None:
            scale = check_accum_factor(scale, "scale")
        if self._count == 0:
            raise RuntimeError("nothing accumulated yet: add() a sub-frame first")
        return self._scene._backend().accum_resolve(scale)

    def float_frame(self):
        """The tap: the sum A as it stands, ``float32 (Hs, Ws, 3)``, rows bottom-up."""
        self._check_open()
        if self._count == 0:
            raise RuntimeError("nothing accumulated yet: add() a sub-frame first")
        return self._scene._backend().accum_read()

    def close(self):
        """Gives the scene's accumulation back (the device keeps the buffer for the next one)."""
        if self._open:
            self._open = False
            if self._scene.__dict__.get("_accumulation") is self:
                self._scene.__dict__["_accumulation"] = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class Scene:
    """``Scene(camera, light, shadows, debug_camera, resolution=(H, W), system, subsystem,
    skymap)`` -- reference ``obj/core.py:558-640``.

    * ``debug_camera`` also clips fragments, exactly as in the reference
      (``obj/triangular.py:39,83``); ``None`` means "same as ``camera``" (the reference raises).
    * ``shadows`` is accepted and ignored like upstream (``obj/core.py:568``): the stencil
      pass always runs.  Use ``render(shadows=False)`` to skip it explicitly.
    * ``supersample`` (an addition; 1, 2 or 4, default 1): ordered-grid anti-aliasing.  With s > 1 the
      frame is rendered on the sample grid ``(s*H, s*W)`` -- upstream's frame of the same scene at that
      resolution, the camera's ``x_offset`` / ``y_offset`` times s, overlay included -- and output pixel
      (x, y) is the mean of samples (s*x + i, s*y + j), 0 <= i, j < s (rows counted from the bottom like
      the reference's buffers: the grid is anchored at the pixel's lower corner), finalised once.
      ``resolution`` stays the OUTPUT size, ``render()`` returns ``uint8 (H, W, 3)``; the device taps
      (``read_z`` ...), ``last_stats`` and the ``verbose`` face report count the sample grid.  Neither
      ``resolution`` nor the camera is changed.  Split frames (``multigpu``) refuse s > 1.
    * ``add_light(light)`` (an addition; up to four lights with ``light``): further shadow-casting lights in the
      same frame -- visibility once, a stencil pass and an additive lighting pass per light; see ``add_light``.
      ``verbose`` and split frames (``multigpu``) refuse more than one light.
    * ``accumulate()`` / ``render_mean(n, step)`` (an addition): a weighted sum of float frames on the device, finalised
      once -- see ``Accumulation``.
    * ``ambient_occlusion`` (an addition; ``None`` by default, or an ``AmbientOcclusion``): screen-space ambient
      obscurance from the z-buffer, applied on the device to the float frame of every frame of the scene -- ``render``,
      ``render_async``, ``render_frames``, the sub-frames of an ``Accumulation`` -- after the sum over the lights and before
      the debug frustum, which is not darkened.  The whole colour is darkened, not the ambient term alone; with several
      lights it is applied once; a ``depth_test=False`` model is shaded by what the z-buffer holds behind it.  Split
      frames (``row_band``, ``multigpu``) refuse it.  With ``None`` a scene enqueues exactly what it did without it.
    * ``depth_of_field`` (an addition; ``None`` by default, or a ``DepthOfField``): a thin lens' blur gathered on the
      device from the float frame and the z-buffer of every frame of the scene, in one pass -- after the lights' sum and
      the obscurance, before the debug frustum, whose lines stay sharp.  One layer (what a lens sees round an occluder is
      not in the frame), no circle wider than 16 samples; the sky blurs too.  Split frames (``row_band``, ``multigpu``)
      refuse it.  With ``None`` a scene enqueues exactly what it did without it.
    * ``motion_blur`` (an addition; ``None`` by default, or a ``MotionBlur``): every frame is blurred along the screen-space
      motion of its samples since the PREVIOUS frame of this scene -- the camera and every model's ``pose`` as they were
      when that frame was issued by ``render()``, ``render_async()`` or a view of ``render_frames()``, in issue order.
      One pass on the device behind the obscurance and the depth of field, before the debug frustum, whose lines stay
      sharp; ``scene._backend().read_velocity()`` returns the velocity buffer.  The first frame after ``motion_blur`` is
      assigned, after ``reset_motion()`` or after the model list changed has no previous frame and is ``render()``'s byte
      for byte.  Bones and morph weights move nothing unless ``MotionBlur(deformation=True)``; one layer only.  Split
      frames (``row_band``, ``multigpu``), ``accumulate()`` and ``render_mean()`` refuse it.  With ``None`` a scene
      enqueues exactly what it did without it.
    * ``temporal_aa`` (an addition; ``None`` by default, or a ``TemporalAA``): anti-aliasing spread over consecutive frames.
      Every frame is rendered once with a sub-sample offset and blended on the device into the history, the previous
      frame fetched where every sample's surface point was -- behind the lights' sum and the obscurance, in front of the
      depth of field and the motion blur, which gather from the stabilised frame, and of the debug frustum.  It shares the
      previous frame's camera and poses with ``motion_blur`` (one velocity pass serves both);
      ``scene._backend().read_velocity()`` and ``read_history()`` return the velocity and the history.  The history is
      forgotten when ``temporal_aa`` or ``motion_blur`` is assigned, by ``reset_motion()``, when the model list changed and
      when the sample grid's size changed (``resolution``, ``supersample``): the next frame is ``render()``'s byte for
      byte.  One frame of the scene at a time: ``render_async()`` refuses while another frame is pending, and
      ``render_frames()`` waits for every frame before it issues the next.  Split frames (``row_band``, ``multigpu``),
      ``accumulate()`` and ``render_mean()`` refuse it.  With ``None`` a scene enqueues exactly what it did without it.
    * ``bloom`` (an addition; ``None`` by default, or a ``Bloom``): a glow round the samples brighter than a threshold,
      gathered on the device from a resolution pyramid behind the motion blur and in front of the debug frustum, whose
      lines do not glow.  A frame no sample of which exceeds the threshold is ``render()``'s byte for byte.  The pass
      keeps nothing between frames: it composes with ``accumulate()``, ``render_mean()``, ``render_frames()``,
      ``render_async()``, several lights and every other pass; the history of ``temporal_aa`` never holds glow.  Split
      frames (``row_band``, ``multigpu``) refuse it.  With ``None`` a scene enqueues exactly what it did without it.
    * ``light_shafts`` (an addition; ``None`` by default, or a ``LightShafts``): the sky's light streaming past the models
      towards one of the scene's lights, marched on the device behind the motion blur and in front of the bloom, which
      may make a bright shaft glow; the debug frustum's lines are neither sources nor brightened.  A frame whose light
      lies behind the camera, or without sky above the threshold, is ``render()``'s byte for byte.  The pass keeps nothing
      between frames and composes like ``bloom``; the history of ``temporal_aa`` never holds shafts.  Split frames
      (``row_band``, ``multigpu``) refuse it.  With ``None`` a scene enqueues exactly what it did without it.
    * ``tone_map`` (an addition; ``None`` by default, or a ``ToneMap``): the frame's last stage on the device, behind the
      bloom and in front of the debug frustum, whose lines keep their colours -- an exposure, fixed or metered from a
      luminance histogram of the frame, and a tone curve, so that what bloom and light shafts add does not burn out to
      white.  ``ToneMap("linear", exposure=1.0)`` is ``render()``'s frame byte for byte.  Metered with ``speed=1`` or fixed,
      the pass keeps nothing between frames and composes like ``bloom`` (sub-frames of ``accumulate()`` are tone-mapped
      before they are summed).  With ``speed`` below 1 the scene adapts: a frame's exposure becomes the previous one when
      the frame is complete, one frame is issued at a time (as under ``temporal_aa``), ``accumulate()`` refuses, and the
      exposure is forgotten by ``reset_motion()`` and whenever ``tone_map`` is assigned.  The history of ``temporal_aa``
      never holds tone-mapped colours.  Split frames (``row_band``, ``multigpu``) refuse it.
    * ``layers`` (an addition; ``None`` by default, or a ``Layers``): every frame also produces the named per-sample data
      layers on the device -- model, face and material ids, perspective-correct barycentrics, eye depth, world position,
      face and shading normals, texture coordinates -- right behind the tile kernel, from the winner map and the face
      records alone; ``read_layers()`` returns them for the last frame.  The frame's bytes are what they are without it.
      It composes with ``supersample`` (the layers live on the sample grid), poses, skins, morphs, ``temporal_aa`` (the
      layers follow the jittered grid the frame was rendered on) and every post pass.  Split frames (``row_band``,
      ``multigpu``) and ``accumulate()`` refuse it.
    """

    camera = Bound()
    light = Bound()
    debug_camera = Bound()

    def __init__(self, camera=None, light=None, shadows=False, debug_camera=None,
                 resolution=(1500, 1500), system=SYSTEM.RH, subsystem=SUBSYSTEM.DIRECTX,
                 skymap=None, device=None, supersample=1):
        self.system = system
        self.subsystem = subsystem
        self.models: List[Model] = []
        self.camera = camera if camera is not None else Camera(position=(0, 0, 1), center=(0, 0, 0))
        self.light = light if light is not None else Light(position=(1, 1, 1))
        self.debug_camera = debug_camera
        self.resolution = resolution
        self.supersample = supersample
        self.skybox = skymap
        self.shadows = shadows
        self.device = device
        self.draw_debug_frustum = True      # like the reference, which always overlays it (core.py:638); switchable here
        self.verbose = False                # the reference always prints its face histogram (core.py:634-636)
        self._renderer = None

    @property
    def supersample(self):
        """Samples per output pixel and axis: 1, 2 or 4 (see the class docstring)."""
        return self._supersample

    @supersample.setter
    def supersample(self, value):
        from ._pack import check_supersample
        self._supersample = check_supersample(value)

    @property
    def ambient_occlusion(self):
        """``None`` (off, the default) or the scene's ``AmbientOcclusion`` (see the class docstring)."""
        return self.__dict__.get("_ambient_occlusion")

    @ambient_occlusion.setter
    def ambient_occlusion(self, value):
        if value is not None and not isinstance(value, AmbientOcclusion):
            raise TypeError(f"ambient_occlusion must be None or an AmbientOcclusion, got {type(value).__name__}")
        self.__dict__["_ambient_occlusion"] = value

    @property
    def depth_of_field(self):
        """``None`` (off, the default) or the scene's ``DepthOfField`` (see the class docstring)."""
        return self.__dict__.get("_depth_of_field")

    @depth_of_field.setter
    def depth_of_field(self, value):
        if value is not None and not isinstance(value, DepthOfField):
            raise TypeError(f"depth_of_field must be None or a DepthOfField, got {type(value).__name__}")
        self.__dict__["_depth_of_field"] = value

    @property
    def motion_blur(self):
        """``None`` (off, the default) or the scene's ``MotionBlur`` (see the class docstring)."""
        return self.__dict__.get("_motion_blur")

    @motion_blur.setter
    def motion_blur(self, value):
        if value is not None and not isinstance(value, MotionBlur):
            raise TypeError(f"motion_blur must be None or a MotionBlur, got {type(value).__name__}")
        self.__dict__["_motion_blur"] = value
        self.reset_motion()

    def reset_motion(self):
        """Forgets the previous frame's camera and poses, the history of ``temporal_aa`` and the exposure an adaptive
        ``tone_map`` carried: the next frame has identity motion, no history and no previous exposure."""
        self.__dict__["_motion_prev"] = None
        self.__dict__["_taa_forget"] = True
        self.__dict__["_tone_forget"] = True

    @property
    def temporal_aa(self):
        """``None`` (off, the default) or the scene's ``TemporalAA`` (see the class docstring)."""
        return self.__dict__.get("_temporal_aa")

    @temporal_aa.setter
    def temporal_aa(self, value):
        if value is not None and not isinstance(value, TemporalAA):
            raise TypeError(f"temporal_aa must be None or a TemporalAA, got {type(value).__name__}")
        self.__dict__["_temporal_aa"] = value
        self.reset_motion()

    @property
    def bloom(self):
        """``None`` (off, the default) or the scene's ``Bloom`` (see the class docstring)."""
        return self.__dict__.get("_bloom")

    @bloom.setter
    def bloom(self, value):
        if value is not None and not isinstance(value, Bloom):
            raise TypeError(f"bloom must be None or a Bloom, got {type(value).__name__}")
        self.__dict__["_bloom"] = value

    @property
    def light_shafts(self):
        """``None`` (off, the default) or the scene's ``LightShafts`` (see the class docstring)."""
        return self.__dict__.get("_light_shafts")

    @light_shafts.setter
    def light_shafts(self, value):
        if value is not None and not isinstance(value, LightShafts):
            raise TypeError(f"light_shafts must be None or a LightShafts, got {type(value).__name__}")
        self.__dict__["_light_shafts"] = value

    @property
    def tone_map(self):
        """``None`` (off, the default) or the scene's ``ToneMap`` (see the class docstring)."""
        return self.__dict__.get("_tone_map")

    @tone_map.setter
    def tone_map(self, value):
        if value is not None and not isinstance(value, ToneMap):
            raise TypeError(f"tone_map must be None or a ToneMap, got {type(value).__name__}")
        self.__dict__["_tone_map"] = value
        self.__dict__["_tone_forget"] = True      # (the exposure another description adapted is not this one's)

    @property
    def layers(self):
        """``None`` (off, the default) or the scene's ``Layers`` (see the class docstring)."""
        return self.__dict__.get("_layers")

    @layers.setter
    def layers(self, value):
        if value is not None and not isinstance(value, Layers):
            raise TypeError(f"layers must be None or a Layers, got {type(value).__name__}")
        self.__dict__["_layers"] = value

    def read_layers(self):
        """The data layers of the last frame, which was rendered with ``layers`` set: a dict name -> NumPy array on the sample
        grid, ``(s*H, s*W)`` or ``(s*H, s*W, c)``, rows bottom-up like ``read_velocity()``, and like it of the frame enqueued
        last -- with frames in flight (``render_async``, ``render_frames``) that is the newest one issued.  ``ValueError``
        where that frame computed none."""
        if self._renderer is None:
            raise ValueError("read_layers: nothing rendered yet")
        return self._renderer.read_layers()

    @property
    def last_stats(self):
        """Statistics of the last frame (``mr_stats``), fetched from the device when asked for."""
        return None if self._renderer is None else self._renderer.last_stats

    def add_model(self, model):
        self.models.append(model)

    # -- more than one light (an addition: upstream's Scene has exactly one) -------------------
    MAX_LIGHTS = 4

    def add_light(self, light):
        """A further shadow-casting light, up to four in all.  ``scene.light`` stays light 0.  With F_k the float
        frame the scene gives with light k alone, a frame shows ``min(F_0 + F_1 + ..., 1)`` where a face covers the
        pixel (float32 adds, in the order of the lights) and F_0's background elsewhere; every F_k keeps upstream's
        ``clip(0.05, 1)``, so a pixel no light reaches shows 0.05 per light.  Lights may be of different kinds and
        are read again at every ``render()``.  A ``show=True`` light gets its gizmo like ``scene.light`` does."""
        if not isinstance(light, Light):
            raise TypeError(f"add_light expects a Light, got {type(light).__name__}")
        extra = self.__dict__.setdefault("_extra_lights", [])
        if 1 + len(extra) >= self.MAX_LIGHTS:
            raise ValueError(f"a scene has at most {self.MAX_LIGHTS} lights")
        light.scene = self
        if getattr(light, "show", False):
            self.add_model(_gizmo(light))
        extra.append(light)

    @property
    def lights(self):
        """``[scene.light, *extra lights]`` (a copy: change the set with ``add_light`` / ``clear_lights``)."""
        return [self.light, *self.__dict__.get("_extra_lights", ())]

    def clear_lights(self):
        """Drops the lights added with ``add_light``; ``scene.light`` stays."""
        self.__dict__["_extra_lights"] = []

    def _check_lights(self):
        if len(self.lights) > 1 and self.verbose:
            raise ValueError("scene.verbose is not available with more than one light: upstream's per-face status "
                             "depends on the one stencil buffer")

    # -- rendering ------------------------------------------------------------------------
    def _backend(self):
        if self._renderer is None:
            from ._native import DeviceRenderer
            self._renderer = DeviceRenderer(self.device)
        return self._renderer

    def render(self, shadows=True, row_band=None):
        """Render one frame on the GPU and return ``uint8 (H, W, 3)`` (row 0 = top).

        Unlike the reference, repeated calls give the same frame: the silhouette is rebuilt
        from scratch every frame instead of being toggled in ``model.silhouette``.  Like the
        reference, the frame carries the debug camera's frustum as red lines (``obj/core.py:638``);
        ``scene.draw_debug_frustum = False`` leaves it out.  With ``scene.verbose`` (off by default)
        the three lines the reference prints per model after its lit pass (``obj/core.py:634-636``)
        are reproduced from the device's per-face codes.  With ``scene.supersample`` = s > 1 the frame is the
        s x s box-filtered mean of the sample grid (class docstring); *row_band* counts output rows."""
        self._check_lights()
        backend = self._backend()
        report = self.verbose and row_band is None
        # the debug camera's frustum, drawn by the device into its own frame and z-buffer right after the
        # tile kernel (obj/core.py:638).  A row band of a multi-GPU split cannot draw it alone (the lines test z at
        # pixels other devices own): multigpu.BandRenderer(overlay=True) gathers the touched pixels' state with
        # the rows and replays the overlay on the assembled frame
        overlay = self.draw_debug_frustum and row_band is None
        out = backend.render(self, shadows=shadows, row_band=row_band, face_status=report, counters=False,
                             keep_buffers=False, timing=False, overlay=overlay)
        if report:
            self._print_face_report(backend.read_face_status())
        return out

    def render_async(self, shadows=True):
        """``render()`` without the wait: the frame's kernels and the copy of its uint8 rows to the host are
        enqueued and the call returns a ``PendingFrame``; ``.result()`` hands out the array (the same bytes
        ``render()`` would have returned).  Up to four frames may be pending on one scene; the copy of frame i
        (longer than the frame's kernels at 1080p) then runs beside the kernels of frame i + 1 and beside the
        host's preparation of frame i + 2.  The reference has no such call: it is an addition for sequences."""
        self._check_lights()
        pending = self.__dict__.setdefault("_pending", {})
        if self.temporal_aa is not None and pending:
            raise ValueError("temporal_aa takes one frame of the scene at a time: another frame is pending, take its "
                             "result() first (every frame reads the history the frame before it left)")
        if self.tone_map is not None and self.tone_map.adaptive and pending:
            raise ValueError("an adaptive tone_map (speed < 1) takes one frame of the scene at a time: another frame is pending, "
                             "take its result() first (every frame reads the exposure the frame before it left)")
        backend = self._backend()
        lane = next((k for k in range(backend.ASYNC_LANES) if k not in pending), None)
        if lane is None:
            raise RuntimeError("four frames of this scene are already pending: take one's result() first")
        out = backend.render_async(self, lane, shadows=shadows, overlay=self.draw_debug_frustum)
        frame = PendingFrame(self, lane, out, shadows, (self.camera, self.debug_camera))
        pending[lane] = frame
        return frame

    def render_frames(self, views, shadows=True, depth=2):
        """Frames of a sequence: for every ``(camera, debug_camera)`` pair of *views* the scene's cameras are set
        and a frame is rendered; yields the uint8 arrays in order, *depth* frames in flight (``render_async``).  Under
        a ``temporal_aa`` every frame reads the history the frame before it left (under an adaptive ``tone_map``, its
        exposure): one frame is issued at a time, and its verdict is waited for before the next is issued, whatever
        *depth* says."""
        if self.temporal_aa is not None or (self.tone_map is not None and self.tone_map.adaptive):
            depth = 1
        queue = []
        try:
            for camera, debug_camera in views:
                self.camera, self.debug_camera = camera, debug_camera
                queue.append(self.render_async(shadows=shadows))
                if len(queue) >= max(1, int(depth)):
                    yield queue.pop(0).result()
            while queue:
                yield queue.pop(0).result()
        finally:
            for frame in queue:
                frame.result()

    def accumulate(self):
        """An ``Accumulation`` of this scene's frames (an addition): ``add(weight)`` renders the scene as it is now and
        adds its float frame on the device, ``result()`` finalises the weighted sum once -- motion blur over poses or
        bones, a soft shadow as a light averaged over positions, a jittered camera, progressive refinement.  Usable as
        a context manager; one per scene at a time (``RuntimeError`` while another is open).  Touches no device before
        the first ``add``."""
        if self.__dict__.get("_accumulation") is not None:
            raise RuntimeError("this scene already has an open accumulation: close() it first")
        if self.motion_blur is not None:
            raise ValueError("motion_blur is not available inside accumulate() / render_mean(): the accumulation is the "
                             "other way to blur motion, and its sub-frames have no previous frame")
        if self.temporal_aa is not None:
            raise ValueError("temporal_aa is not available inside accumulate() / render_mean(): the accumulation is the "
                             "other way to spread samples over frames, and its sub-frames have no history")
        if self.tone_map is not None and self.tone_map.adaptive:
            raise ValueError("an adaptive tone_map (speed < 1) is not available inside accumulate() / render_mean(): its "
                             "sub-frames have no previous frame (speed=1 or a fixed exposure is)")
        if self.layers is not None:
            raise ValueError("layers is not available inside accumulate() / render_mean(): a sum of frames has no one winner a sample")
        acc = self.__dict__["_accumulation"] = Accumulation(self)
        return acc

    def render_mean(self, n, step, shadows=True):
        """The mean of *n* sub-frames: ``step(k)`` is called before sub-frame k (move a light, a pose, the camera),
        every sub-frame weighs 1 and the scale is the default 1 / n.  Returns ``uint8 (H, W, 3)``."""
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError(f"render_mean needs n >= 1 sub-frames, got {n!r}")
        with self.accumulate() as acc:
            for k in range(int(n)):
                step(k)
                acc.add(1.0, shadows=shadows)
            return acc.result()

    def _print_face_report(self, status):
        from .triangular import Errors
        first = 0
        for model in self.models:
            codes = status[first:first + len(model._faces)]
            first += len(model._faces)
            histogram = {err: int((codes == err.value).sum()) for err in Errors}
            print('Total faces', len(model._faces))
            print('Face rendered', int((codes == 0).sum()))
            print('Discarded', histogram)

    def close(self):
        open_acc = self.__dict__.get("_accumulation")
        if open_acc is not None:                 # (its sum goes with the device's scene)
            open_acc.close()
        if self._renderer is not None:
            self._renderer.close()
            self._renderer = None
            self.__dict__["_taa_forget"] = True      # (the history of temporal_aa went with the device's scene)
