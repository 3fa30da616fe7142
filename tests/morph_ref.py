"""What a morphed model must be (the contract of ``Model.morph`` / ``Model.morph_weights``), restated without the feature.

A model with ``morph = Morph(targets, normal_targets)`` and ``morph_weights = w`` renders as the same model with its
``vertices`` replaced by the float64 array ``V_m``: ``acc = float64(vertices[i][c])``, then ``acc = fma(w[k], d_k[i][c], acc)``
for every target k that lists vertex i, k ascending (c in 0..2; the fourth component passes through).  With
``normal_targets`` its ``normals`` is replaced by ``float32`` of the same chain from ``float64(float32(normals[q][c]))``.
Skin, bones, pose and pose_normals apply to that model: morph, then skin, then pose.

``twin`` builds that scene: the recipe afresh, the arrays replaced, no morph set; ``skin``, ``bones``, ``pose`` and
``pose_normals`` go through the existing attributes, which are pinned to their own twins (pose_ref.py, skin_ref.py).  The
arrays are formed here with ``_fp.fma`` alone (pure Python), so the twin does not depend on the code under test."""
import functools
import math

import numpy as np

import pose_ref
import skin_ref
from py_numpy_renderer_amd import _fp

RECIPES = pose_ref.RECIPES
SHAPE_NAMES = ("dense2", "bands", "slices", "edge256", "edge257")
N_TARGETS = {"dense2": 2, "bands": 5, "slices": 5, "edge256": 256, "edge257": 257, "normals": 5, "bands50": 50}
BANDS = ((0.0, 0.25), (0.35, 0.6), (0.5, 0.8), (0.55, 0.7), (0.75, 1.0))      # vertices listed by 0, 1, 2 and 3 targets
BAND_WEIGHTS = (0.8, 0.0, 1.5, -0.4, 0.6)                                      # exactly 0.0, and above 1


def _frame(vertices):
    """(longest axis, the two others, every vertex's place along the longest in [0, 1], the box's longest side)."""
    xyz = np.asarray(vertices, dtype=np.float64)[:, :3]
    axis, t = skin_ref._along(vertices)
    return axis, (axis + 1) % 3, (axis + 2) % 3, t, float((xyz.max(axis=0) - xyz.min(axis=0)).max())


def _band_targets(model, bands, size):
    """One sparse target per band of the longest axis: a bump across the band, turned a little further per band."""
    axis, a1, a2, t, s = _frame(model.vertices)
    targets = []
    for k, (lo, hi) in enumerate(bands):
        index = np.flatnonzero((t >= lo) & (t <= hi))
        bump = size * s * (0.4 + 0.6 * np.sin(np.pi * (t[index] - lo) / (hi - lo)))
        delta = np.zeros((len(index), 3))
        delta[:, a1], delta[:, a2], delta[:, axis] = bump * math.cos(0.9 * k), bump * math.sin(0.9 * k), 0.25 * bump
        targets.append((index, delta))
    return targets


def shape(model, name, frame=0):
    """(targets, normal_targets or None, weights) of a deterministic morph derived from the model's vertex coordinates;
    deltas are a few hundredths to a tenth of the bounding box.  *frame* moves the weights on.

    dense2    two dense targets, weights (0.7, -0.3)
    bands     five sparse targets on overlapping bands along the longest axis (``BANDS``, ``BAND_WEIGHTS``)
    bands50   fifty such bands (for timing)
    slices    index sets at the seams of the 64-vertex slices: 0, 63, 64, 255, 256 and the last vertex; a lone vertex in
              an otherwise empty slice (401); a hub (517) that every target with entries lists, in a slice whose
              neighbours list nothing; one target without entries.  What the model is too small for falls away.
    edge256   t = 256: vertex i is listed by the targets i mod t, t - 1 - (i mod t) and 0
    edge257   the same with t = 257
    normals   ``bands`` plus normal targets on the normals those vertices own; one entry ``None``"""
    n = len(model.vertices)
    axis, a1, a2, t, s = _frame(model.vertices)
    normal_targets = None
    if name == "dense2":
        first, second = np.zeros((n, 3)), np.zeros((n, 3))
        first[:, a1] = 0.08 * s * (0.3 + np.sin(np.pi * t))
        second[:, a2], second[:, axis] = 0.05 * s * (2.0 * t - 1.0), 0.03 * s * t * t
        targets, weights = [first, second], [0.7, -0.3]
    elif name in ("bands", "normals"):
        targets, weights = _band_targets(model, BANDS, 0.07), list(BAND_WEIGHTS)
        if name == "normals":
            owners = np.asarray(skin_ref.normal_owners(model))
            normal_targets = []
            for k, (index, _) in enumerate(targets):
                owned = np.flatnonzero(np.isin(owners, index))
                delta = np.zeros((len(owned), 3))
                delta[:, a1], delta[:, a2], delta[:, axis] = 0.45 * math.cos(1.3 * k), 0.45 * math.sin(1.3 * k), 0.2
                normal_targets.append(None if k == 3 else (owned, delta))
    elif name == "bands50":
        bands = [(0.018 * k, 0.018 * k + 0.1) for k in range(50)]
        targets, weights = _band_targets(model, bands, 0.04), [0.5 * math.cos(0.37 * k) for k in range(50)]
    elif name == "slices":
        hub = 517 if n > 517 else n // 2
        sets = [[0, 63, 64, 255, 256, n - 1, hub], [], [401, hub], [63, 64, hub], [n - 1, 0, hub]]
        targets = []
        for k, wanted in enumerate(sets):
            index = np.array(sorted({i for i in wanted if 0 <= i < n}), dtype=np.int64)
            delta = np.array([[0.09 * s * math.cos(i + k), 0.09 * s * math.sin(i + k), 0.05 * s] for i in index]).reshape(-1, 3)
            targets.append((index, delta))
        weights = [0.9, 0.5, -0.6, 1.2, 0.35]
    elif name in ("edge256", "edge257"):
        count = N_TARGETS[name]
        m = np.arange(n) % count
        everyone = np.zeros((n, 3))
        everyone[:, a1] = 0.05 * s * (0.3 + np.sin(np.pi * t))
        targets = [(np.arange(n), everyone)]
        for k in range(1, count):
            index = np.flatnonzero((m == k) | (m == count - 1 - k))
            delta = np.zeros((len(index), 3))
            delta[:, a1], delta[:, a2], delta[:, axis] = 0.03 * s * math.cos(0.11 * k), 0.03 * s * math.sin(0.11 * k), 0.01 * s
            targets.append((index, delta))
        weights = [0.5] + [0.8 * math.cos(0.7 * k) for k in range(1, count - 1)] + [-0.45]
    else:
        raise KeyError(name)
    weights = np.array(weights, dtype=np.float64)
    if frame:
        weights = weights + 0.06 * frame * np.cos(np.arange(len(weights)) + 0.5 * frame)
    return targets, normal_targets, weights


def _pairs(targets):
    return [(np.arange(len(e)), np.asarray(e, dtype=np.float64)) if isinstance(e, np.ndarray) else
            (np.asarray(e[0], dtype=np.int64), np.asarray(e[1], dtype=np.float64)) for e in targets]


def chain(base, targets, weights):
    """The contract's chain on the first three columns of the float64 array *base*, with ``_fp.fma`` alone."""
    out = np.array(base, dtype=np.float64)
    for k, (index, delta) in enumerate(_pairs(targets)):
        w = float(weights[k])
        for i, d in zip(index.tolist(), delta.tolist()):
            for c in range(3):
                out[i, c] = _fp.fma(w, d[c], float(out[i, c]))
    return out


def morphed_vertices(vertices, targets, weights):
    return chain(np.asarray(vertices).astype(np.float64), targets, weights)


def morphed_normals(normals, normal_targets, weights):
    """N_m (float32) of every normal."""
    n = np.ascontiguousarray(normals, dtype=np.float32)
    kept = [(np.zeros(0, dtype=np.int64), np.zeros((0, 3))) if e is None else e for e in normal_targets]
    out = n.copy()
    out[:, :3] = chain(n[:, :3].astype(np.float64), kept, weights).astype(np.float32)
    return out


def build(api, recipe):
    return pose_ref.build(api, recipe)


def apply(api, scene, shapes, frame=0):
    """``morph`` and ``morph_weights`` on the models of *shapes* (``{model index: shape name}``)."""
    from py_numpy_renderer_amd import Morph
    for k, name in shapes.items():
        targets, normal_targets, weights = shape(scene.models[k], name, frame)
        scene.models[k].morph = Morph(targets, normal_targets)
        scene.models[k].morph_weights = weights


@functools.lru_cache(maxsize=None)
def _arrays(recipe, index, name, frame):
    """(V_m, N_m or None) of one model of a named recipe under one shape."""
    import scenes
    scene, _ = pose_ref.build(scenes.product_api(), recipe)
    return _arrays_of(scene.models[index], name, frame)


def _arrays_of(model, name, frame):
    targets, normal_targets, weights = shape(model, name, frame)
    verts = morphed_vertices(model.vertices, targets, weights)
    normals = None if normal_targets is None or model.normals is None else morphed_normals(model.normals, normal_targets, weights)
    return verts, normals


def twin(api, recipe, shapes, frame=0, rigs=None, skin_normals=False, rig_frame=0, poses=None, pose_normals=False):
    """The recipe built afresh with the arrays of every ``{model index: shape name}`` of *shapes* (a bare name: the
    recipe's own model) replaced by ``V_m`` (and ``N_m``).  *rigs* (``{model index: rig name}``, ``skin_ref.rig`` of the
    model as the recipe builds it), *poses* (``{model index: M}``) and *pose_normals* are set through ``Model.skin`` /
    ``bones`` / ``pose`` / ``pose_normals`` on the replaced arrays.  No model of the twin has a morph."""
    from py_numpy_renderer_amd import Skin
    scene, index = pose_ref.build(api, recipe)
    if not isinstance(shapes, dict):
        shapes = {index: shapes}
    for k, model in enumerate(scene.models):
        rig = None if not rigs or k not in rigs else skin_ref.rig(api, model, rigs[k], rig_frame)     # (from the rest shape)
        if shapes.get(k) is not None:
            verts, normals = _arrays(recipe, k, shapes[k], frame) if isinstance(recipe, str) else _arrays_of(model, shapes[k], frame)
            model.vertices = verts.copy()
            if normals is not None:
                model.normals = normals.copy()
            model._revision += 1
        if rig is not None:
            model.skin = Skin(rig[0], rig[1], normals=skin_normals)
            model.bones = rig[2]
        if poses and poses.get(k) is not None:
            model.pose = poses[k]
            model.pose_normals = pose_normals
    return scene


counted, assert_same = pose_ref.counted, pose_ref.assert_same
