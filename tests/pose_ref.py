"""What a posed model must be (the contract of ``Model.pose``), restated without the feature.

A model with ``pose = M`` renders as the same model with its ``vertices`` replaced by the float64 array
``_fp.matmul_chain(float64(vertices), float64(M))``.  ``twin`` builds that scene: the recipe afresh, the posed models'
vertices replaced, no pose set.  Posed scene and twin hold bit-identical inputs, so on one device their frames are equal
bit for bit, and the oracle's frame of the twin is the oracle's frame of the posed scene."""
import numpy as np

import scenes
from py_numpy_renderer_amd import _fp

# recipe -> (builder, index of the model the tests pose)
RECIPES = {
    "cube_outward": (lambda api: scenes.cube_outward(api, resolution=(120, 160)), 0),     # two models, the posed one float64 already
    "torus_spot": (lambda api: scenes.torus_spot(api, resolution=(180, 320)), 0),         # float32 torus + floor, compact edges before posing
    "diablo_floor": (lambda api: scenes.diablo_floor(api, resolution=(270, 480)), 0),     # tangent normal map
    "welded": (lambda api: scenes.welded(api, seed=0, resolution=(136, 152)), 0),         # edges with more than two faces
    "kat_house": (lambda api: scenes.kat_house(api, resolution=(150, 200)), 0),           # negative indices, several materials
}


def matrices(api):
    """The four poses of the tests: a rotation (float32, widened), a translation, a mirrored non-uniform scale (it
    flips the winding) and the product of the three, formed with ``matmul_chain``."""
    rotation = np.asarray(api.rotate_xyz((17, 31, -9))).astype(np.float64)
    translation = np.asarray(api.translation((0.13, -0.07, 0.21)), dtype=np.float64)
    mirror = np.diag([-0.7, 1.1, 0.9, 1.0])
    product = _fp.matmul_chain(_fp.matmul_chain(rotation, mirror), translation)
    return {"rotation": rotation, "translation": translation, "mirror": mirror, "product": product}


MATRIX_NAMES = ("rotation", "translation", "mirror", "product")


def turn(api, degrees):
    """The pose of frame i of a turning model: ``rotate_xyz((0, 0, degrees))`` widened to float64."""
    return np.asarray(api.rotate_xyz((0, 0, degrees))).astype(np.float64)


def posed_vertices(model, matrix):
    return _fp.matmul_chain(np.asarray(model.vertices).astype(np.float64), np.asarray(matrix, dtype=np.float64))


def build(api, recipe):
    """(scene, index of the model to pose) of a recipe name or a ``(builder, index)`` pair."""
    builder, index = RECIPES[recipe] if isinstance(recipe, str) else recipe
    return builder(api), index


def twin(api, recipe, poses):
    """The recipe built afresh with ``vertices = matmul_chain(float64(vertices), M)`` for every ``{model index: M}``
    of *poses* (a bare matrix: the recipe's own model).  No model of the twin has a pose."""
    scene, index = build(api, recipe)
    if not isinstance(poses, dict):
        poses = {index: poses}
    for k, matrix in poses.items():
        if matrix is not None:
            scene.models[k].vertices = posed_vertices(scene.models[k], matrix)
    return scene


STAT_KEYS = ("frag_tri", "frag_quad", "covered_px", "lit_px", "stencil_updates", "n_faces", "n_faces_setup", "n_quads",
             "n_quads_drawn", "tri_bin_entries", "quad_bin_entries")


def counted(backend, scene, lights=1, **kw):
    """One counted frame (``keep_buffers``) and everything a caller can read of it."""
    out = backend.render(scene, shadows=True, keep_float=True, **kw).copy()
    got = dict(out=out, z=backend.read_z().view(np.uint64).copy(), winner=backend.read_winner().copy(),
               frame=backend.read_frame_f32().view(np.uint32).copy(),
               stats={k: backend.last_stats[k] for k in STAT_KEYS})
    for k in range(lights):
        got[f"stencil{k}"] = backend.read_stencil(k).copy()
        got[f"silhouette{k}"] = sorted(map(tuple, backend.read_silhouette(k).tolist()))
    return got


def assert_same(got, want, label):
    assert set(got) == set(want), label
    for key, w in want.items():
        g = got[key]
        same = np.array_equal(g, w) if isinstance(w, np.ndarray) else g == w
        assert same, f"{label}: {key} differs" + ("" if isinstance(w, np.ndarray) else f" ({g} != {w})")
