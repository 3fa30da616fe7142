"""What a moved model with ``auto_normals = True`` must be (the contract of ``Model.auto_normals``), restated without
the feature.

Such a model renders as the same model with its ``vertices`` replaced by V, the float64 array it renders with (morph,
then skin, then pose: the arrays of morph_ref.py, skin_ref.py and pose_ref.py), and its ``normals`` by N: for normal q,
``L(q)`` is every face that has at least one corner whose normal column (wrapped) is q, once, in ascending order;
``acc`` is the cross product ``(V[b] - V[a]) x (V[c] - V[a])`` of the first face of the list (a, b, c the vertex columns
of corners 0, 1, 2), plus those of the others in order; ``N[q] = float32(acc / sqrt((acc0 * acc0 + acc1 * acc1) +
acc2 * acc2))``.  The authored ``float32(normals[q])`` stays where the list is empty, the length is 0, or the sum or the
length is not finite.  None of ``normal_targets``, ``Skin(normals=True)`` and the vector part of ``pose_normals`` is
applied first; object-space normal maps are re-baked under ``pose`` and ``pose_normals`` as ever.

``twin`` builds that scene: the recipe afresh, the arrays replaced, nothing that moves set.  ``chain`` is written here
with ``*``, ``-``, ``+``, ``/`` and ``math.sqrt`` on Python floats, so the twin does not depend on the code under test.
The generated meshes of this file (``fan``, ``tiny``) are written by this file."""
import functools
import math
import os

import numpy as np

import morph_ref
import pose_normals_ref
import pose_ref
import scenes
import skin_ref

MODES = ("morph", "skin", "pose", "all")        # a ``bands`` morph, a ``bend`` skin, a rotation, the three with a rotation and a translation
MIRROR = "mirror"                               # a further mode: the pose that flips the winding (pose_ref's ``product``), alone
FAN_FACES, FAN_NORMALS = 203, 130
FAN_UNNAMED, FAN_TWICE, FAN_CANCELLED = 127, 126, 128


# ---------------------------------------------------------------------------- generated meshes
def fan_obj():
    """A disc of 200 triangles round a raised hub, and three loose triangles beside it; 130 normals (slices of 64, 64
    and 2), authored off the geometry so that a rebuilt normal shows.

    normal 0        the hub: corner 0 of all 200 disc faces; faces 124..199 name it with all three corners (once each
                    in its list all the same)
    normals 1..125  the rim of faces 0..123: face i names 1 + i and 2 + i, so 2..124 are named by two faces -- 63 and
                    64 sit at the seam of the first two slices -- and 1 and 125 by one
    normal 126      two corners of face 200
    normal 127      no corner
    normal 128      faces 201 and 202: one triangle with both windings, a sum of exactly zero (the authored value stays)
    normal 129      the third corner of face 200: the last slice holds 128 and 129 only"""
    lines = ["v 0 0.05 0.18"]
    for i in range(201):
        a = 2.0 * math.pi * i / 200.0
        lines.append(f"v {0.62 * math.cos(a):.6f} {0.05 + 0.62 * math.sin(a):.6f} {0.03 * math.sin(5 * a):.6f}")
    lines += ["v 0.72 -0.2 0.1", "v 0.95 -0.15 0.05", "v 0.8 0.1 0.2",          # 203..205: face 200
              "v 0.75 0.35 0.1", "v 0.97 0.4 0.0", "v 0.85 0.62 0.15"]            # 206..208: faces 201, 202
    lines.append("vt 0 0")
    for q in range(FAN_NORMALS):
        a = 0.7 * q
        n = np.array([0.35 * math.cos(a), 0.35 * math.sin(a), 1.0])
        n /= np.linalg.norm(n)
        lines.append(f"vn {n[0]:.6f} {n[1]:.6f} {n[2]:.6f}")
    for i in range(200):
        rim = (2 + i, 3 + i) if i < 124 else (1, 1)
        lines.append(f"f 1/1/1 {2 + i}/1/{rim[0]} {3 + i}/1/{rim[1]}")
    lines.append("f 203/1/127 204/1/127 205/1/130")
    lines.append("f 206/1/129 207/1/129 208/1/129")
    lines.append("f 206/1/129 208/1/129 207/1/129")
    return scenes._write_if_changed(os.path.join(scenes.GENERATED, "auto_normals_fan.obj"), "\n".join(lines) + "\n")


def tiny_obj():
    """One triangle, one normal (authored off the triangle's own)."""
    text = "v -0.5 -0.3 0.1\nv 0.6 -0.2 0.0\nv 0.1 0.7 0.3\nvt 0 0\nvn 0.3 -0.2 0.932738\nf 1/1/1 2/1/1 3/1/1\n"
    return scenes._write_if_changed(os.path.join(scenes.GENERATED, "auto_normals_tiny.obj"), text)


def _generated(path_of):
    def builder(api, resolution=(120, 160)):
        cam, dbg = scenes._std_cameras(api)
        return scenes._scene(api, cam, dbg, scenes._std_light(api), resolution,
                             [api.Model.load_model(path_of()), scenes._floor(api, textured=False)])
    return builder


# recipe -> (builder, index of the model the tests move): the existing recipes that have normals, and the two of this file
RECIPES = {name: pose_ref.RECIPES[name] for name in ("cube_outward", "torus_spot", "diablo_floor", "kat_house")}
RECIPES["fan"] = (_generated(fan_obj), 0)
RECIPES["tiny"] = (_generated(tiny_obj), 0)
MESHES = tuple(RECIPES)


def cube_and_fan(api, resolution=(120, 160)):
    """Two float64 models with normals and different face lists -- moving either costs no commit, so the lists on the
    device live across frames -- and the floor."""
    cam, dbg = scenes._std_cameras(api)
    cube = api.Model.load_model(os.path.join(scenes.ASSETS, "cube", "cube.obj"))
    cube.normals = -cube.normals
    cube = cube @ api.scale(0.3) @ api.translation((-0.6, -0.3, 0.4))
    fan = api.Model.load_model(fan_obj()) @ api.scale(0.7)
    return scenes._scene(api, cam, dbg, scenes._std_light(api), resolution, [cube, fan, scenes._floor(api, textured=False)])


CUBE_AND_FAN = (cube_and_fan, 0)
OBJECT_MAP = pose_normals_ref.RECIPES["diablo_nm_object"]


def build(api, recipe):
    return pose_ref.build(api, RECIPES[recipe] if isinstance(recipe, str) else recipe)


# ---------------------------------------------------------------------------- the chain
def wrapped(model):
    """(F, 3) vertex and (F, 3) normal columns of ``_faces`` as lists, negative indices counted from the end."""
    n_verts, n_normals = len(model.vertices), len(model.normals)
    vertex, normal = [], []
    for face in np.asarray(model._faces).tolist():
        vertex.append([c[0] + n_verts if c[0] < 0 else c[0] for c in face])
        normal.append([c[2] + n_normals if c[2] < 0 else c[2] for c in face])
    return vertex, normal


def face_lists(model):
    """L(q) of every normal."""
    lists = [[] for _ in range(len(model.normals))]
    for f, named in enumerate(wrapped(model)[1]):
        for q in sorted(set(named)):
            lists[q].append(f)
    return lists


def chain(model, verts):
    """(N, the normals that kept their authored value) of *model* with the float64 vertices *verts*."""
    vertex, _ = wrapped(model)
    v = [[float(x) for x in row[:3]] for row in np.asarray(verts, dtype=np.float64)]
    normals = np.ascontiguousarray(model.normals, dtype=np.float32)
    out, kept = normals.copy(), []
    for q, faces in enumerate(face_lists(model)):
        acc = None
        for f in faces:
            a, b, c = (v[i] for i in vertex[f])
            e0x, e0y, e0z = b[0] - a[0], b[1] - a[1], b[2] - a[2]
            e1x, e1y, e1z = c[0] - a[0], c[1] - a[1], c[2] - a[2]
            cr = (e0y * e1z - e0z * e1y, e0z * e1x - e0x * e1z, e0x * e1y - e0y * e1x)
            acc = cr if acc is None else (acc[0] + cr[0], acc[1] + cr[1], acc[2] + cr[2])
        length = None
        if acc is not None and all(math.isfinite(x) for x in acc):
            square = (acc[0] * acc[0] + acc[1] * acc[1]) + acc[2] * acc[2]
            if math.isfinite(square) and square != 0.0:      # (sqrt is monotone: the length is finite and not 0 with its square)
                length = math.sqrt(square)
        if length is None or length == 0.0:
            kept.append(q)
            continue
        for j in range(3):
            out[q, j] = np.float32(acc[j] / length)
    return out, kept


# ---------------------------------------------------------------------------- moving a model, and its arrays
def motion(api, model, mode, frame=0):
    """What a mode sets on a model at rest: ``dict(morph=(targets, normal_targets, weights) or None, rig=(joints,
    weights, bones) or None, pose=M or None)``.  *frame* moves the morph's weights and the bones on."""
    matrices = pose_ref.matrices(api)
    matrices["moved"] = pose_ref._fp.matmul_chain(matrices["rotation"], matrices["translation"])
    return dict(morph=morph_ref.shape(model, "bands", frame) if mode in ("morph", "all") else None,
                rig=skin_ref.rig(api, model, "bend", frame) if mode in ("skin", "all") else None,
                pose={"pose": matrices["rotation"], "all": matrices["moved"], MIRROR: matrices["product"]}.get(mode))


def apply(api, model, mode, frame=0, flag=True, skin_normals=False, normal_targets=None, pose_normals=False):
    """The motion of *mode* through ``morph`` / ``morph_weights``, ``skin`` / ``bones`` and ``pose``, and the flag."""
    from py_numpy_renderer_amd import Morph, Skin
    m = motion(api, model, mode, frame)
    if m["morph"] is not None:
        model.morph = Morph(m["morph"][0], normal_targets)
        model.morph_weights = m["morph"][2]
    if m["rig"] is not None:
        model.skin = Skin(m["rig"][0], m["rig"][1], normals=skin_normals)
        model.bones = m["rig"][2]
    if m["pose"] is not None:
        model.pose = m["pose"]
        model.pose_normals = pose_normals
    model.auto_normals = flag


def rest(model):
    """Everything that moves the model taken away; the flag stays."""
    model.morph, model.skin, model.pose = None, None, None


def moved_vertices(api, model, mode, frame=0):
    """V of a model at rest under a mode, by the pure-Python chains of the three reference files."""
    m = motion(api, model, mode, frame)
    verts = np.asarray(model.vertices)
    if m["morph"] is not None:
        verts = morph_ref.morphed_vertices(verts, m["morph"][0], m["morph"][2])
    if m["rig"] is not None:
        verts = skin_ref.skinned_vertices(verts, *m["rig"])
    if m["pose"] is not None:
        verts = pose_ref._fp.matmul_chain(np.asarray(verts).astype(np.float64), m["pose"])
    return np.asarray(verts).astype(np.float64)


@functools.lru_cache(maxsize=None)
def arrays(recipe, mode, frame=0):
    """(V, N, kept) of the model a named recipe moves, under one mode."""
    api = scenes.product_api()
    scene, index = build(api, recipe)
    model = scene.models[index]
    verts = moved_vertices(api, model, mode, frame)
    normals, kept = chain(model, verts)
    return verts, normals, tuple(kept)


def replace(api, model, mode, frame=0, pose_normals=False, cached=None):
    """The two replacements on a twin's model; with *pose_normals* its object-space maps re-baked with G."""
    if cached is not None:
        verts, normals, _ = cached
    else:
        verts = moved_vertices(api, model, mode, frame)
        normals, _ = chain(model, verts)
    matrix = motion(api, model, mode, frame)["pose"]
    model.vertices, model.normals = verts.copy(), normals.copy()
    if pose_normals and matrix is not None:
        g = pose_normals_ref.normal_matrix(matrix)
        for mat in pose_normals_ref.object_space_materials(model):
            mat.norm = np.array(pose_normals_ref.chain_f32(mat.norm, g), dtype=np.dtype(np.float32, metadata={"tangent": False}))
    model._revision += 1


def twin(api, recipe, modes, frame=0, pose_normals=False):
    """The recipe built afresh with ``vertices`` and ``normals`` of every ``{model index: mode}`` of *modes* (a bare
    mode: the recipe's own model) replaced by V and N.  No model of the twin has a morph, a skin, a pose or the flag."""
    scene, index = build(api, recipe)
    if not isinstance(modes, dict):
        modes = {index: modes}
    for k, mode in modes.items():
        cached = arrays(recipe, mode, frame) if isinstance(recipe, str) and k == index else None
        replace(api, scene.models[k], mode, frame, pose_normals, cached)
    return scene


counted, assert_same = pose_ref.counted, pose_ref.assert_same
