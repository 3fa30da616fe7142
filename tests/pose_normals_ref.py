"""What a posed model with ``pose_normals = True`` must be, restated without the feature.

Such a model renders as the twin of ``pose_ref.twin`` (``vertices = matmul_chain(float64(vertices), M)``) with two
further replacements, both made with ``G``, the inverse transpose of ``M[:3, :3]`` (cofactors over determinant):
``normals = float32(matmul_chain(float64(float32(normals)), G))``, and every object-space normal map of the model's
materials registered again as ``float32(matmul_chain(float64(texels), G))``.  Posed scene and twin hold bit-identical
inputs, so on one device their frames are equal bit for bit, and the oracle's frame of the twin is the oracle's frame
of the posed scene."""
import os

import numpy as np

import pose_ref
import scenes
from py_numpy_renderer_amd import _fp

# recipe -> (builder, index of the model the tests pose)
RECIPES = {
    "diablo_floor": (lambda api: scenes.diablo_floor(api, resolution=(270, 480)), 0),     # vertex normals, a tangent map, vn count != v count
    "diablo_nm_object": (lambda api: scenes.diablo_nm_object(api, resolution=(240, 320)), 0),      # object-space map
    "quad_rect_object_nm": (lambda api: scenes.quad_rect_object_nm(api, resolution=(150, 200)), 0),  # non-square object-space map
    "torus_spot": (lambda api: scenes.torus_spot(api, resolution=(180, 320)), 0),         # float32 model: the FF_VERTS_F32 flip
    "cube_outward": (lambda api: scenes.cube_outward(api, resolution=(120, 160)), 0),     # the second model un-posed
    "tetra_bare": (lambda api: scenes.tetra_bare(api, resolution=(120, 160)), 0),         # no normals at all
}
MATRIX_NAMES = ("rotation", "mirror", "product")       # (the translation: G = I, see the CPU tests)


def normal_matrix(matrix):
    """G of a pose in Python floats: ``C[i][j] / det`` with ``C[i][j] = a[i+1][j+1] * a[i+2][j+2] - a[i+1][j+2] * a[i+2][j+1]``
    (indices mod 3) and ``det = (a[0][0] * C[0][0] + a[0][1] * C[0][1]) + a[0][2] * C[0][2]``."""
    a = [[float(matrix[i][j]) for j in range(3)] for i in range(3)]
    g = np.empty((3, 3), dtype=np.float64)
    cof = lambda i, j: (a[(i + 1) % 3][(j + 1) % 3] * a[(i + 2) % 3][(j + 2) % 3]
                        - a[(i + 1) % 3][(j + 2) % 3] * a[(i + 2) % 3][(j + 1) % 3])
    det = (a[0][0] * cof(0, 0) + a[0][1] * cof(0, 1)) + a[0][2] * cof(0, 2)
    for i in range(3):
        for j in range(3):
            g[i, j] = cof(i, j) / det
    return g


def chain_f32(vectors, g):
    """``float32(matmul_chain(float64(float32(vectors)), g))`` of an (..., 3) array."""
    v = np.ascontiguousarray(vectors, dtype=np.float32)
    return _fp.matmul_chain(v.reshape(-1, 3).astype(np.float64), g).astype(np.float32).reshape(v.shape)


def object_space_materials(model):
    """The distinct materials of a model's groups that hold an object-space normal map."""
    found = []
    for k in range(len(model.material_group)):
        mat = model.face_material(k)
        if "norm" in mat.__dict__ and not mat.is_tangent_space("norm") and not any(mat is m for m in found):
            found.append(mat)
    return found


def follow(model, matrix):
    """The two replacements on a twin's model whose vertices were posed with *matrix*."""
    g = normal_matrix(matrix)
    if model.normals is not None:
        model.normals = chain_f32(model.normals, g)
    for mat in object_space_materials(model):
        mat.norm = np.array(chain_f32(mat.norm, g), dtype=np.dtype(np.float32, metadata={"tangent": False}))
    model._revision += 1


def twin(api, recipe, poses, normals=None):
    """``pose_ref.twin`` of a recipe name or ``(builder, index)`` pair for every ``{model index: M}`` of *poses* (a
    bare matrix: the recipe's own model), then ``follow`` for the models listed in *normals* (default: every posed
    model).  No model of the twin has a pose."""
    recipe = RECIPES[recipe] if isinstance(recipe, str) else recipe
    if not isinstance(poses, dict):
        poses = {recipe[1]: poses}
    scene = pose_ref.twin(api, recipe, poses)
    for k, matrix in poses.items():
        if matrix is not None and (normals is None or k in normals):
            follow(scene.models[k], matrix)
    return scene


def build(api, recipe):
    return pose_ref.build(api, RECIPES[recipe] if isinstance(recipe, str) else recipe)


def pose(model, matrix, normals=True):
    """``pose`` and ``pose_normals`` of a model in the order that never holds a pair the caller did not mean."""
    if matrix is None:
        model.pose = None
    model.pose_normals = normals
    model.pose = matrix


# ---------------------------------------------------------------------------- recipes of this file
def two_quads_one_map(api, resolution=(150, 200)):
    """Two quads (neg_uv_obj, the second moved up and back) whose materials hold ONE object-space normal map array, and
    a small textured floor."""
    cam, dbg = scenes._std_cameras(api, backface_culling=False)
    light = scenes._std_light(api)
    first = api.Model.load_model(scenes.neg_uv_obj())
    first.textures.register("normals", scenes.hash_texture(80, 24, 6, normal_map=True), tangent=False)
    first.textures.register("diffuse", scenes.hash_texture(24, 80, 5), normalize=False)
    second = api.Model.load_model(scenes.neg_uv_obj()) @ api.scale(0.5) @ api.translation((0.3, 0.7, -0.6))
    second.materials["default"].__dict__["norm"] = first.materials["default"].norm      # the same array, not a copy
    second._revision += 1
    return scenes._scene(api, cam, dbg, light, resolution, [first, second, scenes._floor(api)])


def small_and_large(api, resolution=(270, 480)):
    """diablo (a normal count that is no multiple of 256) beside the cube (24 normals, fewer than one workgroup) and the
    floor: two posed models in one pass."""
    cam, dbg = scenes._std_cameras(api)
    cube = api.Model.load_model(os.path.join(scenes.ASSETS, "cube", "cube.obj"))
    cube.normals = -cube.normals
    cube = cube @ api.scale(0.3) @ api.translation((0.9, -0.4, 0.5))
    return scenes._scene(api, cam, dbg, scenes._std_light(api), resolution, [scenes._diablo(api), cube, scenes._floor(api)])


TWO_QUADS = (two_quads_one_map, 0)
SMALL_AND_LARGE = (small_and_large, 0)
