"""GPU: ``Model.auto_normals`` -- vertex normals rebuilt from the deformed mesh in the pose pass (host_autonormals.h,
host_pose.h; k_auto_normals in kernels_pose.h).

The yardstick is the twin (auto_normals_ref.py): the recipe built afresh with the moved model's ``vertices`` and
``normals`` replaced by the arrays the contract names, formed in pure Python.  Flagged scene and twin hold bit-identical
inputs, so everything a caller can read of their frames on one device is compared for equality; the oracle's frame of
the twin is held to the project's standing bars (z / winner / stencil / silhouette / counts bit-exact, float frame 2e-6,
uint8 +-1)."""
import functools

import numpy as np
import pytest

import auto_normals_ref as ref
import morph_ref
import pose_normals_ref
import pose_ref
import scenes
import skin_ref
from auto_normals_ref import assert_same, counted
from multilight_ref import extra_lights
from py_numpy_renderer_amd import Skin

pytestmark = pytest.mark.gpu

CASES = [(mesh, mode) for mesh in ref.MESHES for mode in ref.MODES]


@functools.lru_cache(maxsize=None)
def _flagged_and_twin(mesh, mode):
    """One mesh under one mode: the moved frame with the flag off, the frame with it on, the twin's frame (each
    ``counted``), the twin, and the counters after the flagged frame."""
    api = scenes.product_api()
    other = ref.twin(api, mesh, mode)                  # (first: a new Material anywhere makes every scene upload its models again)
    want = counted(other._backend(), other)
    other.close()
    scene, index = ref.build(api, mesh)
    backend, model = scene._backend(), scene.models[index]
    ref.apply(api, model, mode, flag=False)
    off = counted(backend, scene)
    model.auto_normals = True
    on = counted(backend, scene)
    counters, times = backend.auto_normals_counters(), backend.auto_normals_times()
    scene.close()
    return off, on, want, other, counters, times


# ---------------------------------------------------------------------------- 1. flagged equals twin, exactly
@pytest.mark.parametrize("mesh, mode", CASES)
def test_flagged_equals_twin(mesh, mode):
    """Frame bytes, z bits, winner, stencil, silhouette set, float frame and every counter of ``mr_stats`` are the
    twin's; the frame is not the one of the same moved scene with the flag off, though its geometry (z, stencil) is:
    normals move no vertex.  The counters: one model, every normal written, padded lists, and as many normals kept as the
    CPU chain keeps."""
    off, on, want, other, counters, times = _flagged_and_twin(mesh, mode)
    assert_same(on, want, f"{mesh} under {mode}")
    assert not np.array_equal(on["frame"], off["frame"]), f"{mesh} under {mode}: the flag changed nothing"
    assert np.array_equal(on["z"], off["z"]) and np.array_equal(on["stencil0"], off["stencil0"])
    assert np.array_equal(on["winner"], off["winner"]) and on["silhouette0"] == off["silhouette0"]
    n = len(other.models[ref.RECIPES[mesh][1]].normals)
    assert counters[:2] == (1, n), counters
    assert counters[2] % 64 == 0 and counters[2] >= 64 * -(-n // 64), counters
    assert counters[3] == len(ref.arrays(mesh, mode)[2]), counters
    assert times["auto_normals"] > 0


def test_a_mirroring_pose_flips_the_normals_with_the_faces(oracle_mod):
    """The pose that flips the winding: the twin's normals are those of the flipped faces, and so are the frame's."""
    off, on, want, other, counters, _ = _flagged_and_twin("torus_spot", ref.MIRROR)
    assert_same(on, want, "mirrored")
    assert not np.array_equal(on["frame"], off["frame"]) and np.array_equal(on["z"], off["z"])
    assert counters[:2] == (1, len(other.models[0].normals)) and counters[3] == 0
    _hold_to_the_oracle(oracle_mod, on, other, "mirrored")


# ---------------------------------------------------------------------------- 2. flagged equals the oracle of the twin
@pytest.mark.parametrize("mesh, mode", CASES)
def test_flagged_equals_the_oracle_of_the_twin(oracle_mod, mesh, mode):
    _, on, _, other, _, _ = _flagged_and_twin(mesh, mode)
    _hold_to_the_oracle(oracle_mod, on, other, f"{mesh} under {mode}")


def _hold_to_the_oracle(oracle_mod, got, other, label):
    want = oracle_mod.render(other, shadows=True)
    assert np.array_equal(got["z"], want.z.view(np.uint64)), f"{label}: z"
    assert np.array_equal(got["winner"], want.winner), f"{label}: winner"
    assert np.array_equal(got["stencil0"], want.stencil), f"{label}: stencil"
    assert set(got["silhouette0"]) == set(map(tuple, want.silhouette.tolist())), f"{label}: silhouette"
    assert got["stats"]["n_quads"] == want.stats["n_quads"], f"{label}: silhouette edges"
    assert got["stats"]["frag_tri"] == want.stats["frag_tri_pass1"], f"{label}: triangle fragments"
    assert got["stats"]["frag_quad"] == want.stats["frag_quad"], f"{label}: quad fragments"
    err = np.abs(got["frame"].view(np.float32).astype(np.float64) - want.frame.astype(np.float64)).max()
    print(f"{label}: float frame differs from the oracle's by at most {err:.3g}")
    assert err <= 2e-6, f"{label}: float frame {err}"
    assert np.abs(got["out"].astype(np.int16) - want.out.astype(np.int16)).max() <= 1, f"{label}: uint8 frame"


# ---------------------------------------------------------------------------- 3. the flag across frames
def test_on_off_on_brings_the_other_paths_back_and_returns(api):
    """A torus with ``normal_targets``, ``Skin(normals=True)`` and ``pose_normals`` all set: the flag on is the twin; off
    is the frame of a scene that never had the flag (k_morph_normals, k_skin_normals and the normal matrix are back);
    on again is the first flagged frame bit for bit.  Toggling rewrites normals only: no vertex is written."""
    def moved(flag):
        scene, index = ref.build(api, "torus_spot")
        model = scene.models[index]
        ref.apply(api, model, "all", flag=flag, skin_normals=True, pose_normals=True, normal_targets=morph_ref.shape(model, "normals")[1])
        return scene, model
    never, _ = moved(False)
    without = counted(never._backend(), never)
    never.close()
    other = ref.twin(api, "torus_spot", "all")
    want = counted(other._backend(), other)
    other.close()
    scene, model = moved(True)
    backend = scene._backend()
    first = counted(backend, scene)
    assert_same(first, want, "flag on")
    assert not np.array_equal(first["frame"], without["frame"])
    passes = backend.pose_counters()[1]
    model.auto_normals = False
    assert_same(counted(backend, scene), without, "flag off")
    assert backend.auto_normals_counters()[:2] == (0, 0)
    model.auto_normals = True
    assert_same(counted(backend, scene), first, "flag on again")
    assert backend.auto_normals_counters()[:2] == (1, len(model.normals))
    assert backend.pose_counters()[1:] == (passes + 2, 1, 0)        # two passes, and neither wrote a vertex
    scene.close()


@pytest.mark.parametrize("mesh, mode", [("fan", "all"), ("diablo_floor", "skin")])
def test_back_to_rest_renders_the_authored_normals(api, mesh, mode):
    scene, index = ref.build(api, mesh)
    backend, model = scene._backend(), scene.models[index]
    model.auto_normals = True                                      # at rest: no call, no pass
    first = counted(backend, scene)
    assert backend.pose_counters()[1] == 0 and backend.auto_normals_counters() == (0, 0, 0, 0)
    ref.apply(api, model, mode)
    moved = counted(backend, scene)
    assert_same(moved, _flagged_and_twin(mesh, mode)[2], "moved")
    ref.rest(model)
    assert_same(counted(backend, scene), first, "at rest again")
    assert backend.auto_normals_counters()[:2] == (0, 0)
    ref.apply(api, model, mode)
    assert_same(counted(backend, scene), moved, "moved again")
    scene.close()


# ---------------------------------------------------------------------------- 4. several models in one pass
def test_two_flagged_models_and_a_skinned_one_whose_normals_follow(api):
    """diablo (morphed, flagged), the cube (posed, flagged; 24 normals: one slice, one workgroup) and the floor (skinned
    with ``normals=True``, not flagged) in one pass: the rows', the slices' and the lists' offsets differ from 0 for the
    cube, and k_skin_normals writes the floor's normals beside k_auto_normals."""
    recipe = pose_normals_ref.SMALL_AND_LARGE                      # [diablo, cube, floor]
    modes = {0: "morph", 1: "pose"}

    def skin_the_floor(scene):
        rig = skin_ref.rig(api, scene.models[2], "bend")
        scene.models[2].skin = Skin(rig[0], rig[1], normals=True)
        scene.models[2].bones = rig[2]
    other = ref.twin(api, recipe, modes)
    skin_the_floor(other)
    want = counted(other._backend(), other)
    scene, _ = ref.build(api, recipe)
    backend = scene._backend()
    plain = counted(backend, scene)
    for k, mode in modes.items():
        ref.apply(api, scene.models[k], mode)
    skin_the_floor(scene)
    assert_same(counted(backend, scene), want, "three models")
    n = [len(m.normals) for m in scene.models]
    counters = backend.auto_normals_counters()
    assert counters[:2] == (2, n[0] + n[1]) and counters[2] % 64 == 0, counters
    assert counters[3] == len(ref.arrays("diablo_floor", "morph")[2]), counters      # (the same diablo; every normal of the cube is rebuilt)
    assert backend.skin_counters()[-1] == n[2]
    # the cube alone stops: its authored normals are back, diablo's stay rebuilt
    scene.models[1].auto_normals = False
    third = ref.twin(api, recipe, {0: "morph"})
    third.models[1].pose = ref.motion(api, third.models[1], "pose")["pose"]
    skin_the_floor(third)
    assert_same(counted(backend, scene), counted(third._backend(), third), "the cube unflagged")
    assert backend.auto_normals_counters()[:2] == (1, n[0])
    for model in scene.models:
        ref.rest(model)
    assert_same(counted(backend, scene), plain, "all at rest")
    scene.close(), other.close(), third.close()


def test_a_model_flagged_again_after_another_was_first_flagged(api):
    """Two float64 models (no commit in between, so nothing rebuilds the device lists by the way): the cube flagged and
    moved; the cube at rest and the fan newly flagged and moved -- the lists are uploaded again, with the fan's; the cube
    moved again: it walks its own lists, wherever they are now, and the frame is the twin's."""
    recipe = ref.CUBE_AND_FAN
    wants = []
    for modes in ({0: "pose"}, {1: "skin"}, {0: "pose", 1: "skin"}):
        other = ref.twin(api, recipe, modes)
        wants.append(counted(other._backend(), other))
        other.close()
    scene, _ = ref.build(api, recipe)
    backend, cube, fan = scene._backend(), scene.models[0], scene.models[1]
    assert np.asarray(cube.vertices).dtype == np.float64 and np.asarray(fan.vertices).dtype == np.float64
    ref.apply(api, cube, "pose")
    assert_same(counted(backend, scene), wants[0], "the cube")
    entries = backend.auto_normals_counters()[2]
    ref.rest(cube)
    ref.apply(api, fan, "skin")
    assert_same(counted(backend, scene), wants[1], "the fan, the cube at rest")
    assert backend.auto_normals_counters()[:2] == (1, len(fan.normals)) and backend.auto_normals_counters()[2] > entries
    ref.apply(api, cube, "pose")
    assert_same(counted(backend, scene), wants[2], "the cube again")
    assert backend.auto_normals_counters()[:2] == (2, len(cube.normals) + len(fan.normals))
    assert backend.auto_normals_counters()[3] == 2                 # (the fan's unnamed and cancelled normals)
    assert backend.pose_counters()[0] == 1                         # one commit: the lists were never rebuilt by the way
    ref.rest(fan)
    assert_same(counted(backend, scene), wants[0], "the fan at rest")
    ref.apply(api, fan, "skin")
    assert_same(counted(backend, scene), wants[2], "the fan again")
    assert backend.pose_counters()[0] == 1
    scene.close()


# ---------------------------------------------------------------------------- 5. a sequence
def test_eight_frames_of_new_weights(api):
    """Every frame its twin's; one pass per frame that rebuilds the torus' normals and no others; inputs left alone launch
    nothing."""
    want = {}
    for i in range(1, 9):
        other = ref.twin(api, "torus_spot", "morph", frame=i)
        want[i] = counted(other._backend(), other)
        other.close()
    scene, index = ref.build(api, "torus_spot")
    backend, torus = scene._backend(), scene.models[index]
    backend.render(scene, shadows=True)
    for i in range(1, 9):
        if i == 1:
            ref.apply(api, torus, "morph", frame=1)
        else:
            torus.morph_weights = morph_ref.shape(torus, "bands", frame=i)[2]
        assert_same(counted(backend, scene), want[i], f"frame {i}")
        assert backend.pose_counters()[1] == i and backend.auto_normals_counters()[:2] == (1, len(torus.normals))
    commits, passes = backend.pose_counters()[:2]
    torus.morph_weights = np.array(torus.morph_weights)            # the same weights in a new array, the same flag
    torus.auto_normals = 1
    assert_same(counted(backend, scene), want[8], "inputs unchanged")
    assert backend.pose_counters()[:2] == (commits, passes)
    scene.close()


# ---------------------------------------------------------------------------- 6. object-space maps
def test_an_object_space_map_under_pose_normals_is_still_rebaked(api):
    """diablo_nm_object: the flag takes the vertex normals from ``pose_normals``, not the texels of the map."""
    recipe = ref.OBJECT_MAP
    other = ref.twin(api, recipe, "pose", pose_normals=True)
    want = counted(other._backend(), other)
    scene, index = pose_ref.build(api, recipe)
    backend, model = scene._backend(), scene.models[index]
    first = counted(backend, scene)
    ref.apply(api, model, "pose", pose_normals=True, flag=False)
    followed = counted(backend, scene)
    model.auto_normals = True
    assert_same(counted(backend, scene), want, "flag on under pose_normals")
    times = backend.pose_normals_times()
    assert times["pose_texels"] > 0 and times["pose_normals"] == 0     # the texels re-baked, the normals left out of k_pose_normals' rows
    model.pose_normals = False
    unbaked = ref.twin(api, recipe, "pose")
    assert_same(counted(backend, scene), counted(unbaked._backend(), unbaked), "pose_normals off: the map as registered")
    model.pose_normals = True
    model.auto_normals = False
    assert_same(counted(backend, scene), followed, "flag off: the normal matrix again")
    ref.rest(model)
    assert_same(counted(backend, scene), first, "at rest")
    scene.close(), other.close(), unbaked.close()


# ---------------------------------------------------------------------------- 7. the other frame kinds
def _pair(api, mesh, mode="morph", prepare=lambda scene: None):
    other = ref.twin(api, mesh, mode)
    prepare(other)
    scene, index = ref.build(api, mesh)
    prepare(scene)
    scene._backend().render(scene, shadows=True)                   # (at rest first: the motion arrives between frames)
    ref.apply(api, scene.models[index], mode)
    return scene, other


def test_supersampled(api):
    def prepare(scene):
        scene.supersample = 2
    scene, other = _pair(api, "torus_spot", prepare=prepare)
    assert_same(counted(scene._backend(), scene), counted(other._backend(), other), "supersample = 2")
    assert np.array_equal(scene.render(), other.render())
    scene.close(), other.close()


def test_three_lights(api):
    def prepare(scene):
        for light in extra_lights(api)[:2]:
            scene.add_light(light)
    scene, other = _pair(api, "fan", "all", prepare=prepare)
    assert_same(counted(scene._backend(), scene, lights=3), counted(other._backend(), other, lights=3), "three lights")
    scene.close(), other.close()


def test_overlay(api):
    scene, other = _pair(api, "cube_outward", "skin")
    assert_same(counted(scene._backend(), scene, overlay=True), counted(other._backend(), other, overlay=True), "overlay")
    scene.draw_debug_frustum = other.draw_debug_frustum = True
    assert np.array_equal(scene.render(), other.render())
    scene.close(), other.close()


def test_row_band(api):
    scene, other = _pair(api, "torus_spot", "all")
    h = scene.resolution[0]
    whole = other.render().copy()
    for band in ((0, 64), (48, 112), (112, h)):
        # (without the fragment counters: a counted frame never culls clusters, a band without them does by default)
        got = scene._backend().render(scene, shadows=True, counters=False, keep_buffers=True, row_band=band).copy()
        want = other._backend().render(other, shadows=True, counters=False, keep_buffers=True, row_band=band).copy()
        assert np.array_equal(got, want) and np.array_equal(got, whole[band[0]:band[1]]), band
    scene.close(), other.close()


def test_render_async_with_new_weights_each_frame(api):
    """Eight frames two deep, new weights in front of each: the pass drains the frames in flight, and every frame is its
    twin's synchronous one."""
    scene, index = ref.build(api, "torus_spot")
    torus = scene.models[index]
    scene.render()
    queue, got = [], []
    for i in range(1, 9):
        if i == 1:
            ref.apply(api, torus, "morph", frame=1)
        else:
            torus.morph_weights = morph_ref.shape(torus, "bands", frame=i)[2]
        queue.append(scene.render_async())
        if len(queue) >= 2:
            got.append(queue.pop(0).result().copy())
    got += [p.result().copy() for p in queue]
    assert scene._backend().pose_counters()[1] == 8
    scene.close()
    for i in range(1, 9):
        other = ref.twin(api, "torus_spot", "morph", frame=i)
        assert np.array_equal(got[i - 1], other.render()), f"frame {i}"
        other.close()


def test_a_float32_model_flagged_and_unflagged_again(api):
    """torus_spot's torus is float32: with the identity pose its faces lose the float32 bit (one ordinary commit, which
    drops the face lists: the pass builds them again) and its normals are rebuilt from the mesh at rest; the flag off
    leaves the posed torus with its authored normals, and ``pose = None`` gives the first frame back bit for bit."""
    other, index = ref.build(api, "torus_spot")            # (the twins first: a new Material anywhere makes every scene upload its models again)
    verts = pose_ref.posed_vertices(other.models[index], np.eye(4))
    other.models[index].normals = ref.chain(other.models[index], verts)[0]
    other.models[index].vertices = verts
    unflagged = pose_ref.twin(api, "torus_spot", np.eye(4))
    want, want_unflagged = counted(other._backend(), other), counted(unflagged._backend(), unflagged)
    other.close(), unflagged.close()
    scene, index = ref.build(api, "torus_spot")
    backend, torus = scene._backend(), scene.models[index]
    assert np.asarray(torus.vertices).dtype == np.float32
    first = counted(backend, scene)
    assert backend.pose_counters()[:2] == (1, 0)
    torus.auto_normals, torus.pose = True, np.eye(4)
    rebuilt = counted(backend, scene)
    assert_same(rebuilt, want, "rebuilt at rest")
    assert backend.pose_counters()[:2] == (2, 1) and backend.auto_normals_counters()[:2] == (1, len(torus.normals))
    assert not np.array_equal(rebuilt["frame"], first["frame"])
    torus.auto_normals = False
    assert_same(counted(backend, scene), want_unflagged, "unflagged")
    assert backend.pose_counters()[:2] == (2, 2)
    torus.pose = None
    assert_same(counted(backend, scene), first, "at rest again")
    assert backend.pose_counters()[0] == 3
    scene.close()
