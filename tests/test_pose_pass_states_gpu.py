"""GPU: one scene walked through the states of the pose pass (host_pose.h), across the features.

Every other file stays inside one feature and what it sits on; the steps here are the transitions where a shared dirty
bit or a shared restore can go wrong: morph weights, then bones on a skin whose normals follow, then a pose with pose
normals, ``auto_normals`` on and off, and the four taken away again in another order -- while a second model has only its
normal matrix change and a third never moves.  After every step the frame is, bit for bit, the frame of a fresh scene
built directly in that state (the twins of morph_ref.py and auto_normals_ref.py), the counters follow the rules the five
files assert piecewise, and every ``*_times()`` returns its fixed number of values with exact 0.0 for a kernel the step
did not launch.

The scenes are the small ones those files build, every model's vertices widened to float64 first (the values stay), so
that a model that starts or stops moving costs no commit and the device's tables live through the whole walk."""
import collections

import numpy as np
import pytest

import auto_normals_ref as ref
import morph_ref
import pose_normals_ref
import pose_ref
from auto_normals_ref import assert_same, counted
from py_numpy_renderer_amd import Morph, Skin

pytestmark = pytest.mark.gpu


def _widened(builder):
    def build(api):
        scene = builder(api)
        for model in scene.models:
            model.vertices = np.asarray(model.vertices).astype(np.float64)
            model._revision += 1
        return scene
    return build


# name -> ((builder, the model that walks), the model whose normal matrix alone changes or None, an object-space map?)
LAYOUTS = {
    "cube_and_fan": ((_widened(ref.cube_and_fan), 1), 0, False),                    # the fan walks, the cube turns its normals, the floor stays
    "kat_house": ((_widened(pose_ref.RECIPES["kat_house"][0]), 0), 1, False),       # negative indices, several materials; the porch, the floor
    "diablo_nm_object": ((_widened(ref.OBJECT_MAP[0]), 0), None, True),             # one model, its map re-baked and given back
}

# One step (``_do`` holds its setters): whether it is the second model's, the state a fresh scene is built in (what
# moves the walker, ``auto``, ``g``: its pose normals, ``sg``: the second model's), whether vertices are written,
# which of (k_morph_vertices, k_morph_normals) and (k_skin_vertices, k_skin_normals) the pass launches (None: no such pass
# yet), whether k_auto_normals runs, the models with a row of k_pose_normals (None: that part launches nothing, the values
# are an earlier pass's) and whether the walker's object-space maps are re-baked.
Step = collections.namedtuple("Step", "label needs_second state geometry morph skin auto rows texels")
STEPS = (
    Step("rest", False, "", True, None, None, None, None, False),
    Step("morph weights", False, "morph sg", True, (1, 1), None, None, "s", False),
    Step("bones", False, "morph skin sg", True, (1, 1), (1, 1), None, "s", False),
    Step("second: normal matrix off", True, "morph skin", False, (0, 1), (0, 1), None, None, False),
    Step("pose with pose normals", False, "morph skin pose g", True, (1, 1), (1, 1), None, None, True),
    Step("auto_normals on", False, "morph skin pose g auto", False, (0, 0), (0, 0), True, None, True),
    Step("second: normal matrix on", True, "morph skin pose g auto sg", False, (0, 0), (0, 0), True, "s", True),
    Step("auto_normals off", False, "morph skin pose g sg", False, (0, 1), (0, 1), False, "s", True),
    Step("weights removed", False, "skin pose g sg", True, (0, 0), (1, 1), False, "s", True),
    Step("bones removed", False, "pose g sg", True, (0, 0), (0, 0), False, "ws", True),
    Step("pose normals removed", False, "pose sg", False, (0, 0), (0, 0), False, "s", False),
    Step("pose removed", False, "sg", True, (0, 0), (0, 0), False, None, False),
)


def _states(second):
    """The steps of a layout with the state each leaves: without a second model its steps and its ``sg`` fall away."""
    steps = [(step, set(step.state.split())) for step in STEPS if second is not None or not step.needs_second]
    return steps if second is not None else [(step, state - {"sg"}) for step, state in steps]


def _motion(api, recipe):
    """What the walker is given: the ``all`` mode of auto_normals_ref (``bands`` morph, ``bend`` rig, rotation and
    translation) with the normal targets of morph_ref's ``normals`` shape; and the second model's pose."""
    scene, index = ref.build(api, recipe)
    walker = scene.models[index]
    m = ref.motion(api, walker, "all")
    m["normal_targets"] = morph_ref.shape(walker, "normals")[1]
    m["second"] = pose_ref.matrices(api)["rotation"]
    m["verts"] = [len(model.vertices) for model in scene.models]
    m["normals"] = len(walker.normals)
    scene.close()
    return m


def _fresh(api, recipe, second, m, state):
    """A scene built directly in a state: the recipe afresh, the walker's arrays replaced by the twins' helpers."""
    index = recipe[1]
    if "auto" in state:
        assert {"morph", "skin", "pose"} <= state
        scene = ref.twin(api, recipe, {index: "all"}, pose_normals="g" in state)
    else:
        scene = morph_ref.twin(api, recipe, {index: "normals"} if "morph" in state else {},
                               rigs={index: "bend"} if "skin" in state else None, skin_normals=True,
                               poses={index: m["pose"]} if "pose" in state else None, pose_normals="g" in state)
    if second is not None:
        pose_normals_ref.pose(scene.models[second], m["second"], "sg" in state)
    return scene


def _do(step, walker, other, m, again=False):
    """The setters of a step; with *again* one of them repeated with the value it holds (in a new array)."""
    label = step.label
    if label == "morph weights":
        if not again:
            walker.morph = Morph(m["morph"][0], m["normal_targets"])
            if other is not None:
                other.pose_normals = True
        walker.morph_weights = np.array(m["morph"][2])
    elif label == "bones":
        if not again:
            walker.skin = Skin(m["rig"][0], m["rig"][1], normals=True)
        walker.bones = np.array(m["rig"][2])
    elif label == "second: normal matrix off":
        other.pose_normals = False
    elif label == "pose with pose normals":
        pose_normals_ref.pose(walker, np.array(m["pose"]), True)
    elif label == "auto_normals on":
        walker.auto_normals = True
    elif label == "second: normal matrix on":
        other.pose_normals = True
    elif label == "auto_normals off":
        walker.auto_normals = False
    elif label == "weights removed":
        walker.morph_weights = None
    elif label == "bones removed":
        walker.bones = None
    elif label == "pose normals removed":
        walker.pose_normals = False
    elif label == "pose removed":
        walker.pose = None


def _times(read):
    """The values of one ``*_times()``, or None while the library has seen no such pass."""
    try:
        return read()
    except RuntimeError:
        return None


def _check_times(backend, step, has_second, has_map, label):
    """Fixed counts, and exact 0.0 for what the step's pass did not launch."""
    for name, read, want in (("morph", backend.morph_times, step.morph), ("skin", backend.skin_times, step.skin)):
        got = _times(read)
        print(f"{label}: {name}_times {got}")
        if want is None:
            assert got is None, f"{label}: {name}_times before the first such pass"
            continue
        assert len(got) == 2, label
        for ran, value in zip(want, got.values()):
            assert (value > 0) if ran else (value == 0.0), f"{label}: {name}_times {got}, launched {want}"
    got = _times(backend.auto_normals_times)
    print(f"{label}: auto_normals_times {got}")
    if step.auto is None:
        assert got is None, f"{label}: auto_normals_times before the first such pass"
    else:
        assert len(got) == 1 and ((got["auto_normals"] > 0) if step.auto else (got["auto_normals"] == 0.0)), f"{label}: {got}"
    rows = bool(step.rows) and (has_second or "w" in step.rows)
    texels = step.texels and has_map
    got = _times(backend.pose_normals_times)
    print(f"{label}: pose_normals_times {got}")
    if got is not None:
        assert len(got) == 2, label
    if rows or texels:                                             # (else: the values of an earlier pass, or none yet)
        assert (got["pose_normals"] > 0) if rows else (got["pose_normals"] == 0.0), f"{label}: {got}"
        assert (got["pose_texels"] > 0) if texels else (got["pose_texels"] == 0.0), f"{label}: {got}"
    got = _times(backend.pose_times)
    print(f"{label}: pose_times {got}")
    if got is not None:                                            # (of the last pass that wrote vertices)
        assert len(got) == 5 and all(v >= 0 for v in got.values()), f"{label}: {got}"


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_walk(api, layout):
    recipe, second, has_map = LAYOUTS[layout]
    index = recipe[1]
    m = _motion(api, recipe)
    steps = _states(second)
    wants = []                                                     # (the fresh scenes first: a new Material anywhere makes every scene upload its models again)
    for step, state in steps:
        other = _fresh(api, recipe, second, m, state)
        wants.append(counted(other._backend(), other))
        other.close()
    scene, _ = ref.build(api, recipe)
    backend, walker = scene._backend(), scene.models[index]
    other = None if second is None else scene.models[second]
    if other is not None:
        other.pose = m["second"]
    n_walker, n_second = m["verts"][index], 0 if second is None else m["verts"][second]
    passes, pass_seen = 0, False
    for (step, state), want in zip(steps, wants):
        label = f"{layout}, {step.label}"
        _do(step, walker, other, m)
        assert_same(counted(backend, scene), want, label)
        changed = step.label != "rest" or second is not None       # (at rest, and nothing posed: no pass at all)
        passes += 1 if changed else 0
        pass_seen = pass_seen or changed
        walker_written = n_walker if (state & {"morph", "skin", "pose"}) or step.label == "pose removed" else 0
        written = walker_written + n_second if step.geometry and changed else 0
        posed = int("pose" in state) + int(second is not None)
        counters = backend.pose_counters()
        print(f"{label}: pose_counters {counters}")
        assert counters == (1, passes, posed, written), f"{label}: {counters}"
        if pass_seen:
            mc, sk, au = backend.morph_counters(), backend.skin_counters(), backend.auto_normals_counters()
            print(f"{label}: morph {mc} skin {sk} auto_normals {au}")
            morph, skin = step.morph or (0, 0), step.skin or (0, 0)
            assert mc[0] == int("morph" in state) and mc[2:4] == (n_walker * morph[0], m["normals"] * morph[1]), f"{label}: {mc}"
            assert sk[0] == int("skin" in state) and sk[2:4] == (n_walker * skin[0], m["normals"] * skin[1]), f"{label}: {sk}"
            assert au[:2] == ((1, m["normals"]) if step.auto else (0, 0)), f"{label}: {au}"
        _check_times(backend, step, second is not None, has_map, label)
        if changed and step.label != "rest":
            _do(step, walker, other, m, again=True)                # the value it holds already: no pass
            backend.render(scene, shadows=True)
            assert backend.pose_counters() == counters, f"{label}: a repeated setter ran a pass"
    scene.close()
