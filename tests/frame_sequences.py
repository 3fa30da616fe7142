"""Seeded sequences of frames for one long-lived scene: the state space, the covering walk, and the walker that renders it.

Almost every GPU test builds a scene, renders it once or twice and closes it.  The renderer is made for the opposite:
one ``mr_scene``, a few frame slots and thousands of frames, with state carried from each frame into the next -- list
cursors zeroed by the tile kernel that read them, frame counters cleared by the previous frame, the tiles' class bytes
and the order and split derived from them, the silhouette cache, pose and skin keys, learnt list capacities, overlay
lists, and the one-entry caches of ``DeviceRenderer``.  ``sequence(seed)`` is a list of frame *states* (``State``) that
walks that protocol: tests/test_frame_sequences_cpu.py holds the walk to what it must cover, and
tests/test_frame_sequences_gpu.py renders it on one scene and holds every frame to the same frame of a scene that has
never rendered anything (``Rig`` built directly in the state: the *twin*), and that one to the oracle.

A state names, per axis, an index or value of the tables below.  ``legal`` restates what the library
(``validate_frame``, ``mr_render``, ``mr_read_face_status``) and ``DeviceRenderer._prepare`` accept: several lights
exclude stripes and the face status, the face status and the overlay come with whole frames only, a supersampled frame
has no stripes.

The walk.  For the axes of ``AXES`` every ordered pair of distinct values occurs as a transition between two consecutive
frames of some seed (``PAIRS``, dealt round-robin over ``SEEDS``); the other axes are drawn from the seed meanwhile.
Every seed also holds the scripted transitions of ``SCRIPTED`` (``spans(seed)`` says where), and visits every grid and
every kind of part.  The camera with nothing on the screen appears only between two frames that show the mesh: next to
it a change of light or pose alone would not show in any frame, and the oracle could not tell a stale frame from a new one.
"""
import copy
from collections import namedtuple

import numpy as np

import scenes

# ----------------------------------------------------------------------------------------------- the tables
GRIDS = ((136, 152), (152, 136), (144, 160), (72, 88))       # 9x10 tiles, 10x9, 9x10 without a ragged edge, 5x6
SUPERSAMPLE = (1, 2, 4)
WHOLE = ("whole",)
BANDS = (("band", 0, 3), ("band", 1, 3), ("band", 2, 3))      # band k of n, cut at rows that are no multiple of 16
STRIPES = (("stripe", 0, 2), ("stripe", 1, 3), ("stripe", 2, 3))
PART_KINDS = ("whole", "band", "stripe")
LIGHTS = (1, 2, 4)
MODES = ("counted", "frame")
LIGHT_AT = ((2.0, 3.0, 4.0), (-1.5, 3.5, 2.5))                 # where light 0 stands
# the mesh under its shadow volume; grazing, a fifth of a unit above the floor; looking away from everything
CAMERAS = (((0.5, 1.0, 2.0), (0.0, 0.0, 0.0)), ((2.5, -0.8, 0.2), (0.0, 0.0, 0.0)), ((0.5, 1.0, 2.0), (3.0, 6.0, 6.0)))
HEAVY, GRAZING, EMPTY = 0, 1, 2
DEBUG_CAMERA = ((-2.0, 1.5, 1.5), (0.0, 0.0, 0.0))            # whose frustum the overlay draws (and which clips, as upstream)
CAMERA_KW = dict(fovy=60, near=0.1, far=20, backface_culling=True)
N_POSES, N_BONES = 3, 2                                        # Model.pose: None and two matrices; Model.bones: two sets
EDIT_ROWS, EDIT_SHIFT = slice(0, 160), (0.0, 0.18, 0.0)        # the in-place vertex edit (then Model.invalidate())
SQUEEZED = dict(small_pairs=4, big_pairs=2, quads=3, work=16)  # test_dense_tile_with_lists_far_too_small's capacities
ASYNC_LANES = 4
SEEDS = tuple(range(6))

State = namedtuple("State", "grid supersample part lights light_at shadows overlay face_status mode lane camera pose "
                            "bones edited event")
BASE = State(grid=0, supersample=1, part=WHOLE, lights=1, light_at=0, shadows=True, overlay=False, face_status=False,
             mode="frame", lane=None, camera=HEAVY, pose=0, bones=0, edited=False, event="")

AXES = {"grid": tuple(range(len(GRIDS))), "supersample": SUPERSAMPLE, "part": PART_KINDS, "lights": LIGHTS, "mode": MODES,
        "shadows": (True, False), "overlay": (False, True)}
PAIRS = tuple((axis, a, b) for axis, values in AXES.items() for a in values for b in values if a != b)
SCRIPTED = ("grid_flip", "band_whole_band", "stripe_whole", "counted_frame_counted", "split_history", "overflow",
            "empty_between_heavy", "lanes", "light_moves_under_a_warm_cache")


def axis_value(state, axis):
    return state.part[0] if axis == "part" else getattr(state, axis)


def content_key(state):
    """What the whole frame shows: everything but which rows are rendered, how, and on which lane."""
    return (state.grid, state.supersample, state.lights, state.light_at, state.shadows, state.overlay, state.camera,
            state.pose, state.bones, state.edited)


def twin_key(state):
    """What a twin is memoised by: the whole-frame state, the part and the mode (with what the mode was asked for)."""
    return content_key(state) + (state.part, state.mode, state.face_status)


def legal(state):
    """What the library and the Python layer accept of a state (and what this walk keeps to: the face status comes with
    counted frames, a lane with whole frame-mode frames, the squeezed lists with a whole frame)."""
    kind = state.part[0]
    if state.lights > 1 and (kind == "stripe" or state.face_status):
        return False
    if state.supersample > 1 and kind == "stripe":
        return False
    if state.overlay and kind != "whole":
        return False
    if state.face_status and (state.mode != "counted" or kind != "whole"):
        return False
    if state.lane is not None and (state.mode != "frame" or kind != "whole"):
        return False
    if state.event == "squeeze" and (kind != "whole" or state.lane is not None):
        return False
    return state.event in ("", "squeeze")


def legalise(state, keep=None):
    """The nearest legal state that keeps the value of axis *keep*."""
    s = state
    if s.part[0] == "stripe" and (s.lights > 1 or s.supersample > 1):
        s = s._replace(lights=1, supersample=1) if keep == "part" else s._replace(part=WHOLE)
    if s.overlay and s.part != WHOLE:
        s = s._replace(part=WHOLE) if keep == "overlay" else s._replace(overlay=False)
    if s.face_status and (s.lights > 1 or s.mode != "counted" or s.part != WHOLE):
        s = s._replace(face_status=False)
    if s.lane is not None and (s.mode != "frame" or s.part != WHOLE):
        s = s._replace(lane=None)
    assert legal(s), s
    return s


# ----------------------------------------------------------------------------------------------- rows of a part
def band_rows(state):
    """(begin, end) output rows of a band state, else None: band k of n is cut at ``round(H * k / n)``."""
    if state.part[0] != "band":
        return None
    _, k, n = state.part
    h = GRIDS[state.grid][0]
    return (h * k + n // 2) // n, (h * (k + 1) + n // 2) // n


def stripe_of(state):
    return (state.part[1], state.part[2]) if state.part[0] == "stripe" else None


def own_rows(state):
    """bool (H,): the output pixel rows, counted from the bottom like the device's buffers, that the state's part owns."""
    h = GRIDS[state.grid][0]
    y = np.arange(h)
    if state.part[0] == "band":
        r0, r1 = band_rows(state)
        return (y >= h - r1) & (y < h - r0)
    if state.part[0] == "stripe":
        return (y // 16) % state.part[2] == state.part[1]
    return np.ones(h, bool)


def tap_rows(state):
    """The same for the taps, which are buffers of the sample grid."""
    return np.repeat(own_rows(state), state.supersample)


def out_rows(state):
    """For every owned output row, top first (the order of the uint8 frame): its row in the array the render returns --
    the band's rows in order, or the striped layout (multigpu.unstripe_index: the rank's tile rows highest first, rows
    inside a tile row top-down, padded to the longest rank's share)."""
    h = GRIDS[state.grid][0]
    if state.part[0] == "band":
        r0, r1 = band_rows(state)
        return np.arange(r1 - r0)
    if state.part[0] != "stripe":
        return np.arange(h)
    _, index, count = state.part
    per = -(-(-(-h // 16)) // count) * 16
    py = h - 1 - np.arange(h)
    g = py // 16
    local = (per // 16 - 1 - g // count) * 16 + (16 * g + 15 - py)
    return local[g % count == index]


# ----------------------------------------------------------------------------------------------- the walk
def _scripted(name, cur, rng):
    """The states of one scripted transition, continued from *cur*."""
    if name == "grid_flip":                        # 9x10 -> 10x9 -> 9x10, nothing else changed
        s = legalise(cur._replace(grid=0, event=""))
        return [s, s._replace(grid=1), s]
    if name == "band_whole_band":                  # a slot renders rows it did not own in the frame before
        k, k2 = (int(v) for v in rng.choice(3, 2, replace=False))
        s = legalise(cur._replace(part=BANDS[k], overlay=False, lane=None, event=""), keep="part")
        return [s, s._replace(part=WHOLE), s._replace(part=BANDS[k2])]
    if name == "stripe_whole":
        s = legalise(cur._replace(part=STRIPES[int(rng.integers(3))], overlay=False, lane=None, event=""), keep="part")
        return [s, s._replace(part=WHOLE)]
    if name == "counted_frame_counted":            # on one slot: no lane
        s = cur._replace(mode="counted", lane=None, event="")
        return [s, s._replace(mode="frame", face_status=False), s]
    if name == "split_history":
        # a frame whose heaviest tile qualifies for the split; again, now ordered and split from the class bytes it
        # left; under four lights, where no tile is split; one light again
        s = cur._replace(grid=int(rng.integers(3)), supersample=1, part=WHOLE, lights=1, shadows=True, camera=HEAVY,
                         lane=None, face_status=False, event="")
        return [s, s, s._replace(lights=4), s]
    if name == "overflow":
        # a frame; the lists squeezed far below what it needs, so that the next one overflows; a frame of another grid
        s = cur._replace(part=WHOLE, camera=HEAVY, shadows=True, lane=None, event="")
        other = (s.grid + 1 + int(rng.integers(3))) % len(GRIDS)
        return [s, s._replace(event="squeeze"), s._replace(grid=other)]
    if name == "empty_between_heavy":              # every tile takes the empty-tile exit and still leaves its state right
        s = cur._replace(camera=HEAVY, event="")
        return [s, s._replace(camera=EMPTY), s]
    if name == "lanes":                            # lanes 0, 1, 2, 0, then a synchronous frame: plan_frame's "alone" both ways
        s = legalise(cur._replace(mode="frame", part=WHOLE, face_status=False, camera=HEAVY, event=""))
        return [s._replace(lane=0), s._replace(lane=1, camera=GRAZING), s._replace(lane=2), s._replace(lane=0, camera=GRAZING),
                s._replace(lane=None)]
    if name == "light_moves_under_a_warm_cache":
        # one light three times -- the silhouette cache sees its key, captures, serves -- then the light somewhere else,
        # where the cached silhouette is the wrong one, and back, where the cache still holds the right one
        s = legalise(cur._replace(lights=1, shadows=True, lane=None, event=""))
        moved = s._replace(light_at=1 - s.light_at)
        return [s, s, s, moved, s]
    raise KeyError(name)


def _drift(state, rng, step, seed):
    """One of the axes that the pairs do not cover, changed from the seed: camera (never the empty one), where light 0
    stands, the pose, the face status, the lane, which band or stripe.  The one change of bones and the one in-place
    edit of a sequence come at fixed steps."""
    s = state._replace(event="")
    what = int(rng.integers(7))
    if what == 0:
        s = s._replace(camera=GRAZING if s.camera == HEAVY else HEAVY)
    elif what == 1:
        s = s._replace(light_at=1 - s.light_at)
    elif what == 2:
        s = s._replace(pose=(s.pose + 1 + int(rng.integers(N_POSES - 1))) % N_POSES)
    elif what == 3:
        s = s._replace(face_status=not s.face_status)
    elif what == 4:
        s = s._replace(lane=None if s.lane is not None else int(rng.integers(ASYNC_LANES)))
    elif what == 5 and s.part[0] == "band":
        s = s._replace(part=BANDS[(s.part[1] + 1 + int(rng.integers(2))) % 3])
    elif what == 5 and s.part[0] == "stripe":
        s = s._replace(part=STRIPES[(STRIPES.index(s.part) + 1 + int(rng.integers(2))) % 3])
    if step == 2 + seed % 3:
        s = s._replace(bones=1)
    if step == 6 + seed % 3:
        s = s._replace(edited=True)
    return s


def _with_axis(state, axis, value, rng):
    if axis != "part":
        return state._replace(**{axis: value})
    table = {"whole": (WHOLE,), "band": BANDS, "stripe": STRIPES}[value]
    return state._replace(part=table[int(rng.integers(len(table)))])


def _build(seed):
    rng = np.random.default_rng(20261101 + seed)
    states, where = [], {}
    cur = BASE._replace(mode=MODES[seed % 2], light_at=seed % 2, pose=seed % N_POSES)
    pairs = [p for i, p in enumerate(PAIRS) if i % len(SEEDS) == seed]
    names = list(SCRIPTED[seed % len(SCRIPTED):] + SCRIPTED[:seed % len(SCRIPTED)])
    step = 0
    while pairs or names:
        if names:                                  # a scripted transition, then a pair, in turn
            name = names.pop(0)
            block = _scripted(name, cur, rng)
            where[name] = (len(states), len(states) + len(block))
            states += block
            cur = block[-1]._replace(event="")
        if pairs:
            axis, a, b = pairs.pop(0)
            first = legalise(_with_axis(_drift(cur, rng, step, seed), axis, a, rng), keep=axis)
            if first.camera == EMPTY:
                first = first._replace(camera=HEAVY)
            second = legalise(_with_axis(_drift(first, rng, step + 1, seed), axis, b, rng), keep=axis)
            step += 2
            if not states or first != states[-1]:
                states.append(first)
            states.append(second)
            cur = second
    for grid in range(len(GRIDS)):                 # every seed visits every grid and every kind of part
        if all(s.grid != grid for s in states):
            states.append(legalise(cur._replace(grid=grid)))
    for kind in PART_KINDS:
        assert any(s.part[0] == kind for s in states), kind
    assert all(legal(s) for s in states)
    return states, where


_BUILT = {}


def sequence(seed):
    """The states of one seed, in order."""
    if seed not in _BUILT:
        _BUILT[seed] = _build(seed)
    return list(_BUILT[seed][0])


def spans(seed):
    """``{name of a scripted transition: (first index, index past its last)}`` in ``sequence(seed)``."""
    sequence(seed)
    return dict(_BUILT[seed][1])


# ----------------------------------------------------------------------------------------------- scenes in a state
_TEMPLATE = {}


def _template(api):
    """diablo_small's model over the floor, loaded once; its rig (skin_ref's ``bend``, from the vertices as loaded)."""
    if "models" not in _TEMPLATE:
        import skin_ref
        _TEMPLATE["models"] = scenes.diablo_floor(api, resolution=GRIDS[0]).models
        mesh = _TEMPLATE["models"][0]
        joints, weights, _ = skin_ref.rig(api, mesh, "bend", 0)
        _TEMPLATE["skin"] = (joints, weights)
        _TEMPLATE["bones"] = tuple(skin_ref.rig(api, mesh, "bend", frame)[2] for frame in (0, 5))
    return _TEMPLATE


def poses(api):
    import pose_ref
    m = pose_ref.matrices(api)
    return (None, m["rotation"], m["translation"])


def _models(api):
    mesh, floor = (copy.copy(m) for m in _template(api)["models"])
    mesh.vertices = np.array(mesh.vertices)                  # (its own: the in-place edit must not reach the template)
    return mesh, floor


def _edit(vertices):
    vertices[EDIT_ROWS, :3] += np.asarray(EDIT_SHIFT, dtype=vertices.dtype)


def _cameras(api, index):
    (eye, centre), (dbg_eye, dbg_centre) = CAMERAS[index], DEBUG_CAMERA
    return api.Camera(eye, centre, **CAMERA_KW), api.Camera(dbg_eye, dbg_centre, **CAMERA_KW)


def _light(api, at):
    return api.Light(LIGHT_AT[at], ambient_strength=0.1, specular_strength=0.1)


class Rig:
    """A scene and what ``put`` needs to move it from state to state through the product's own interface:
    ``scene.resolution``, ``supersample``, the cameras (a pair of objects per camera and grid, kept: a camera's matrices
    are cached for life, as upstream), ``light.set_position``, ``add_light`` / ``clear_lights``, ``Model.pose``,
    ``Model.bones``, an in-place edit with ``invalidate()``, ``draw_debug_frustum``.  ``Rig(api, state)`` is the twin of
    a state: built directly in it."""

    def __init__(self, api, state):
        from multilight_ref import extra_lights
        from py_numpy_renderer_amd import Skin
        self.api = api
        t = _template(api)
        self.mesh, floor = _models(api)
        self.cams = {(state.camera, state.grid): _cameras(api, state.camera)}
        cam, dbg = self.cams[state.camera, state.grid]
        self.scene = api.Scene(cam, _light(api, state.light_at), debug_camera=dbg, resolution=GRIDS[state.grid])
        self.scene.add_model(self.mesh), self.scene.add_model(floor)
        self.extras = extra_lights(api)
        self.poses = poses(api)
        self.light_at, self.edited = state.light_at, False
        if state.edited:                           # (the twin's mesh has the edit before its first commit)
            _edit(self.mesh.vertices)
            self.edited = True
        self.mesh.skin = Skin(*t["skin"])
        self.put(state)

    def put(self, state):
        scene, mesh = self.scene, self.mesh
        if tuple(scene.resolution) != GRIDS[state.grid]:
            scene.resolution = GRIDS[state.grid]
        key = (state.camera, state.grid)
        if key not in self.cams:
            self.cams[key] = _cameras(self.api, state.camera)
        if scene.camera is not self.cams[key][0]:
            scene.camera, scene.debug_camera = self.cams[key]
        scene.supersample = state.supersample
        if self.light_at != state.light_at:
            scene.light.set_position(np.array(LIGHT_AT[state.light_at]))
            self.light_at = state.light_at
        if len(scene.lights) != state.lights:
            scene.clear_lights()
            for light in self.extras[:state.lights - 1]:
                scene.add_light(light)
        if state.edited and not self.edited:
            _edit(mesh.vertices)
            mesh.invalidate()
            self.edited = True
        assert state.edited == self.edited, "an edit is not taken back"
        bones = _template(self.api)["bones"][state.bones]
        if mesh.bones is None or mesh.bones.tobytes() != bones.tobytes():
            mesh.bones = bones
        pose = self.poses[state.pose]
        if (mesh.pose is None) != (pose is None) or (pose is not None and mesh.pose.tobytes() != pose.tobytes()):
            mesh.pose = pose
        scene.draw_debug_frustum = bool(state.overlay)

    def close(self):
        self.scene.close()


_REFERENCE_VERTICES = {}


def reference_scene(api, state):
    """The scene the oracle renders for a state, restated without the features under test: at the sample grid's
    resolution (supersample_ref), one light at a time (multilight_ref.compose swaps them), the mesh's vertices replaced
    by skin_ref's and pose_ref's pure-Python chains."""
    import pose_ref
    import skin_ref
    from multilight_ref import extra_lights
    t = _template(api)
    mesh, floor = _models(api)
    key = (state.edited, state.bones)
    if key not in _REFERENCE_VERTICES:
        if state.edited:
            _edit(mesh.vertices)
        joints, weights = t["skin"]
        _REFERENCE_VERTICES[key] = skin_ref.skinned_vertices(mesh.vertices, joints, weights, t["bones"][state.bones])
    mesh.vertices = _REFERENCE_VERTICES[key].copy()
    pose = poses(api)[state.pose]
    if pose is not None:
        mesh.vertices = pose_ref.posed_vertices(mesh, pose)
    mesh._revision += 1
    s = state.supersample
    h, w = GRIDS[state.grid]
    cam, dbg = _cameras(api, state.camera)
    scene = api.Scene(cam, _light(api, state.light_at), debug_camera=dbg, resolution=(s * h, s * w))
    scene.add_model(mesh), scene.add_model(floor)
    for light in extra_lights(api)[:state.lights - 1]:
        scene.add_light(light)
    scene.draw_debug_frustum = False
    return scene


def expected(api, oracle_mod, state):
    """The oracle's buffers of a state's whole frame: ``compose`` over its lights on the sample grid (overlay included),
    and ``out``, the uint8 frame after supersample_ref's resolve."""
    from multilight_ref import compose
    from supersample_ref import resolve
    ref = compose(oracle_mod, reference_scene(api, state), shadows=state.shadows, overlay=state.overlay)
    if state.supersample > 1:
        ref.out = resolve(ref.frame, state.supersample)
    return ref


def expected_many(api, oracle_mod, states, keep=lambda ref: ref, workers=8):
    """``{content_key: keep(expected(state))}`` of every distinct whole-frame state of *states*.  The oracle keeps no
    state between calls and runs outside the interpreter's lock, every state has a scene of its own: a few threads
    render them side by side (what is shared -- the template, the skinned vertices -- is made before they start)."""
    import os
    from concurrent.futures import ThreadPoolExecutor
    todo = {}
    for state in states:
        todo.setdefault(content_key(state), state)
    oracle_mod.lib()
    for state in todo.values():
        reference_scene(api, state)
    with ThreadPoolExecutor(max_workers=max(1, min(workers, os.cpu_count() or 1))) as pool:
        done = list(pool.map(lambda state: keep(expected(api, oracle_mod, state)), todo.values()))
    return dict(zip(todo, done))


# ----------------------------------------------------------------------------------------------- rendering a state
COUNTERS = ("frag_tri", "frag_quad", "n_quads", "n_quads_drawn", "covered_px", "lit_px", "stencil_updates")


def _sorted_rows(rows):
    rows = np.asarray(rows, dtype=np.int32).reshape(-1, 3)
    return rows[np.lexsort(rows.T[::-1])] if len(rows) else rows


def read_counted(backend, state, out):
    """Everything a counted frame leaves, as arrays: the uint8 rows, z as uint64, winner, float frame as uint32, every
    light's stencil and silhouette (sorted rows), the counters, the face status where asked for."""
    got = dict(out=np.array(out), z=backend.read_z().view(np.uint64), winner=backend.read_winner(),
               frame=backend.read_frame_f32().view(np.uint32),
               counters=np.array([backend.last_stats[k] for k in COUNTERS], dtype=np.int64))
    for k in range(state.lights):
        got[f"stencil{k}"] = backend.read_stencil(light=k)
        got[f"sil{k}"] = _sorted_rows(backend.read_silhouette(light=k))
    if state.face_status:
        got["face_status"] = backend.read_face_status()
    return got


def render_state(rig, state):
    """One synchronous frame of *rig* (already ``put`` in *state*) in the state's mode."""
    scene, backend = rig.scene, rig.scene._backend()
    band, stripe = band_rows(state), stripe_of(state)
    if state.mode == "counted":
        out = backend.render(scene, shadows=state.shadows, row_band=band, stripe=stripe, keep_float=True,
                             face_status=state.face_status, counters=True, overlay=state.overlay)
        return read_counted(backend, state, out)
    if stripe is not None:                         # (Scene.render has no stripes: the call it makes, with one)
        out = backend.render(scene, shadows=state.shadows, stripe=stripe, counters=False, keep_buffers=False, timing=False)
    else:
        out = scene.render(shadows=state.shadows, row_band=band)
    return dict(out=np.array(out))


def same(got, want, state):
    """None when two results of one state are equal bit for bit on the rows the state's part owns, else what differs."""
    if set(got) != set(want):
        return f"keys {sorted(got)} != {sorted(want)}"
    taps, rows = tap_rows(state), out_rows(state)
    for key, w in want.items():
        g = got[key]
        if g.shape != w.shape:
            return f"{key}: shape {g.shape} != {w.shape}"
        if key == "out":
            g, w = g[rows], w[rows]
        elif key in ("z", "winner", "frame") or key.startswith("stencil"):
            g, w = g[taps], w[taps]
        if not np.array_equal(g, w):
            bad = g != w
            if key == "counters":
                return f"counters {dict(zip(COUNTERS, g.tolist()))} != {dict(zip(COUNTERS, w.tolist()))}"
            return f"{key}: {int(bad.sum())} of {bad.size} values differ"
    return None


class Walker:
    """One long-lived scene and backend that render a sequence in order.  ``frames(states)`` yields
    ``(index, state, result)`` in order; ``flags[i]`` is what ``overflowed()`` said after frame i (for the squeezed
    frame: after its first enqueue with the short lists), ``probe(index, state, backend)`` is called after every
    synchronous frame, before anything else touches the backend."""

    def __init__(self, api, states, probe=None):
        self.states, self.probe = list(states), probe
        self.rig = Rig(api, self.states[0])
        self.backend = self.rig.scene._backend()
        self.flags = {}
        self.rerendered = 0                        # frames a lane reported as overflowed

    def _squeezed(self, state):
        """The lists set far too small, and the state's frame enqueued once with them on the slot mr_render uses: it
        must report the overflow (the lists are grown by that report)."""
        import torch
        scene, backend = self.rig.scene, self.backend
        backend.set_list_capacities(**SQUEEZED)
        h, w = GRIDS[state.grid]
        out = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
        backend.render_device(scene, out.data_ptr(), 0, shadows=state.shadows, no_timing=True, overlay=state.overlay)
        torch.cuda.synchronize()
        return backend.overflowed()

    def _wait(self, pending, done):
        index, state, out = pending
        if not self.backend.render_wait(state.lane):           # overflowed, lists grown: rendered again, as documented
            self.rerendered += 1
            self.rig.put(state)
            out = self.rig.scene.render(shadows=state.shadows)
        done[index] = dict(out=np.array(out))

    def frames(self):
        pending, done, emitted = {}, {}, 0         # lane -> (index, state, array) in flight

        def drain():
            for lane in sorted(pending, key=lambda k: pending[k][0]):
                self._wait(pending.pop(lane), done)

        for i, state in enumerate(self.states):
            prev = self.states[i - 1] if i else state
            only_view = prev._replace(camera=0, lane=None) == state._replace(camera=0, lane=None)
            if state.lane is None or not only_view:            # frames stay in flight only while nothing but the view changes
                drain()
            elif state.lane in pending:
                self._wait(pending.pop(state.lane), done)
            self.rig.put(state)
            if state.lane is not None:
                out = self.backend.render_async(self.rig.scene, state.lane, shadows=state.shadows, overlay=state.overlay)
                pending[state.lane] = (i, state, out)
            else:
                if state.event == "squeeze":
                    self.flags[i] = self._squeezed(state)
                done[i] = render_state(self.rig, state)
                if self.probe is not None:
                    self.probe(i, state, self.backend)
                if state.event != "squeeze":
                    self.flags[i] = self.backend.overflowed()
            while emitted in done:
                yield emitted, self.states[emitted], done.pop(emitted)
                emitted += 1
        drain()
        self.flags[len(self.states)] = self.backend.overflowed()
        while emitted in done:
            yield emitted, self.states[emitted], done.pop(emitted)
            emitted += 1

    def close(self):
        self.rig.close()
