"""GPU: frames that follow other frames are the frames of a fresh scene (tests/frame_sequences.py).

For each seed one long-lived scene and its backend render the sequence in order.  Every frame is held, bit for bit, to
its *twin*: a new scene built directly in that state with a new ``DeviceRenderer``, which renders that one frame once
with the same options and is closed (memoised by whole-frame state, part and mode).  Every twin is held to the
sequential oracle with the project's bars -- z bits, winners and every light's stencil exact, float frame 2e-6 (with n
lights n * 2e-6 + 1e-6, test_multilight_gpu.py's), uint8 +-1 -- over the rows it owns, so the yardstick is the oracle and
not the code under test.  What is carried from frame to frame (list cursors, double-buffered counters, class bytes,
tile order and split, the silhouette cache, pose and skin keys, learnt capacities, overlay lists, the Python layer's
one-entry caches) may cost time when it is stale, never a bit of the frame: DESIGN.md's claim, walked here.

The project already requires a second render to equal the first bit for bit whatever order the lists were filled in
(test_adversarial_gpu.py::test_seed_matches_oracle), so bit equality against the twin is the project's own bar."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import frame_sequences as fs
from frame_sequences import SEEDS, Walker, content_key, sequence, twin_key

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SMALL_LEN, BIG_LEN, QUAD_LEN = 5, 6, 7            # columns of a tile record (test_adversarial_gpu.py)
FORCED = dict(MR_TILE_ORDER="heaviest", MR_TILE_SPLIT="1", MR_CLUSTER_CULL="1")
CHILD_SEEDS = (1, 4)


def assert_within_bars(got, state, ref, label):
    """A twin's result against the oracle's whole frame, over the rows the twin owns."""
    own_top_first = np.flatnonzero(fs.own_rows(state)[::-1])
    out = got["out"][fs.out_rows(state)]
    assert out.shape == ref.out[own_top_first].shape, label
    d = np.abs(out.astype(np.int16) - ref.out[own_top_first].astype(np.int16))
    assert d.max() <= 1, f"{label}: uint8 frame off by {d.max()} ({int((d > 1).sum())} values > 1)"
    if state.mode != "counted":
        return
    rows = fs.tap_rows(state)
    bad_z = int((got["z"][rows] != ref.z.view(np.uint64)[rows]).sum())
    assert bad_z == 0, f"{label}: {bad_z} z-buffer entries not bit-exact"
    assert np.array_equal(got["winner"][rows], ref.winner[rows]), f"{label}: winner map differs"
    for k in range(state.lights):
        assert np.array_equal(got[f"stencil{k}"][rows], ref.stencils[k][rows]), f"{label}: stencil of light {k} differs"
    n = state.lights
    bound = 2e-6 if n == 1 else n * 2e-6 + 1e-6
    err = np.abs(got["frame"].view(np.float32)[rows].astype(np.float64) - ref.frame[rows].astype(np.float64)).max()
    assert err <= bound, f"{label}: float frame off by {err:.3g} (bound {bound:.3g})"
    return float(err)


@pytest.fixture(scope="module")
def twins(api, oracle_mod):
    """``get(state)`` -> the twin's result, rendered once per (whole-frame state, part, mode) by a scene and a
    DeviceRenderer of its own, closed afterwards, and held to the oracle; ``get.prepare(states)`` renders the oracle's
    frames of a sequence ahead, side by side."""
    done, refs, worst = {}, {}, {"float": 0.0, "oracle_s": 0.0, "twin_s": 0.0}

    def prepare(states):
        t0 = time.perf_counter()
        refs.update(fs.expected_many(api, oracle_mod, [s for s in states if content_key(s) not in refs]))
        worst["oracle_s"] += time.perf_counter() - t0

    def get(state):
        key = twin_key(state)
        if key not in done:
            plain = state._replace(lane=None, event="")
            t0 = time.perf_counter()
            rig = fs.Rig(api, plain)
            try:
                got = fs.render_state(rig, plain)
                assert not rig.scene._backend().overflowed(), f"the twin of {state} overflowed its lists"
            finally:
                rig.close()
            worst["twin_s"] += time.perf_counter() - t0
            if content_key(state) not in refs:
                prepare([state])
            err = assert_within_bars(got, plain, refs[content_key(state)], f"twin of {plain}")
            worst["float"] = max(worst["float"], err or 0.0)
            done[key] = got
        return done[key]

    get.prepare, get.done, get.worst = prepare, done, worst
    return get


def _changed(a, b):
    return ", ".join(f"{f} {getattr(a, f)} -> {getattr(b, f)}" for f in a._fields if getattr(a, f) != getattr(b, f)) or "nothing"


def _check_flags(states, flags, label):
    squeezed = {i for i, s in enumerate(states) if s.event == "squeeze"}
    assert len(squeezed) == 1
    for i, flag in sorted(flags.items()):
        assert flag == (i in squeezed), f"{label}: overflowed() said {flag} after frame {i}"
    assert squeezed <= set(flags) and len(states) in flags


@pytest.mark.parametrize("seed", SEEDS)
def test_every_frame_of_a_sequence_equals_its_twin(api, twins, seed):
    """The uint8 rows always; in counted mode z, winner, every light's stencil, the float frame, the silhouette set and
    the counters too, and the face status where it was asked for.  ``overflowed()`` is set after the squeezed frame's
    first enqueue and at no other time, and ``stats()`` reports no overflow left behind."""
    states = sequence(seed)
    twins.prepare(states)
    walker = Walker(api, states)
    differ = []
    try:
        for i, state, got in walker.frames():
            why = fs.same(got, twins(state), state)
            if why:
                differ.append(f"frame {i} ({_changed(states[i - 1], state) if i else 'first'}): {why}")
        walker.backend.stats()
    finally:
        walker.close()
    print(f"seed {seed}: {len(states)} frames, {len(twins.done)} twins so far, {walker.rerendered} lane frames rendered again, "
          f"worst float error of a twin {twins.worst['float']:.3g}; so far {twins.worst['oracle_s']:.1f} s in the oracle, "
          f"{twins.worst['twin_s']:.1f} s in the twins")
    assert not differ, f"seed {seed}: {len(differ)} frames differ from their twins:\n" + "\n".join(differ[:12])
    _check_flags(states, walker.flags, f"seed {seed}")


def test_what_the_library_refuses_the_python_layer_refuses(api):
    """The combinations the walk leaves out, pinned where they are refused.  The library renders a row band or a stripe
    with MR_FRAME_FACE_STATUS and then refuses to hand the status out (mr_read_face_status); ``DeviceRenderer.render``
    used to let such a frame through and fail at the read, and now refuses it like the others, before any device work
    for the frame."""
    rig = fs.Rig(api, fs.BASE)
    scene, backend = rig.scene, rig.scene._backend()
    try:
        whole = backend.render(scene, face_status=True).copy()
        assert len(backend.read_face_status()) == sum(len(m._faces) for m in scene.models)
        for kw in (dict(row_band=(0, 45)), dict(row_band=(45, 136)), dict(stripe=(1, 3))):
            with pytest.raises(ValueError, match="per-face status"):
                backend.render(scene, face_status=True, **kw)
        assert np.array_equal(backend.render(scene, face_status=True, row_band=(0, 136)), whole)
        backend.read_face_status()
        with pytest.raises(RuntimeError, match="overlay"):
            backend.render(scene, row_band=(0, 45), overlay=True)
        rig.put(fs.BASE._replace(lights=2))
        for kw in (dict(face_status=True), dict(stripe=(0, 2))):
            with pytest.raises(ValueError, match="more than one light"):
                backend.render(scene, **kw)
        rig.put(fs.BASE._replace(supersample=2))
        with pytest.raises(RuntimeError, match="striped"):
            backend.render(scene, stripe=(0, 2))
        rig.put(fs.BASE)
        assert np.array_equal(backend.render(scene, face_status=True), whole)
    finally:
        rig.close()


def test_the_sequences_reach_what_they_were_made_for(api):
    """Over the six walks: a tile that meets the small grid's split thresholds (32 quads, cost 350) in a frame whose
    slot rendered the same number of tiles the frame before; tile orders that are permutations of their grids, and one
    that is not row-major (the history was used); the silhouette cache's fused or capture path and its cached path;
    pose passes and skinned vertices.  A table that misses one of these is changed, not this list."""
    seen = dict(frames=0, split_after_same_count=0, split_tiles=0, reordered=0, paths=set(), most_quads=0, most_cost=0)
    counters = {}

    for seed in SEEDS:
        last = {"tiles": None}

        def probe(i, state, backend):
            rec = backend.read_tile_records().astype(np.int64)
            order = backend.read_tile_order().astype(np.int64)
            assert np.array_equal(np.sort(order), np.arange(len(rec))), f"seed {seed} frame {i}: the tile order is no permutation"
            cost = 20 + 2 * rec[:, SMALL_LEN] + 30 * rec[:, BIG_LEN] + 3 * rec[:, QUAD_LEN]
            split = (rec[:, QUAD_LEN] >= 32) & (cost >= 350)
            seen["frames"] += 1
            seen["split_tiles"] += int(split.sum())
            seen["most_quads"] = max(seen["most_quads"], int(rec[:, QUAD_LEN].max()))
            seen["most_cost"] = max(seen["most_cost"], int(cost.max()))
            if split.any() and last["tiles"] == len(rec) and len(rec) <= 2048:
                seen["split_after_same_count"] += 1
            seen["reordered"] += int(not np.array_equal(order, np.arange(len(rec))))
            if state.shadows:
                seen["paths"].add(backend.sil_cache()[0])
            last["tiles"] = len(rec)

        walker = Walker(api, sequence(seed), probe=probe)
        try:
            for _ in walker.frames():
                pass
            counters[seed] = (walker.backend.pose_counters(), walker.backend.skin_counters(), walker.backend.sil_cache())
        finally:
            walker.close()
    print(f"probed frames {seen['frames']}; frames with a tile over the split thresholds after a frame of the same tile count "
          f"{seen['split_after_same_count']} ({seen['split_tiles']} such tiles in all, most quads in a tile {seen['most_quads']}, "
          f"highest cost {seen['most_cost']}); frames not in row-major order {seen['reordered']}; silhouette paths {sorted(seen['paths'])}")
    for seed, (pose, skin, sil) in counters.items():
        print(f"seed {seed}: commits {pose[0]}, pose passes {pose[1]}, skinned vertices of the last pass {skin[2]}, "
              f"bone matrices {skin[1]}, silhouette captures {sil[2]}")
    assert seen["split_after_same_count"] >= 1
    assert seen["reordered"] >= 1
    assert seen["paths"] & {0, 1} and 2 in seen["paths"], seen["paths"]
    for seed, (pose, skin, sil) in counters.items():
        assert pose[0] >= 2 and pose[1] >= 3, f"seed {seed}: {pose}"          # the edit committed again; poses and bones moved
        assert skin[0] == 1 and skin[1] > 0 and skin[2] > 0, f"seed {seed}: {skin}"


_CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import scenes
import frame_sequences as fs
api = scenes.product_api()
saved = {{}}
for seed in {seeds!r}:
    states = fs.sequence(seed)
    walker = fs.Walker(api, states)
    for i, state, got in walker.frames():
        for key, value in got.items():
            saved[f"{{seed}}_{{i}}_{{key}}"] = value
    walker.backend.stats()
    saved[f"{{seed}}_flags"] = np.array(sorted((i, int(flag)) for i, flag in walker.flags.items()), dtype=np.int64)
    walker.close()
np.savez({path!r}, **saved)
"""


def test_forced_order_split_and_culling_change_no_frame(api, twins, tmp_path):
    """Two sequences in a fresh interpreter under MR_TILE_ORDER=heaviest MR_TILE_SPLIT=1 MR_CLUSTER_CULL=1 (read per
    process or per frame: a child, as in test_edge_spread_gpu.py): the stale history and the split are used on every
    grid, not only where the defaults choose them.  Held to the same twins, rendered here under the default
    environment."""
    path = str(tmp_path / "forced.npz")
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), seeds=CHILD_SEEDS, path=path)
    env = dict(os.environ, **FORCED)
    proc = subprocess.run([sys.executable, "-c", code], env=env, timeout=300, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-3000:]
    saved = np.load(path)
    differ = []
    for seed in CHILD_SEEDS:
        states = sequence(seed)
        twins.prepare(states)
        for i, state in enumerate(states):
            prefix = f"{seed}_{i}_"
            got = {name[len(prefix):]: saved[name] for name in saved.files if name.startswith(prefix)}
            assert got, f"seed {seed}: frame {i} is missing"
            why = fs.same(got, twins(state), state)
            if why:
                differ.append(f"seed {seed} frame {i} ({_changed(states[i - 1], state) if i else 'first'}): {why}")
        _check_flags(states, {int(i): bool(flag) for i, flag in saved[f"{seed}_flags"]}, f"seed {seed}, forced")
    assert not differ, f"{len(differ)} frames differ from their twins:\n" + "\n".join(differ[:12])


def test_four_frames_in_flight_end_at_the_twin(api, twins):
    """``BandRenderer(scene, 0, 1, frames_in_flight=4)`` through one seed's whole-frame, frame-mode states with one light
    and no supersampling (what it accepts): the scene is moved on between ``synchronize()`` and the next ``prime()``,
    four frames are enqueued on four streams, and the last one is the twin's uint8 frame.  A renderer's size, shadows
    and overlay are fixed when it is built: another one takes over the same streams when they change."""
    import torch
    from py_numpy_renderer_amd.multigpu import BandRenderer
    states = [s._replace(lane=None, event="") for s in sequence(5)
              if s.part == fs.WHOLE and s.mode == "frame" and s.supersample == 1 and s.lights == 1]
    states = [s for i, s in enumerate(states) if i == 0 or s != states[i - 1]]
    assert len(states) >= 6 and len({s.grid for s in states}) >= 2, states
    twins.prepare(states)
    streams = [torch.cuda.Stream() for _ in range(4)]
    rig = fs.Rig(api, states[0])
    renderer, built_for = None, None
    try:
        for i, state in enumerate(states):
            rig.put(state)
            fixed = (state.grid, state.shadows, state.overlay)
            if fixed != built_for:
                if renderer is not None:
                    renderer.synchronize()
                renderer = BandRenderer(rig.scene, 0, 1, shadows=state.shadows, frames_in_flight=4, overlay=state.overlay,
                                        streams=streams)
                built_for = fixed
            else:
                renderer.prime()
            for _ in range(4):
                frame = renderer.step()
            assert renderer.verify(), f"state {i}: a frame in flight overflowed its lists"
            got = frame.cpu().numpy()
            want = twins(state)["out"]
            assert got.shape == want.shape, (i, state)
            bad = int((got != want).any(axis=-1).sum())
            assert bad == 0, f"state {i} ({_changed(states[i - 1], state) if i else 'first'}): {bad} pixels differ from the twin"
    finally:
        if renderer is not None:
            renderer.synchronize()
        rig.close()
    print(f"{len(states)} states, four frames in flight each")
