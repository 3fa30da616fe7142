"""The walk of tests/frame_sequences.py is worth running: what it covers, and that the oracle tells its frames apart.

No GPU.  The census holds the generator to the transitions tests/test_frame_sequences_gpu.py is there to walk; the
second half is a condition on the state tables, met by the oracle alone: two consecutive states that show different
things have different oracle frames, so a renderer that handed back the previous frame, or rendered from a stale
descriptor, cannot pass against the twin AND the oracle.  A pair that fails it is a reason to change a table (move a
camera or a light), never to loosen the check."""
import numpy as np
import pytest

import frame_sequences as fs
from frame_sequences import AXES, GRIDS, PAIRS, SCRIPTED, SEEDS, axis_value, content_key, sequence, spans


def _transitions():
    for seed in SEEDS:
        states = sequence(seed)
        for a, b in zip(states, states[1:]):
            yield seed, a, b


def test_every_ordered_pair_of_every_axis_is_a_transition():
    assert len(PAIRS) == 12 + 6 + 6 + 6 + 2 + 2 + 2
    seen = {(axis, axis_value(a, axis), axis_value(b, axis)) for _, a, b in _transitions() for axis in AXES}
    missing = [p for p in PAIRS if p not in seen]
    assert not missing, missing


def test_every_state_is_one_the_library_accepts():
    for seed in SEEDS:
        for i, s in enumerate(sequence(seed)):
            assert fs.legal(s), (seed, i, s)
            kind = s.part[0]
            assert not (s.lights > 1 and (kind == "stripe" or s.face_status)), (seed, i)        # validate_frame, _prepare
            assert not (s.overlay and kind != "whole"), (seed, i)                                # mr_render
            assert not (s.face_status and kind != "whole"), (seed, i)                            # mr_read_face_status, _prepare
            assert not (s.supersample > 1 and kind == "stripe"), (seed, i)
            if kind == "band":                     # a supersampled band: sample rows that are multiples of s
                r0, r1 = fs.band_rows(s)
                assert 0 <= r0 < r1 <= GRIDS[s.grid][0]
            assert s.camera != fs.EMPTY or (0 < i < len(sequence(seed)) - 1), "the empty camera stands between two frames"
    lengths = [len(sequence(seed)) for seed in SEEDS]
    print("frames per seed:", lengths)
    assert all(36 <= n <= 48 for n in lengths), lengths


def test_every_seed_visits_every_grid_and_part_and_is_deterministic():
    for seed in SEEDS:
        states = sequence(seed)
        assert {s.grid for s in states} == set(range(len(GRIDS))), seed
        assert {s.part[0] for s in states} == set(fs.PART_KINDS), seed
        assert len({s.part for s in states if s.part[0] == "band"}) >= 2, seed
        fs._BUILT.pop(seed)
        assert sequence(seed) == states, seed
    bands = {s.part for seed in SEEDS for s in sequence(seed) if s.part[0] == "band"}
    stripes = {s.part for seed in SEEDS for s in sequence(seed) if s.part[0] == "stripe"}
    assert len(bands) >= 2 and len(stripes) >= 2
    assert {s.camera for seed in SEEDS for s in sequence(seed)} == {0, 1, 2}
    assert {s.pose for seed in SEEDS for s in sequence(seed)} == set(range(fs.N_POSES))
    assert {s.lane for seed in SEEDS for s in sequence(seed)} == {None, 0, 1, 2, 3}
    assert any(s.face_status for seed in SEEDS for s in sequence(seed))
    assert {s.light_at for seed in SEEDS for s in sequence(seed)} == {0, 1}


def _only(a, b, *axes):
    """The two states differ in *axes* and in nothing else."""
    fields = [f for f in a._fields if getattr(a, f) != getattr(b, f)]
    return sorted(fields) == sorted(axes)


@pytest.mark.parametrize("seed", SEEDS)
def test_every_seed_holds_the_scripted_transitions(seed):
    states, where = sequence(seed), spans(seed)
    assert set(where) == set(SCRIPTED)
    tiles = lambda s: -(-GRIDS[s.grid][0] * s.supersample // 16) * -(-GRIDS[s.grid][1] * s.supersample // 16)
    part = lambda name: states[where[name][0]:where[name][1]]

    a, b, c = part("grid_flip")
    assert (a.grid, b.grid, c.grid) == (0, 1, 0) and _only(a, b, "grid") and a == c and tiles(a) == tiles(b)

    a, b, c = part("band_whole_band")
    assert a.part[0] == c.part[0] == "band" and a.part[2] == c.part[2] == 3 and a.part != c.part and b.part == fs.WHOLE
    assert _only(a, b, "part") and _only(b, c, "part")

    a, b = part("stripe_whole")
    assert a.part[0] == "stripe" and b.part == fs.WHOLE and _only(a, b, "part")

    a, b, c = part("counted_frame_counted")
    assert (a.mode, b.mode, c.mode) == ("counted", "frame", "counted") and a.lane is b.lane is c.lane is None
    assert a == c and _only(a, b, *(("mode", "face_status") if a.face_status else ("mode",)))

    a, b, c, d = part("split_history")
    assert a == b == d and _only(b, c, "lights") and (a.lights, c.lights) == (1, 4)
    assert a.camera == fs.HEAVY and a.shadows and a.part == fs.WHOLE and a.supersample == 1 and tiles(a) == 90 and a.lane is None

    a, b, c = part("overflow")
    assert (a.event, b.event, c.event) == ("", "squeeze", "") and _only(a, b, "event") and _only(a, c, "grid")
    assert b.part == fs.WHOLE and b.lane is None and b.camera == fs.HEAVY and b.shadows
    assert sum(s.event == "squeeze" for s in states) == 1

    a, b, c = part("empty_between_heavy")
    assert (a.camera, b.camera, c.camera) == (fs.HEAVY, fs.EMPTY, fs.HEAVY) and a == c and _only(a, b, "camera")

    lanes = part("lanes")
    assert [s.lane for s in lanes] == [0, 1, 2, 0, None]
    assert all(s.mode == "frame" and s.part == fs.WHOLE for s in lanes)
    assert all(_only(x, y, "lane", "camera") or _only(x, y, "lane") for x, y in zip(lanes, lanes[1:]))

    a, b, c, d, e = part("light_moves_under_a_warm_cache")
    assert a == b == c == e and _only(c, d, "light_at") and a.lights == 1 and a.shadows and a.lane is None

    assert sum(x.bones != y.bones for x, y in zip(states, states[1:])) == 1, "one change of bones"
    assert sum(x.edited != y.edited for x, y in zip(states, states[1:])) == 1 and not states[0].edited and states[-1].edited


def test_rows_of_the_parts():
    """Bands of three tile every grid at rows that are no multiple of 16; the stripes of a split tile it too; the
    rows of a striped result are the layout multigpu.unstripe_index describes."""
    from py_numpy_renderer_amd.multigpu import stripe_rows, unstripe_index
    for grid, (h, _) in enumerate(GRIDS):
        base = fs.BASE._replace(grid=grid)
        cover = sum(fs.own_rows(base._replace(part=p)).astype(int) for p in fs.BANDS)
        assert (cover == 1).all()
        if h % 48:                                 # (144 rows are nine tile rows: its bands are cut between tiles)
            assert any(fs.band_rows(base._replace(part=p))[1] % 16 for p in fs.BANDS[:2])
        for count in (2, 3):
            index = unstripe_index(h, count).numpy()
            per = stripe_rows(h, count)
            cover = np.zeros(h, int)
            for rank in range(count):
                s = base._replace(part=("stripe", rank, count))
                own = fs.own_rows(s)
                cover += own
                assert np.array_equal(fs.out_rows(s), index[own[::-1]] - rank * per)
            assert (cover == 1).all()
        for s in (1, 2, 4):
            assert fs.tap_rows(base._replace(supersample=s)).shape == (s * h,)


@pytest.fixture(scope="module")
def frames(api, oracle_mod):
    """The oracle's uint8 frame of a state's whole frame; every distinct one of the six sequences rendered once."""
    done = fs.expected_many(api, oracle_mod, [s for seed in SEEDS for s in sequence(seed)], keep=lambda ref: ref.out)
    return lambda state: done[content_key(state)]


def test_the_oracle_tells_consecutive_frames_apart(frames):
    """Consecutive states that show different things: different oracle frames (after compose and resolve).  States
    that show the same and differ in their part: different rows.  (Those that differ in nothing but the mode, the
    lane, the face status or the squeezed lists render the same rows of the same frame: there is nothing to tell.)"""
    fewest, n_content, n_part = None, 0, 0
    for seed, a, b in _transitions():
        if content_key(a) != content_key(b):
            fa, fb = frames(a), frames(b)
            n_content += 1
            if fa.shape != fb.shape:
                continue
            differ = int((fa != fb).any(axis=-1).sum())
            fewest = differ if fewest is None else min(fewest, differ)
            assert differ >= 16, (seed, differ, a, b)
        elif a.part != b.part:
            n_part += 1
            assert not np.array_equal(fs.own_rows(a), fs.own_rows(b)), (seed, a, b)
    print(f"{n_content} transitions change the frame (fewest pixels that differ: {fewest}), {n_part} only the part")
    assert n_content >= 100 and n_part >= 12


def test_the_empty_camera_shows_nothing_and_the_others_show_the_mesh(frames, api, oracle_mod):
    for camera in (fs.HEAVY, fs.GRAZING, fs.EMPTY):
        ref = fs.expected(api, oracle_mod, fs.BASE._replace(camera=camera))
        covered = int((ref.winner >= 0).sum())
        mesh = int(((ref.winner >= 0) & (ref.winner < len(fs._template(api)["models"][0]._faces))).sum())
        print(f"camera {camera}: {covered} covered pixels, {mesh} of the mesh, {ref.per[0].stats['n_quads']} shadow quads")
        assert (covered == 0) if camera == fs.EMPTY else (mesh >= 500)
