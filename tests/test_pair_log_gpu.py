"""GPU: the winners' sweep of ``k_tile``'s small pairs (kernels_tile.h, phase 2) under ``MR_PAIR_LOG`` = 0, 1, 2 and the
default.

The first sweep over a tile's small (triangle, tile) pairs leaves every covered sample's z key, pixel and face in the
lane's log; the winners' sweep answers from the log and walks again only from the first sample that did not fit.  The
capacity changes where the keys come from, never a bit of the result: counted frames equal the committed captures (z,
winner map, stencil and fragment counts exact, float frame 2e-6, uint8 +-1), frame-only frames are the same bytes for
every capacity and the same as the general kernel's, and generated tiles whose list length sits on either side of every
threshold of the dealing rule (8 / 4 / 2 lanes per pair at 32 / 64, a second round at 128, a third at 256) equal the
sequential C oracle (test_pair_log_cpu.py holds the generator to what it was made for).  ``mr_debug_pair_log`` shows
that both paths ran.

The variable is read once per process: a child process per value renders and saves (the pattern of
test_quad_walk_gpu.py); ``MR_TILE_SPLIT=1``, read once too, gets a second child per value.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import scenes
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SCENES = ["dense_tile_s0", "soup_s0", "welded_s0", "fins_nonmanifold", "cube_tetra_nodepth", "diablo_floor_lh_gl",
          "torus_spot", "diablo_small"]
VARIANTS = "torus_spot"                   # also supersampled and as row bands whose edges cut through pixel boxes
SPLIT = "diablo_floor_small"              # with MR_TILE_SPLIT=1 its heavy tiles' quads are shared out
CAPS = ["0", "1", "2", "default"]
LENGTHS = [32, 33, 64, 65, 128, 129, 257]
GEN_CAPS = ["default", "1"]
LOG_K = 4                                 # PAIR_LOG_K, the default capacity
SMALL_LEN = 5                             # column of a tile record: the length of the tile's list of small pairs
GEN_RESOLUTION = (128, 160)
GEN_TILE = (4, 4)                         # the tile of pixels 64..79 x 64..79

# ---- generated tiles: N tiny faces inside one 16 x 16 tile, in front of one face over the whole frame
_EYE = np.array([0.5, 1.0, 2.0])
_FWD = -_EYE / np.linalg.norm(_EYE)
_RIGHT = np.cross(_FWD, [0.0, 1.0, 0.0]) / np.linalg.norm(np.cross(_FWD, [0.0, 1.0, 0.0]))
_UP = np.cross(_RIGHT, _FWD)
_PX = 2 * math.tan(math.radians(30)) / GEN_RESOLUTION[0]


def _at(px, py, d):
    """World point the standard camera sees at the sample of pixel (px, py) of the 128 x 160 frame, *d* in front of it
    (scenes._at for this resolution)."""
    h, w = GEN_RESOLUTION
    return _EYE + d * (_FWD + (px - w / 2) * _PX * _RIGHT + (py - h / 2) * _PX * _UP)


def pair_log_obj(n):
    """*n* faces whose pixel boxes lie inside the tile of pixels 64..79 x 64..79, every one around the sample of a
    pixel so that it covers it (it is then listed, and the list is *n* long), facing the camera, of three kinds: dots of
    1 to 3 pixels; wedges 4 to 11 pixels wide and 1 to 5 rows high (a box of at most 24 samples), which give a lane
    several covered samples inside one pair; and exact repeats of earlier faces, which tie to the bit.  Depths are drawn from one narrow range, so the faces
    fight for the pixels they share.  Behind them one face over the whole frame (a big pair in every tile)."""
    rng = np.random.default_rng(20261101 + n)
    obj = scenes._ObjWriter(rng)
    made, wedges = [], 0
    for i in range(n):
        d = rng.uniform(2.38, 2.5)
        if i % 8 == 7:                                    # a repeat: the same three points again
            made.append(made[int(rng.integers(0, len(made)))])
            obj.triangle(*made[-1])
            continue
        if i % 8 in (2, 5):                               # a wedge, apex up: rows cy .. cy + rows - 1 of the box
            cx, cy = int(rng.integers(70, 74)), int(rng.integers(65, 74))
            # (left, right, top, apex): the box is ceil(cx - left) .. ceil(cx + right) wide and ceil(cy + top) - cy rows high.
            # The first three are 8 x 3, 4 x 4 and 4 x 5 samples with a whole column covered: the lane that owns the column
            # covers 3 samples where 8 lanes share the pair, 4 and 5 where 4 do.
            left, right, top, apex = ((3.6, 4.4, 2.4, 0.4), (1.6, 2.4, 3.4, 0.1), (1.6, 2.4, 4.4, 0.05), (3.4, 3.4, 1.4, None),
                                      (3.4, 3.4, 2.4, None), (2.4, 2.4, 2.4, None), (5.4, 5.4, 1.4, None), (4.4, 4.4, 1.9, None),
                                      (2.4, 2.4, 3.4, None), (5.4, 5.4, 0.9, None))[wedges % 10]      # each in turn
            wedges += 1
            apex = rng.uniform(-0.2, 0.2) if apex is None else apex
            pts = [_at(cx - left, cy - 0.4, d), _at(cx + right, cy - 0.4, d), _at(cx + apex, cy + top, d)]
        else:                                             # a dot around the sample of (cx, cy)
            cx, cy = int(rng.integers(66, 78)), int(rng.integers(66, 78))
            r = rng.uniform(1.0, 1.6)
            ang = np.radians(np.array([0.0, 120.0, 240.0]) + rng.uniform(0, 360) + rng.uniform(-15, 15, 3))
            pts = [_at(cx + r * math.cos(t), cy + r * math.sin(t), d) for t in np.sort(ang)]
        obj.triangle(*pts)
        made.append(pts)
    a, b, c = _at(-200, -40, 5.0), _at(360, -40, 5.0), _at(80, 330, 5.0)
    obj.triangle(a, b, c)
    return scenes._write_if_changed(os.path.join(scenes.GENERATED, f"pair_log_{n}.obj"), obj.text())


def pair_log_scene(api, n):
    return scenes._adversarial(api, pair_log_obj(n), "std", GEN_RESOLUTION)


CHILD = r'''
import os, sys
ROOT, OUT, WHAT = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import scenes

api = scenes.product_api()

def counted(backend, scene, tag, save):
    save[tag + "out"] = backend.render(scene, shadows=True, keep_float=True).copy()
    save[tag + "frame"] = backend.read_frame_f32()
    save[tag + "z"] = backend.read_z()
    save[tag + "winner"] = backend.read_winner()
    save[tag + "stencil"] = backend.read_stencil()
    save[tag + "frags"] = np.array([backend.last_stats["frag_tri"], backend.last_stats["frag_quad"]], dtype=np.int64)
    save[tag + "log"] = np.array(backend.pair_log(), dtype=np.int64)
    save[tag + "records"] = backend.read_tile_records().astype(np.int64)

def frame_only(backend, scene, tag, save):
    save[tag] = backend.render(scene, counters=False).copy()
    assert not backend.frame_path()["full"]
    backend.force_full(True)
    save[tag + "_full"] = backend.render(scene, counters=False).copy()
    assert backend.frame_path()["full"]
    backend.force_full(False)

if WHAT == "split":
    scene = scenes.build(api, sys.argv[4])
    backend = scene._backend()
    for _ in range(3):
        frame = backend.render(scene, counters=False).copy()
    np.savez(os.path.join(OUT, "split.npz"), frame=frame, split=int(backend.frame_path()["split"]))
    scene.close()
    print("ok split")
    sys.exit(0)

if WHAT == "generated":
    import test_pair_log_gpu as T
    for n in T.LENGTHS:
        save = {}
        scene = T.pair_log_scene(api, n)
        backend = scene._backend()
        counted(backend, scene, "c_", save)
        scene.close()
        np.savez(os.path.join(OUT, "gen_%d.npz" % n), **save)
        print("ok", n)
    sys.exit(0)

for name in sys.argv[4:]:
    save = {}
    scene = scenes.build(api, name)
    backend = scene._backend()
    counted(backend, scene, "c_", save)
    nodepth = any(not getattr(m, "depth_test", True) for m in scene.models)
    if nodepth:                              # the scene takes the general kernel whatever is asked
        save["frame"] = save["frame_full"] = backend.render(scene, counters=False).copy()
    else:
        frame_only(backend, scene, "frame", save)
    scene.close()
    if name == sys.argv[-1]:                 # the variants' scene comes last
        scene = scenes.build(api, name)
        backend = scene._backend()
        h = scene.render().shape[0]
        cuts = [0, 37, 101, h]               # no multiple of the tile: the bands' edges cut through tiles and pixel boxes
        save["bands"] = np.concatenate([backend.render(scene, counters=False, row_band=(cuts[i], cuts[i + 1])) for i in range(3)])
        scene.supersample = 2
        frame_only(backend, scene, "ss2", save)
        scene.close()
    np.savez(os.path.join(OUT, name + ".npz"), **save)
    print("ok", name)
'''


@pytest.fixture(scope="module")
def expected(api, oracle_mod):
    """Computed once and left alone: the committed capture of every scene, and the oracle's z and winners of the
    generated tiles."""
    want = {name: load_golden(name) for name in SCENES}
    for n in LENGTHS:
        scene = pair_log_scene(api, n)
        r = oracle_mod.render(scene)
        want[n] = dict(z=r.z, winner=r.winner)
        scene.close()
    return want


@pytest.fixture(scope="module")
def rendered(tmp_path_factory):
    """(capacity, what) -> directory of the child's .npz files."""
    done = {}

    def run(cap, what="scenes"):
        if (cap, what) not in done:
            out = tmp_path_factory.mktemp(f"pair_log_{cap}_{what}")
            script = out / "child.py"
            script.write_text(CHILD)
            env = dict(os.environ)
            env.pop("MR_TILE_SPLIT", None)
            env.pop("MR_PAIR_LOG", None)
            if cap != "default":
                env["MR_PAIR_LOG"] = cap
            names = [n for n in SCENES if n != VARIANTS] + [VARIANTS] if what == "scenes" else [SPLIT] if what == "split" else []
            if what == "split":
                env["MR_TILE_SPLIT"] = "1"
            got = subprocess.run([sys.executable, str(script), ROOT, str(out), what] + names, env=env,
                                 capture_output=True, text=True, timeout=300)
            assert got.returncode == 0, got.stdout[-2000:] + got.stderr[-3000:]
            want_ok = {"scenes": len(names), "split": 1, "generated": len(LENGTHS)}[what]
            assert got.stdout.count("ok ") == want_ok, got.stdout
            done[(cap, what)] = out
        return done[(cap, what)]
    return run


def _load(rendered, cap, name):
    return np.load(os.path.join(rendered(cap), name + ".npz"))


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("cap", CAPS)
def test_counted_frames_match_the_captures(expected, rendered, cap, name):
    got = _load(rendered, cap, name)
    g, meta = expected[name]
    label = f"MR_PAIR_LOG={cap} {name}"
    assert np.array_equal(got["c_z"].view(np.uint64), g["z"].view(np.uint64)), f"{label}: z"
    assert np.array_equal(got["c_winner"], g["winner"]), f"{label}: winner"
    assert np.array_equal(got["c_stencil"], g["stencil"]), f"{label}: stencil"
    assert got["c_frags"].tolist() == [meta["counts"]["frag_tri_pass1"], meta["counts"]["frag_quad"]], f"{label}: fragment counts"
    err = np.abs(got["c_frame"].astype(np.float64) - g["frame"].astype(np.float64)).max()
    worst = int(np.abs(got["c_out"].astype(np.int16) - g["out"].astype(np.int16)).max())
    print(f"{label}: float frame off by {err:.3g}, uint8 by {worst}; log {got['c_log'].tolist()}")
    assert err <= 2e-6, f"{label}: float frame off by {err:.3g}"
    assert worst <= 1, f"{label}: uint8 off by {worst}"


@pytest.mark.parametrize("name", SCENES)
def test_frame_only_frames_are_the_same_bytes(rendered, name):
    first = _load(rendered, CAPS[0], name)["frame"]
    assert first.size and first.max() > first.min()
    for cap in CAPS:
        got = _load(rendered, cap, name)
        assert np.array_equal(got["frame"], first), f"{name}: MR_PAIR_LOG={cap} differs from {CAPS[0]}"
        assert np.array_equal(got["frame_full"], first), f"{name}: the general kernel's frame differs, MR_PAIR_LOG={cap}"


@pytest.mark.parametrize("what", ["ss2", "bands", "split"])
def test_variants_are_the_same_bytes(rendered, what):
    """torus_spot supersampled and as three row bands cut at rows 37 and 101; diablo_floor_small with its heavy tiles'
    quads shared out."""
    def frame(cap, key=what):
        if what == "split":
            got = np.load(os.path.join(rendered(cap, "split"), "split.npz"))
            assert int(got["split"]) == 1, "the frame did not take the kernel that shares heavy tiles out"
            return got["frame"]
        return _load(rendered, cap, VARIANTS)[key]
    first = frame(CAPS[0])
    assert first.size and first.max() > first.min()
    for cap in CAPS[1:]:
        assert np.array_equal(frame(cap), first), f"{what}: MR_PAIR_LOG={cap} differs from {CAPS[0]}"
    if what == "ss2":
        for cap in CAPS:
            assert np.array_equal(frame(cap, "ss2_full"), first), f"ss2: the general kernel's frame differs, MR_PAIR_LOG={cap}"
    if what == "bands":
        assert np.array_equal(first, _load(rendered, CAPS[0], VARIANTS)["frame"]), "bands: differ from the whole frame"


def test_both_paths_are_reached(rendered):
    """``mr_debug_pair_log`` of the counted frames: (covered samples answered from the log, samples walked again)."""
    logs = {cap: {name: _load(rendered, cap, name)["c_log"].tolist() for name in SCENES} for cap in CAPS}
    for name in SCENES:
        small = int(_load(rendered, "default", name)["c_records"][:, SMALL_LEN].sum())
        print(f"{name}: {small} small pairs; (from the log, walked again) by capacity: " +
              ", ".join(f"{cap}: {tuple(logs[cap][name])}" for cap in CAPS))
        assert logs["0"][name][0] == 0, f"{name}: capacity 0 answered {logs['0'][name][0]} entries from the log"
        if small:
            assert logs["0"][name][1] > 0, f"{name}: capacity 0 walked nothing again"
            assert logs["default"][name][0] > 0, f"{name}: nothing answered from the log at the default capacity"
        answered = [logs[cap][name][0] for cap in CAPS]
        again = [logs[cap][name][1] for cap in CAPS]
        assert answered == sorted(answered) and again == sorted(again, reverse=True), f"{name}: not monotonic in the capacity"
    for name in ("dense_tile_s0", "torus_spot"):
        assert min(logs["1"][name]) > 0, f"{name}: capacity 1 gave {logs['1'][name]}"
    nodepth = logs["default"]["cube_tetra_nodepth"]
    print(f"cube_tetra_nodepth at the default capacity: {nodepth}")


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("cap", GEN_CAPS)
def test_generated_tiles_match_the_oracle(expected, rendered, cap, n):
    got = np.load(os.path.join(rendered(cap, "generated"), f"gen_{n}.npz"))
    want = expected[n]
    label = f"MR_PAIR_LOG={cap}, {n} pairs"
    longest = int(got["c_records"][:, SMALL_LEN].max())
    print(f"{label}: longest list of small pairs {longest}; log {got['c_log'].tolist()}")
    assert longest == n, f"{label}: the tile lists {longest} small pairs"
    assert np.array_equal(got["c_z"].view(np.uint64), want["z"].view(np.uint64)), f"{label}: z"
    assert np.array_equal(got["c_winner"], want["winner"]), f"{label}: winner"
    assert got["c_log"][0] > 0, f"{label}: nothing answered from the log"
    if cap == "1" or n > 32:
        assert got["c_log"][1] > 0, f"{label}: nothing walked again"


def test_a_list_runs_to_a_third_round(rendered):
    """dense_tile_s0's longest list of small pairs stays inside two rounds (2 lanes per pair: 128 pairs a round); the
    generated tile of 257 is the one whose lanes log across three rounds.  It is held to the oracle above."""
    dense = int(_load(rendered, "default", "dense_tile_s0")["c_records"][:, SMALL_LEN].max())
    third = int(np.load(os.path.join(rendered("default", "generated"), "gen_257.npz"))["c_records"][:, SMALL_LEN].max())
    print(f"longest list of small pairs: dense_tile_s0 {dense}, the generated tile {third}")
    assert max(dense, third) > 256
