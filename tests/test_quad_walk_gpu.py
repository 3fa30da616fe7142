"""GPU: phase 3 of ``k_tile`` (kernels_tile.h) under ``MR_QUAD_WALK=auto | strips | spans``, on small scenes.

``strips`` walks a tile's shadow quads one at a time, every lane of a wavefront testing its own pixel of the wavefront's
16x4 strip; ``spans`` deals (quad, row) items to the lanes, sixteen quads to a round, finds each row's span by bisection
with the strip walk's own rounded edge expression and adds to the pixels' stencil words in LDS; ``auto`` chooses per
(quad, strip).  The three must be indistinguishable: z, winner and stencil bit-exact and the counters equal to the
committed captures in counted frames, the uint8 frames byte-identical to each other in frame-only ones.

The variable is read once per process, so a child process per value renders and saves (the pattern of
test_edge_spread_gpu.py); ``MR_TILE_SPLIT=1``, read once too, gets a second child per value.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import scenes
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SCENES = ["cube_small", "torus_spot", "dense_tile_s0", "fins_nonmanifold", "diablo_floor_lh_gl", "tetra_ortho",
          "soup_behind_camera_s0", "cube_tetra_nodepth"]
VARIANTS = "diablo_floor_small"          # also supersampled, as row bands, as stripes and with split tiles
MODES = ["auto", "strips", "spans"]
COUNTERS = ("frag_quad", "stencil_updates", "covered_px", "lit_px")

CHILD = r'''
import os, sys
ROOT, OUT, WHAT = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import scenes
COUNTERS = sys.argv[4].split(",")
api = scenes.product_api()

def counted(backend, scene, tag, save):
    save[tag + "out"] = backend.render(scene, shadows=True, keep_float=True).copy()
    save[tag + "z"] = backend.read_z()
    save[tag + "winner"] = backend.read_winner()
    save[tag + "stencil"] = backend.read_stencil()
    save[tag + "counters"] = np.array([backend.last_stats[c] for c in COUNTERS], dtype=np.int64)
    save[tag + "walks"] = np.array(backend.quad_walks(), dtype=np.int64)

if WHAT == "split":                      # MR_TILE_SPLIT=1: the parts of a heavy tile share its quads from the second frame on
    scene = scenes.build(api, sys.argv[5])
    backend = scene._backend()
    for _ in range(3):
        frame = backend.render(scene, counters=False).copy()
    np.savez(os.path.join(OUT, "split.npz"), frame=frame)
    scene.close()
    print("ok split")
    sys.exit(0)

for name in sys.argv[5:]:
    save = {}
    scene = scenes.build(api, name)
    backend = scene._backend()
    counted(backend, scene, "c_", save)
    save["frame"] = backend.render(scene, counters=False).copy()
    scene.close()
    if name == sys.argv[-1]:             # the variants' scene comes last
        scene = scenes.build(api, name)
        backend = scene._backend()
        h = scene.render().shape[0]
        cuts = [round(i * h / 3) for i in range(4)]
        save["bands"] = np.concatenate([backend.render(scene, counters=False, row_band=(cuts[i], cuts[i + 1])) for i in range(3)])
        save["stripes"] = np.concatenate([backend.render(scene, counters=False, stripe=(r, 3)) for r in range(3)])
        scene.supersample = 2
        save["ss2"] = backend.render(scene, counters=False).copy()
        counted(backend, scene, "ss2_", save)
        scene.close()
    np.savez(os.path.join(OUT, name + ".npz"), **save)
    print("ok", name)
'''


@pytest.fixture(scope="module")
def expected(api, oracle_mod):
    """Per scene, computed once and left alone: the committed capture, the oracle's stencil updates (the one counter
    the captures do not record) and the oracle's uint8 frame (soup_behind_camera_s0's capture shows the background where
    a face with corners behind the camera plane won the pixel, see test_oracle_golden.py: its frame is compared with
    the oracle's, every other scene's with both)."""
    want = {}
    for name in SCENES + [VARIANTS]:
        scene = scenes.build(api, name)
        r = oracle_mod.render(scene)
        want[name] = dict(golden=load_golden(name), updates=int(r.stats["stencil_updates"]), oracle_out=r.out)
        scene.close()
    return want


@pytest.fixture(scope="module")
def rendered(tmp_path_factory):
    """(mode, what) -> directory of the child's .npz files; one child per mode, and one more per mode for the split."""
    done = {}

    def run(mode, what="scenes"):
        if (mode, what) not in done:
            out = tmp_path_factory.mktemp(f"walk_{mode}_{what}")
            script = out / "child.py"
            script.write_text(CHILD)
            env = dict(os.environ, MR_QUAD_WALK=mode)
            env.pop("MR_TILE_SPLIT", None)
            names = SCENES + [VARIANTS]
            if what == "split":
                env["MR_TILE_SPLIT"] = "1"
                names = [VARIANTS]
            got = subprocess.run([sys.executable, str(script), ROOT, str(out), what, ",".join(COUNTERS)] + names, env=env,
                                 capture_output=True, text=True, timeout=300)
            assert got.returncode == 0, got.stdout[-2000:] + got.stderr[-3000:]
            assert got.stdout.count("ok ") == (1 if what == "split" else len(names)), got.stdout
            done[(mode, what)] = out
        return done[(mode, what)]
    return run


def test_the_reference_makes_the_cases_count(expected):
    """What keeps the comparisons below from passing vacuously, from the reference alone: every scene draws shadow-quad
    fragments and ends with a non-zero stencil somewhere."""
    for name in SCENES + [VARIANTS]:
        g, meta = expected[name]["golden"]
        print(f"{name}: {meta['counts']['n_quads']} quads, {meta['counts']['frag_quad']} quad fragments, "
              f"{int((g['stencil'] != 0).sum())} px with a stencil count, {expected[name]['updates']} stencil updates")
        assert meta["counts"]["frag_quad"] > 0 and (g["stencil"] != 0).any() and expected[name]["updates"] > 0, name


@pytest.mark.parametrize("name", SCENES + [VARIANTS])
@pytest.mark.parametrize("mode", MODES)
def test_counted_frames_match_the_captures(expected, rendered, mode, name):
    got = np.load(os.path.join(rendered(mode), name + ".npz"))
    g, meta = expected[name]["golden"]
    label = f"{mode} {name}"
    assert np.array_equal(got["c_z"].view(np.uint64), g["z"].view(np.uint64)), f"{label}: z"
    assert np.array_equal(got["c_winner"], g["winner"]), f"{label}: winner"
    assert np.array_equal(got["c_stencil"], g["stencil"]), f"{label}: stencil"
    covered = g["winner"] >= 0
    want = dict(frag_quad=meta["counts"]["frag_quad"], stencil_updates=expected[name]["updates"],
                covered_px=int(covered.sum()), lit_px=int((covered & (g["stencil"] == 0)).sum()))
    counters = dict(zip(COUNTERS, got["c_counters"].tolist()))
    print(f"{label}: {counters}, walks (items, strips, of them polygons > 4, non-finite) {got['c_walks'].tolist()}")
    assert counters == want, f"{label}: counters, expected {want}"
    for ref, what in ((expected[name]["oracle_out"], "oracle"), (g["out"], "capture")):
        if what == "capture" and name in scenes.BEHIND_CAMERA:
            continue
        worst = int(np.abs(got["c_out"].astype(np.int16) - ref.astype(np.int16)).max())
        assert worst <= 1, f"{label}: uint8 off by {worst} from the {what}"


@pytest.mark.parametrize("name", SCENES + [VARIANTS])
def test_frame_only_frames_are_the_same_bytes(rendered, name):
    frames = {mode: np.load(os.path.join(rendered(mode), name + ".npz"))["frame"] for mode in MODES}
    for mode in MODES[1:]:
        assert np.array_equal(frames[mode], frames[MODES[0]]), f"{name}: {mode} differs from {MODES[0]}"


@pytest.mark.parametrize("what", ["ss2", "bands", "stripes", "split"])
def test_variants_are_the_same_bytes(rendered, what):
    """diablo_floor_small supersampled, as three row bands, as three stripes and with its heavy tiles' quads shared out."""
    def frame(mode):
        if what == "split":
            return np.load(os.path.join(rendered(mode, "split"), "split.npz"))["frame"]
        return np.load(os.path.join(rendered(mode), VARIANTS + ".npz"))[what]
    first = frame(MODES[0])
    assert first.size and first.max() > first.min()
    for mode in MODES[1:]:
        assert np.array_equal(frame(mode), first), f"{what}: {mode} differs from {MODES[0]}"
    plain = np.load(os.path.join(rendered(MODES[0]), VARIANTS + ".npz"))["frame"]
    if what in ("bands", "split"):
        assert np.array_equal(first, plain), f"{what}: differs from the whole frame"
    if what == "ss2":                    # the sample grid's z, winner and stencil: the same in every mode
        for key in ("ss2_z", "ss2_winner", "ss2_stencil", "ss2_counters"):
            a = np.load(os.path.join(rendered(MODES[0]), VARIANTS + ".npz"))[key]
            for mode in MODES[1:]:
                b = np.load(os.path.join(rendered(mode), VARIANTS + ".npz"))[key]
                assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                      b.view(np.uint64) if b.dtype == np.float64 else b), f"{key}: {mode}"


def test_every_walk_is_reached(rendered):
    """``mr_debug_quad_walks`` of the counted frames: strips walks no item, spans walks strips only where the span walk is
    not defined, auto uses both on diablo_floor_small."""
    walks = {mode: {name: np.load(os.path.join(rendered(mode), name + ".npz"))["c_walks"].tolist()
                    for name in SCENES + [VARIANTS]} for mode in MODES}
    polygons = 0
    for name in SCENES + [VARIANTS]:
        for mode in MODES:
            items, strips, poly, wild = walks[mode][name]
            print(f"{name} {mode}: {items} (quad, row) items, {strips} (quad, strip) walks, of them {poly} of polygons with "
                  f"more than four vertices and {wild} with a non-finite edge value")
            assert items + strips > 0, f"{name} {mode}: no quad walked"
        assert walks["strips"][name][0] == 0, f"{name}: strips walked items"
        items, strips, poly, wild = walks["spans"][name]
        assert items > 0 and strips <= poly + wild, f"{name}: spans walked {strips} strips, {poly} + {wild} excluded"
        assert walks["strips"][name][2:] == walks["spans"][name][2:], f"{name}: the excluded kinds differ between modes"
        polygons += walks["strips"][name][2]
    print(f"(quad, strip) walks of polygons with more than four vertices, all scenes: {polygons}")
    items, strips, _, _ = walks["auto"][VARIANTS]
    assert items > 0 and strips > 0, f"auto on {VARIANTS}: {items} items, {strips} strips"
