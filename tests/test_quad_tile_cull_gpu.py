"""GPU: ``MR_QUAD_TILE_CULL=0 | 1`` -- ``k_tile``'s frame-only single-light kernels stage and classify every shadow quad a
tile lists, or only those that pass ``k_bin_work``'s bound against the tile's most favourable covered z
(``quad_tile_bound`` / ``quad_tile_none``, csrc/quad_reject.h; test_quad_tile_cull_cpu.py holds the rule itself to the
strip rule and to the per-sample rule).  A dropped quad would have been rejected by the strip rule in all four
wavefronts or -- in the frames of a right-handed camera, whose depths are negative and whose quads the strip rule keeps --
fails the depth test at every sample of the tile, so the two settings must be indistinguishable: the uint8 frame, z and
winner equal byte for byte and the stencil equal wherever a triangle was drawn (the frame-only contract).  ``count0`` / ``count`` are off / on with the
number of quads a tile staged in word 8 of its record: never more than it lists, and in every single-light scene some
tile that draws a triangle stages fewer.  Counted frames (the general kernels, behind the same ``k_bin_work``) keep every
counter.

The variable is looked up for every frame, so one process renders both; ``MR_TILE_SPLIT=1`` is read once per process and
gets a child.  Small scenes only: cube_small, torus_spot, diablo_floor_small, diablo_floor_lh_gl (left-handed, hundreds
of quads in a tile: several batches), and torus_spot / diablo_floor_small supersampled, as a row band, as a stripe and
under two lights.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SWITCH = "MR_QUAD_TILE_CULL"
SCENES = ["cube_small", "torus_spot", "diablo_floor_small", "diablo_floor_lh_gl"]
VARIANTS = ["ss2", "band", "stripe"]
QUAD_LEN, KEPT = 7, 8                     # columns of a tile record: the length of the quad list, the quads staged


def _frame_only(backend, scene, value, **kw):
    os.environ[SWITCH] = value
    out = backend.render(scene, shadows=True, counters=False, keep_buffers=True, **kw).copy()
    assert backend.frame_path()["full"] is False
    return dict(out=out, z=backend.read_z().view(np.uint64).copy(), winner=backend.read_winner().copy(),
                stencil=backend.read_stencil().copy(), records=backend.read_tile_records().astype(np.int64))


def _counted(backend, scene, value, **kw):
    os.environ[SWITCH] = value
    out = backend.render(scene, shadows=True, counters=True, **kw).copy()
    stats = {k: v for k, v in backend.last_stats.items() if not k.startswith("gpu_ms")}
    return dict(out=out, z=backend.read_z().view(np.uint64).copy(), winner=backend.read_winner().copy(),
                stencil=backend.read_stencil().copy()), stats


def _same_frames(label, off, on):
    assert off["out"].size and off["out"].max() > off["out"].min(), f"{label}: an empty frame"
    for key in ("out", "z", "winner"):
        assert np.array_equal(off[key], on[key]), f"{label}: {key} differs"
    drawn = off["winner"] >= 0
    assert drawn.any(), label
    assert np.array_equal(off["stencil"][drawn], on["stencil"][drawn]), f"{label}: the stencil differs where a triangle was drawn"


def _kept(label, off, on, single_light=True):
    """Word 8 of the records.  Off: a tile that walks its quads stages all it lists (and one that draws no triangle none)."""
    listed, kept_off, kept_on = off["records"][:, QUAD_LEN], off["records"][:, KEPT], on["records"][:, KEPT]
    assert np.array_equal(listed, on["records"][:, QUAD_LEN]), f"{label}: the lists' lengths differ"
    assert (kept_on <= listed).all() and (kept_off <= listed).all(), f"{label}: a tile staged more quads than it lists"
    walks = kept_off > 0
    print(f"{label}: {int((listed > 0).sum())} tiles list {int(listed.sum())} quads; {int(walks.sum())} of them draw a triangle and "
          f"list {int(listed[walks].sum())}; staged {int(kept_off.sum())} -> {int(kept_on.sum())}; "
          f"{int((walks & (kept_on == 0)).sum())} tiles skip phase 3")
    if single_light:
        assert walks.any() and np.array_equal(kept_off[walks], listed[walks]), label
        assert (kept_on <= kept_off).all(), label
        assert (kept_on[walks] < listed[walks]).any(), f"{label}: no tile that draws a triangle stages fewer quads than it lists"
    else:                                 # (the multi-light kernels keep the strip rule alone and report nothing)
        assert not kept_off.any() and not kept_on.any(), label


def _restore(before):
    if before is None:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = before


@pytest.mark.parametrize("name", SCENES)
def test_whole_frames_do_not_depend_on_the_switch(api, name):
    scene = scenes.build(api, name)
    before = os.environ.get(SWITCH)
    try:
        backend = scene._backend()
        off, on = _frame_only(backend, scene, "count0"), _frame_only(backend, scene, "count")
        _same_frames(name, off, on)
        _kept(name, off, on)
        # the plain spellings render the same frame and leave word 8 alone
        plain = [_frame_only(backend, scene, v) for v in ("0", "1")]
        for p in plain:
            assert np.array_equal(p["out"], off["out"]) and not p["records"][:, KEPT].any(), name
        # counted frames: the general kernels behind the same k_bin_work
        (c_off, s_off), (c_on, s_on) = _counted(backend, scene, "0"), _counted(backend, scene, "1")
        assert s_off == s_on and s_off["frag_quad"] > 0, f"{name}: {s_off} -> {s_on}"
        for key in c_off:
            assert np.array_equal(c_off[key], c_on[key]), f"{name}: counted {key} differs"
        assert np.array_equal(c_off["out"], off["out"]), f"{name}: frame-only and counted frames differ"
    finally:
        _restore(before)
        scene.close()


@pytest.mark.parametrize("what", VARIANTS)
def test_supersampled_and_partial_frames(api, what):
    scene = scenes.build(api, "torus_spot" if what == "ss2" else "diablo_floor_small")
    before = os.environ.get(SWITCH)
    try:
        backend = scene._backend()
        h = int(scene.resolution[0])
        kw = {}
        if what == "ss2":
            scene.supersample = 2
        elif what == "band":
            kw["row_band"] = (h // 3 + 5, 2 * h // 3 + 3)         # no multiple of the tile
        else:
            kw["stripe"] = (1, 3)
        off, on = _frame_only(backend, scene, "count0", **kw), _frame_only(backend, scene, "count", **kw)
        _same_frames(what, off, on)
        _kept(what, off, on)
    finally:
        _restore(before)
        scene.close()


def test_two_lights(api):
    scene = scenes.build(api, "torus_spot")
    before = os.environ.get(SWITCH)
    try:
        scene.add_light(api.Light((-2, 3, 1), ambient_strength=0.1, specular_strength=0.1))
        backend = scene._backend()
        off, on = _frame_only(backend, scene, "count0"), _frame_only(backend, scene, "count")
        _same_frames("two lights", off, on)
        _kept("two lights", off, on, single_light=False)
        (c_off, s_off), (c_on, s_on) = _counted(backend, scene, "0"), _counted(backend, scene, "1")
        assert s_off == s_on and s_off["frag_quad"] > 0
    finally:
        _restore(before)
        scene.close()


CHILD = r'''
import os, sys
ROOT, OUT = sys.argv[1], sys.argv[2]
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import scenes

api = scenes.product_api()
scene = scenes.build(api, "diablo_floor_small")
backend = scene._backend()
save = {}
for value in ("count0", "count"):
    os.environ["MR_QUAD_TILE_CULL"] = value
    for _ in range(3):                   # the second frame shares out the tiles the first found heavy
        save[value + "_out"] = backend.render(scene, shadows=True, counters=False, keep_buffers=True).copy()
    save[value + "_split"] = np.array(int(backend.frame_path()["split"]))
    save[value + "_z"] = backend.read_z().view(np.uint64)
    save[value + "_winner"] = backend.read_winner()
    save[value + "_stencil"] = backend.read_stencil()
    save[value + "_records"] = backend.read_tile_records().astype(np.int64)
scene.close()
np.savez(os.path.join(OUT, "split.npz"), **save)
print("ok split")
'''


def test_split_tiles_apply_it_to_their_share(tmp_path):
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ, MR_TILE_SPLIT="1")
    env.pop(SWITCH, None)
    got = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path)], env=env, capture_output=True, text=True, timeout=300)
    assert got.returncode == 0 and "ok split" in got.stdout, got.stdout[-2000:] + got.stderr[-3000:]
    d = np.load(tmp_path / "split.npz")
    off, on = ({k: d[f"{v}_{k}"] for k in ("out", "z", "winner", "stencil", "records")} for v in ("count0", "count"))
    assert int(d["count0_split"]) == 1 and int(d["count_split"]) == 1, "the child's frames did not split their heavy tiles"
    _same_frames("split", off, on)
    _kept("split", off, on)
