"""GPU: the rasteriser on adversarial meshes (``scenes.soup`` / ``welded`` / ``dense_tile``).

The other GPU tests vary cameras, lights and host modes over a few well-behaved meshes.  What is specific to the HIP
path is decided by geometry: a (triangle, tile) pair is small or big at 24 box pixels, a face bins itself up to four
tiles and becomes 64-tile work items above, a tile walks its lists in rounds of 64 records, a one-sample box and a
one-fragment face take NumPy's dot path, ties go to the largest face index whatever order the lists were filled in,
edges with more than two faces go through the edge stage's extra lists.  The generated meshes put counts and boxes on
both sides of each limit, and ``test_the_seeds_reach_what_they_were_made_for`` holds them to it.

The sequential C oracle is the yardstick: on these meshes it was compared with the unmodified reference (the five
captures soup_s0, welded_s0, welded_s4_ortho, dense_tile_s0 and soup_behind_camera_s0 under tests/golden/, and a wider
sweep over ten seeds and six variants of each, whose outcome DESIGN.md gives where it lists the captures).
Bars, the project's: z bits, winners, stencil, counters and the silhouette set exact, float frame 2e-6, uint8 +-1.
"""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import scenes
from conftest import load_golden
from multilight_ref import compose, extra_lights
from supersample_ref import max_diff, pair, resolve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

GENERATORS = ("soup", "welded", "dense_tile")
SEEDS = tuple(range(8))
TILE = 16
SMALL_LEN, BIG_LEN, QUAD_LEN = 5, 6, 7            # columns of a tile record: the lengths of the tile's three lists


def variant_of(seed):
    return scenes.VARIANTS[seed % len(scenes.VARIANTS)]


def build(api, gen, seed, **kw):
    return getattr(scenes, gen)(api, seed=seed, variant=variant_of(seed), **kw)


def _sil(rows):
    return set(map(tuple, np.asarray(rows).tolist()))


def _taps(backend):
    return dict(z=backend.read_z(), winner=backend.read_winner(), stencil=backend.read_stencil(),
                frame=backend.read_frame_f32())


def assert_matches(got, out, want, label, pixels=None):
    """The project's bars; *pixels* (H, W) bool limits the two frame comparisons (rows bottom-up like the buffers)."""
    bad_z = int((got["z"].view(np.uint64) != want.z.view(np.uint64)).sum())
    assert bad_z == 0, f"{label}: {bad_z} z-buffer entries not bit-exact"
    assert int((got["winner"] != want.winner).sum()) == 0, f"{label}: winner map differs"
    assert int((got["stencil"] != want.stencil).sum()) == 0, f"{label}: stencil differs"
    keep = np.ones(want.winner.shape, bool) if pixels is None else pixels
    err = np.abs(got["frame"].astype(np.float64) - want.frame.astype(np.float64))[keep]
    print(f"{label}: float frame off by {err.max():.3g}")
    assert err.max() <= 2e-6, f"{label}: float frame off by {err.max():.3g}"
    d = np.abs(out.astype(np.int16) - want.out.astype(np.int16))[keep[::-1]]
    assert d.max() <= 1, f"{label}: uint8 frame off by {d.max()} ({int((d > 1).sum())} values > 1)"


@pytest.fixture(scope="module")
def rendered(api, oracle_mod):
    """(generator, seed) -> the oracle's result, the device's buffers of two renders and what the reach test reads.
    Rendered once, on first use, and left alone."""
    done = {}

    def get(gen, seed):
        if (gen, seed) not in done:
            scene = build(api, gen, seed)
            want = oracle_mod.render(scene)
            backend = scene._backend()
            out = backend.render(scene, keep_float=True).copy()
            first = _taps(backend)
            stats = dict(backend.last_stats)
            sil = _sil(backend.read_silhouette())
            records = backend.read_tile_records().astype(np.int64)
            again = backend.render(scene, keep_float=True).copy()
            second = _taps(backend)
            frame_only = scene.render().copy()
            done[gen, seed] = dict(want=want, out=out, first=first, stats=stats, sil=sil, records=records, again=again,
                                   second=second, frame_only=frame_only, geometry=scenes.face_geometry(scene))
            scene.close()
        return done[gen, seed]
    return get


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("gen", GENERATORS)
def test_seed_matches_oracle(rendered, gen, seed):
    """Eight seeds of each generator, cycling through the variants: buffers, counters and the silhouette set against
    the oracle, the frame-only mode against the counted one, and a second render against the first -- the order in
    which the tile lists were filled differs between the two, the frame may not."""
    r = rendered(gen, seed)
    want, label = r["want"], f"{gen} seed {seed} ({variant_of(seed)})"
    assert_matches(r["first"], r["out"], want, label)
    st = r["stats"]
    assert st["frag_tri"] == want.stats["frag_tri_pass1"], label
    assert st["frag_quad"] == want.stats["frag_quad"], label
    assert st["n_quads"] == want.stats["n_quads"], label
    assert r["sil"] == _sil(want.silhouette), f"{label}: silhouette set differs"
    assert np.array_equal(r["frame_only"], r["out"]), f"{label}: frame-only mode differs"
    assert np.array_equal(r["again"], r["out"]), f"{label}: second render, uint8 frame"
    assert np.array_equal(r["second"]["frame"].view(np.uint32), r["first"]["frame"].view(np.uint32)), f"{label}: second render, frame"
    assert np.array_equal(r["second"]["z"].view(np.uint64), r["first"]["z"].view(np.uint64)), f"{label}: second render, z"
    assert np.array_equal(r["second"]["winner"], r["first"]["winner"]), f"{label}: second render, winners"


def test_the_seeds_reach_what_they_were_made_for(api, rendered):
    """Across the seeds above: the tile-list lengths on both sides of a round of 64 and of two, small and big pairs in
    one tile, pixel boxes on both sides of 24 pixels, of one sample, of 4 tiles and of 64 tiles -- and a welded edge with
    five faces or more.  A generator that misses one of these is changed, not this list."""
    from collections import Counter
    small, big, quads, both = [], [], [], 0
    area, tiles = [], []
    for gen in GENERATORS:
        for seed in SEEDS:
            r = rendered(gen, seed)
            rec = r["records"]
            small.append(rec[:, SMALL_LEN]), big.append(rec[:, BIG_LEN]), quads.append(rec[:, QUAD_LEN])
            both += int(((rec[:, SMALL_LEN] > 0) & (rec[:, BIG_LEN] > 0)).sum())
            _, culled, box = r["geometry"]
            box = box[~culled]
            a = (box[:, 1] - box[:, 0]) * (box[:, 3] - box[:, 2])
            box, a = box[a > 0], a[a > 0]
            area.append(a)
            tiles.append(((box[:, 1] - 1) // TILE - box[:, 0] // TILE + 1) * ((box[:, 3] - 1) // TILE - box[:, 2] // TILE + 1))
    small, big, quads, area, tiles = (np.concatenate(v) for v in (small, big, quads, area, tiles))
    print(f"longest lists: small {small.max()}, big {big.max()}, quads {quads.max()}; tiles with small and big pairs {both}")
    print(f"boxes: {len(area)}, of one sample {int((area == 1).sum())}, up to 24 px {int((area <= 24).sum())}, "
          f"on 4 tiles {int((tiles == 4).sum())}, on 5 to 64 {int(((tiles > 4) & (tiles <= 64)).sum())}, on more {int((tiles > 64).sum())}")
    assert ((small >= 1) & (small <= 63)).any() and ((small >= 65) & (small <= 128)).any() and (small > 128).any()
    assert (big > 64).any() and (quads > 64).any() and both > 0
    assert (area <= 24).any() and (area > 24).any() and (area == 1).any()
    assert (tiles == 4).any() and ((tiles >= 5) & (tiles <= 64)).any() and (tiles > 64).any()
    for seed in SEEDS:
        scene = build(api, "welded", seed)
        corners = np.asarray(scene.models[0]._faces)[:, :, 0]
        scene.close()
        incident = Counter(frozenset((int(f[k]), int(f[(k + 1) % 3]))) for f in corners for k in range(3))
        assert max(n for e, n in incident.items() if len(e) == 2) >= 5, f"welded seed {seed}"


def _in_tile_box(box, px, py):
    """Pixels of every face's box (x0, x1, y0, y1) inside the tile of pixel (px, py): what pair_class goes by."""
    x0, y0 = px // TILE * TILE, py // TILE * TILE
    w = np.minimum(box[:, 1], x0 + TILE) - np.maximum(box[:, 0], x0)
    h = np.minimum(box[:, 3], y0 + TILE) - np.maximum(box[:, 2], y0)
    return np.maximum(w, 0) * np.maximum(h, 0)


def test_a_small_and_a_big_pair_tie_in_one_tile(api, oracle_mod, rendered):
    """dense_tile's pivot faces share their first corner, which lies on the sample of the frame's centre: there each of
    them has that corner's z to the bit, whatever its size (scenes._dense_tile).  For every seed but the one under the
    f64 variant, whose rotation moves the vertex: the oracle renders the pivot faces whose box in the centre tile has
    at most 24 pixels and those with more separately, and at some pixel both are there with identical z bits, the whole
    scene has that z there too, and its winner is the larger face index of the two -- small for some seeds, big for
    others.  The device lists them in the centre tile's small and big lists as their boxes say, and has to agree with
    the oracle's winner (test_seed_matches_oracle), whatever order its two lists were filled in."""
    winners_are = set()
    for seed in SEEDS:
        if variant_of(seed) == "f64":
            continue
        want = rendered("dense_tile", seed)["want"]
        scene = build(api, "dense_tile", seed)
        faces = np.asarray(scene.models[0]._faces).copy()
        pivot = np.flatnonzero(scenes.dense_tile_groups(seed) == "pivot")
        _, culled, box = scenes.face_geometry(scene)
        assert not culled[pivot].any()
        h, w = scene.resolution
        area = _in_tile_box(box[pivot], w // 2, h // 2)
        parts = {}
        for kind, idx in (("small", pivot[area <= 24]), ("big", pivot[area > 24])):
            assert len(idx) >= 2, (seed, kind, area.tolist())
            scene.models[0]._faces = faces[idx]
            r = oracle_mod.render(scene)
            parts[kind] = (r.z.view(np.uint64).copy(), np.where(r.winner >= 0, idx[np.maximum(r.winner, 0)], -1))
        # and the device classes them as the host boxes say (pair_class sends a face that needs the per-fragment clip
        # test to the big list whatever its size): of the pivot faces alone, the centre tile lists exactly the small
        # ones as small pairs and the big ones as big pairs
        scene.models[0]._faces = faces[pivot]
        backend = scene._backend()
        backend.render(scene, keep_float=True)
        rec = backend.read_tile_records().astype(np.int64)
        lengths = (int((area <= 24).sum()), int((area > 24).sum()))
        assert ((rec[:, SMALL_LEN] == lengths[0]) & (rec[:, BIG_LEN] == lengths[1])).any(), \
            (seed, lengths, rec[rec[:, SMALL_LEN] + rec[:, BIG_LEN] > 0][:, [SMALL_LEN, BIG_LEN]].tolist())
        scene.close()
        (zs, ws), (zb, wb) = parts["small"], parts["big"]
        tie = (ws >= 0) & (wb >= 0) & (zs == zb) & (want.z.view(np.uint64) == zs)
        ys, xs = np.nonzero(tie)
        print(f"dense_tile seed {seed} ({variant_of(seed)}): a small and a big pair tie at the front at {list(zip(xs.tolist(), ys.tolist()))}")
        assert len(xs) >= 1, f"seed {seed}: no pixel where a small and a big pair tie at the front"
        for x, y in zip(xs, ys):
            assert _in_tile_box(box[[ws[y, x]]], x, y)[0] <= 24 < _in_tile_box(box[[wb[y, x]]], x, y)[0]
            assert want.winner[y, x] == max(ws[y, x], wb[y, x]), f"seed {seed}: the larger index does not win at ({x}, {y})"
            winners_are.add("small" if ws[y, x] > wb[y, x] else "big")
    assert winners_are == {"small", "big"}


@pytest.mark.parametrize("gen", GENERATORS)
def test_uneven_bands_and_stripes_tile_the_frame(api, gen):
    """Row bands cut at rows that are no multiple of 16, and every rank's tile rows of a three-way stripe split,
    assembled as test_gpu_parity.py assembles them: exactly the whole frame."""
    import torch
    from py_numpy_renderer_amd.multigpu import stripe_rows, unstripe
    scene = build(api, gen, 0)
    backend = scene._backend()
    full = scene.render().copy()
    h = full.shape[0]
    for cuts in ((0, 37, 90, h), (0, 1, 17, 100, 135, h)):
        parts = [scene.render(row_band=(cuts[i], cuts[i + 1])) for i in range(len(cuts) - 1)]
        assert np.array_equal(np.concatenate(parts, axis=0), full), cuts
    parts = [backend.render(scene, counters=False, stripe=(r, 3)) for r in range(3)]
    assert all(p.shape[0] == stripe_rows(h, 3) for p in parts)
    frame = unstripe(torch.from_numpy(np.concatenate(parts, axis=0)), h, 3).numpy()
    assert np.array_equal(frame, full)
    scene.close()


def _rows_clear_of_first_cluster(scene):
    """A row band (0, k) below everything the first 64 faces' bounding box can reach on the screen, from its eight
    corners through ``camera.MVP`` and ``camera.viewport`` with the two pixels' margin that k_setup's cluster test adds."""
    model = scene.models[0]
    corners = np.asarray(model._faces)[:64, :, 0]
    v = np.asarray(model.vertices, dtype=np.float64)[corners.ravel()][:, :3]
    lo, hi = v.min(axis=0), v.max(axis=0)
    box = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2], 1.0] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    clip = box @ scene.camera.MVP
    assert (clip[:, 3] > 0).all()
    y = ((clip / clip[:, 3:4]) @ scene.camera.viewport)[:, 1]
    return int(np.floor(y.min() - 2.0)) - 1


@pytest.mark.parametrize("gen", ["soup", "welded"])
def test_cluster_culling_changes_nothing(api, gen, monkeypatch):
    """MR_CLUSTER_CULL (re-read every frame) in 0 / count / box: clusters of 64 faces that hold faces without area,
    whose cone and box flags are built from them, give the same frame, z, winners, stencil and set-up counts.  That a
    cluster can go at all is shown on welded: on the rows below its first 64 faces' box that cluster must be dropped."""
    scene = build(api, gen, 0)
    backend = scene._backend()
    bands = [(37, 90)]
    if gen == "welded":
        k = _rows_clear_of_first_cluster(scene)
        assert k >= 1, "the first cluster's box reaches the frame's first rows: no band to drop it on"
        bands.append((0, k))
    results = {}
    for mode in ("0", "count", "box"):
        monkeypatch.setenv("MR_CLUSTER_CULL", mode)
        full = backend.render(scene, counters=False, keep_buffers=True).copy()
        culled = [backend.clusters_culled()]
        taps = (backend.read_z().copy(), backend.read_winner().copy(), backend.read_stencil().copy())
        stats = {k: backend.last_stats[k] for k in ("n_faces_setup", "n_quads", "n_quads_drawn", "tri_bin_entries", "quad_bin_entries")}
        parts = []
        for band in bands:
            parts.append(backend.render(scene, counters=False, row_band=band).copy())
            culled.append(backend.clusters_culled())
        print(f"{gen}, MR_CLUSTER_CULL={mode}: clusters dropped on the whole frame and on rows {bands}: {culled}")
        results[mode] = (full, taps, stats, parts, culled)
    ref = results["0"]
    assert ref[4] == [0] * (1 + len(bands))
    for mode in ("count", "box"):
        got = results[mode]
        assert np.array_equal(got[0], ref[0]), mode
        for a, b in zip(got[1], ref[1]):
            assert np.array_equal(a, b, equal_nan=True), mode
        assert got[2] == ref[2], mode
        for a, b in zip(got[3], ref[3]):
            assert np.array_equal(a, b), mode
    if gen == "welded":
        assert results["count"][4][2] >= 1, "the first cluster lies off the band's rows and was not dropped"
    scene.close()


_SPREAD_CHILD = r"""
import os, sys
import numpy as np
sys.path[:0] = [{root!r}, {tests!r}]
import scenes
api = scenes.product_api()
scene = scenes.welded(api, seed=0)
backend = scene._backend()
out = backend.render(scene, keep_float=True).copy()
np.savez({path!r}, out=out, z=backend.read_z(), winner=backend.read_winner(), stencil=backend.read_stencil(),
         frame=backend.read_frame_f32(), silhouette=backend.read_silhouette(),
         counters=np.array([backend.last_stats[k] for k in ("frag_tri", "frag_quad", "n_quads")], dtype=np.int64))
scene.close()
"""


@pytest.mark.parametrize("spread", [-1, 0, 4])
def test_edge_spread_on_welded(rendered, tmp_path, spread):
    """MR_EDGE_SPREAD (read once per process: a child process per value, as in test_edge_spread_gpu.py) on edges with
    up to seven faces: every layout of the edge stage builds the oracle's silhouette and frame."""
    want = rendered("welded", 0)["want"]
    path = str(tmp_path / "welded.npz")
    code = _SPREAD_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), path=path)
    env = dict(os.environ, MR_EDGE_SPREAD=str(spread))
    env.pop("MR_SIL_CACHE", None)
    proc = subprocess.run([sys.executable, "-c", code], env=env, timeout=300, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-3000:]
    got = np.load(path)
    assert_matches(got, got["out"], want, f"welded at spread {spread}")
    assert len(got["silhouette"]) == want.stats["n_quads"] and _sil(got["silhouette"]) == _sil(want.silhouette)
    assert got["counters"].tolist() == [want.stats[k] for k in ("frag_tri_pass1", "frag_quad", "n_quads")]


def test_dense_tile_supersampled(api, oracle_mod):
    """supersample = 2 against the oracle's sample grid, box-filtered (supersample_ref): +-1, and the grid bit for bit."""
    scene, twin = pair(api, "dense_tile", 2)
    backend = scene._backend()
    out = backend.render(scene)
    r = oracle_mod.render(twin)
    worst, n_one = max_diff(out, resolve(r.frame, 2))
    assert worst <= 1, f"max diff {worst}, {n_one} pixels off by one"
    assert np.array_equal(backend.read_z().view(np.uint64), r.z.view(np.uint64)), "z-buffer not bit-exact"
    assert np.array_equal(backend.read_winner(), r.winner), "winner map differs"
    assert np.array_equal(backend.read_stencil(), r.stencil), "stencil differs"
    assert np.array_equal(scene.render(), out)
    scene.close()


def test_welded_under_four_lights(api, oracle_mod):
    """The three lights of multilight_ref on top of the scene's own, with test_multilight_gpu.py's bars: uint8 +-1, float
    frame n * 2e-6 + 1e-6, z, winners, every light's stencil, silhouette and the counters exact."""
    scene = scenes.welded(api, seed=0)
    for light in extra_lights(api):
        scene.add_light(light)
    n = len(scene.lights)
    assert n == 4
    ref = compose(oracle_mod, scene)
    backend = scene._backend()
    out = backend.render(scene, keep_float=True)
    st = dict(backend.last_stats)
    worst, n_one = max_diff(out, ref.out)
    assert worst <= 1, f"uint8 frame off by {worst}"
    err = float(np.abs(backend.read_frame_f32().astype(np.float64) - ref.frame.astype(np.float64)).max())
    print(f"float frame: max error {err:.3g} (bound {n * 2e-6 + 1e-6:.3g})")
    assert err <= n * 2e-6 + 1e-6, f"float frame off by {err:.3g}"
    assert np.array_equal(backend.read_z().view(np.uint64), ref.z.view(np.uint64)), "z-buffer not bit-exact"
    assert np.array_equal(backend.read_winner(), ref.winner), "winner map differs"
    for k, r in enumerate(ref.per):
        assert np.array_equal(backend.read_stencil(light=k), r.stencil), f"stencil of light {k} differs"
        sil = backend.read_silhouette(light=k)
        assert len(sil) == r.stats["n_quads"] and _sil(sil) == _sil(r.silhouette), f"silhouette of light {k} differs"
    assert st["frag_tri"] == ref.per[0].stats["frag_tri_pass1"]
    for key in ("frag_quad", "n_quads", "n_quads_drawn", "stencil_updates"):
        assert st[key] == sum(r.stats[key] for r in ref.per), key
    assert np.array_equal(scene.render(), out)
    scene.close()


def test_dense_tile_with_lists_far_too_small(api, rendered):
    """Lists that start at 4 small pairs, 2 big pairs, 3 quads and 16 work items where a tile needs hundreds: the
    frame grows them and ends at the unconstrained frame.  The first frame enqueued with such lists must report the
    overflow (so the capacities were taken), and the tile lists of the frame that ends it are the unconstrained ones."""
    import torch
    r = rendered("dense_tile", 0)
    want, records = r["out"], r["records"]
    longest = records[:, [SMALL_LEN, BIG_LEN, QUAD_LEN]].max(axis=0)
    assert (longest > [4, 2, 3]).all(), longest
    scene = build(api, "dense_tile", 0)
    backend = scene._backend()
    backend.set_list_capacities(small_pairs=4, big_pairs=2, quads=3, work=16)
    h, w = (int(v) for v in scene.resolution)
    out = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    backend.render_device(scene, out.data_ptr(), stream.cuda_stream, shadows=True, no_timing=True)
    stream.synchronize()
    assert backend.overflowed(), "a frame with lists of 4 / 2 / 3 entries did not overflow"
    assert np.array_equal(scene.render(), want)
    backend.render(scene, keep_float=True)
    assert np.array_equal(backend.read_tile_records().astype(np.int64)[:, [SMALL_LEN, BIG_LEN, QUAD_LEN]],
                          records[:, [SMALL_LEN, BIG_LEN, QUAD_LEN]])
    scene.close()


def test_soup_behind_camera_matches_capture_in_front_of_the_camera(api):
    """The capture of a soup with three large faces that have corners behind the camera plane.  z bits, winners, stencil,
    face status and counts are the reference's everywhere; the frame is held to it at every pixel whose winner lies
    in front of the camera plane.  At the others upstream writes z and no colour (obj/triangular.py:139-141 filters every
    fragment away) and the kernels, like the oracle, shade: parity is defined in front of the camera plane."""
    name, = scenes.BEHIND_CAMERA
    g, meta = load_golden(name)
    scene = scenes.build(api, name)
    left_out = scenes.behind_camera_pixels(scene, g["winner"])
    share = left_out.mean()
    print(f"left out: {int(left_out.sum())} pixels, {100 * share:.1f} % of the frame")
    assert 1 <= left_out.sum() and share <= 0.25
    background = np.float32([64 / 255, 0.5, 198 / 255])
    assert (g["frame"][left_out] == background).all(), "the capture shows something under a face behind the camera"
    backend = scene._backend()
    out = backend.render(scene, keep_float=True, face_status=True)
    want = SimpleNamespace(z=g["z"], winner=g["winner"], stencil=g["stencil"], frame=g["frame"], out=g["out"])
    assert_matches(_taps(backend), out, want, name, pixels=~left_out)
    assert np.array_equal(backend.read_face_status(), g["face_status"])
    st = backend.last_stats
    assert st["frag_tri"] == meta["counts"]["frag_tri_pass1"]
    assert st["frag_quad"] == meta["counts"]["frag_quad"]
    assert st["n_quads"] == meta["counts"]["n_quads"]
    assert _sil(backend.read_silhouette()) == _sil(g["silhouette"])
    scene.close()
