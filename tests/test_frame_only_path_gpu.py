"""GPU: the frame-only kernels (k_setup, k_tile) against the general ones (k_setup_full, k_tile_full).

One source, one compile-time switch (kernels_tile.h tile_body, kernels_geometry.h setup_body): the frame-only kernels
carry no fragment counters and know no face of a ``depth_test=False`` model; the frame plan (host_frame.h) sends a frame
to them unless it is counted, asks for the per-face status or the scene has such a model.  Everything here is an
equality: the frame, z, the winners and -- where a triangle was drawn, the frame-only contract of
test_gpu_parity.test_frame_only_mode_renders_the_same_frame -- the stencil are the same bytes either way
(``mr_debug_force_full``), and the frame the plan chose is the committed capture (the project's bars: z and winner
bits exact, uint8 +-1).  ``mr_debug_frame_path`` says which kernels ran.
"""
import functools

import numpy as np
import pytest

import scenes
from conftest import load_golden

pytestmark = pytest.mark.gpu

SCENES = ["cube_small", "diablo_floor_small", "kat_house", "torus_skybox_small", "gizmos_small", "fins_nonmanifold",
          "torus_spot", "dense_tile_s0", "soup_behind_camera_s0"]
STAT_KEYS = ("frag_tri", "frag_quad", "covered_px", "lit_px", "stencil_updates", "n_faces", "n_faces_setup", "n_quads",
             "n_quads_drawn", "tri_bin_entries", "quad_bin_entries")


def _taps(backend):
    return backend.read_z().copy(), backend.read_winner().copy(), backend.read_stencil().copy()


@functools.lru_cache(maxsize=None)
def _both(name):
    """The scene rendered with the buffers kept, by the kernels the plan chooses and by the general ones: each
    (frame, z, winner, stencil, frame_path), computed once and shared."""
    api = scenes.product_api()
    scene = scenes.build(api, name)
    backend = scene._backend()
    got = []
    for force in (False, True):
        backend.force_full(force)
        frame = backend.render(scene, counters=False, keep_buffers=True).copy()
        got.append((frame, *_taps(backend), backend.frame_path()))
    scene.close()
    for g in got:
        for a in g[:4]:
            a.setflags(write=False)
    return got


@pytest.mark.parametrize("name", SCENES)
def test_same_bytes_from_either_variant(name):
    (frame, z, winner, stencil, path), (f_frame, f_z, f_winner, f_stencil, f_path) = _both(name)
    assert path["full"] is False and f_path["full"] is True
    assert np.array_equal(frame, f_frame)
    assert np.array_equal(z.view(np.uint64), f_z.view(np.uint64))
    assert np.array_equal(winner, f_winner)
    covered = winner >= 0
    assert covered.any()
    assert np.array_equal(stencil[covered], f_stencil[covered])


@pytest.mark.parametrize("name", SCENES)
def test_frame_only_frame_is_the_capture(api, name):
    g, _ = load_golden(name)
    frame, z, winner, stencil, path = _both(name)[0]
    assert path["full"] is False
    assert np.array_equal(z.view(np.uint64), g["z"].view(np.uint64))
    assert np.array_equal(winner, g["winner"])
    covered = winner >= 0
    assert np.array_equal(stencil[covered], g["stencil"][covered])
    held = np.ones(winner.shape, bool)
    if name in scenes.BEHIND_CAMERA:         # the frame is the reference's in front of the camera plane
        scene = scenes.build(api, name)
        held = ~scenes.behind_camera_pixels(scene, g["winner"])
        scene.close()
    d = np.abs(frame.astype(np.int16) - g["out"].astype(np.int16))[held[::-1]]      # (the buffers' rows are bottom-up)
    assert d.max() <= 1, f"{name}: uint8 frame off by {d.max()}"


def test_plan_chooses_the_variant(api):
    scene = scenes.build(api, "cube_small")
    backend = scene._backend()
    plain = scene.render().copy()
    assert backend.frame_path()["full"] is False
    lengths = backend.read_tile_records()[:, 5:8].copy()
    assert lengths.any() and not backend.read_tile_records()[:, 8:12].any()      # list lengths, and no time stamps
    assert not backend.read_tile_records()[:, 0:5].any()                         # ... and no counts
    st = backend.stats()
    assert st["frag_tri"] == st["frag_quad"] == st["covered_px"] == st["lit_px"] == st["stencil_updates"] == -1
    assert st["n_faces_setup"] > 0 and st["tri_bin_entries"] == int(lengths[:, 0:2].sum())
    counted = backend.render(scene, counters=True).copy()
    assert backend.frame_path()["full"] is True and backend.last_stats["frag_tri"] > 0
    assert np.array_equal(backend.read_tile_records()[:, 5:8], lengths) and backend.read_tile_records()[:, 8:10].all()
    status = backend.render(scene, counters=False, face_status=True).copy()
    assert backend.frame_path()["full"] is True
    assert np.array_equal(backend.read_face_status(), load_golden("cube_small")[0]["face_status"])
    assert np.array_equal(counted, plain) and np.array_equal(status, plain)
    scene.render()
    assert backend.frame_path()["full"] is False
    backend.force_full(True)
    assert np.array_equal(scene.render(), plain) and backend.frame_path()["full"] is True
    backend.force_full(False)
    assert np.array_equal(scene.render(), plain) and backend.frame_path()["full"] is False
    scene.close()


def test_scene_with_a_nodepth_model_takes_the_general_kernels(api):
    g, _ = load_golden("cube_tetra_nodepth")
    scene = scenes.build(api, "cube_tetra_nodepth")
    backend = scene._backend()
    frame = scene.render().copy()
    assert backend.frame_path()["full"] is True
    assert np.abs(frame.astype(np.int16) - g["out"].astype(np.int16)).max() <= 1
    kept = backend.render(scene, counters=False, keep_buffers=True)
    assert backend.frame_path()["full"] is True and np.array_equal(kept, frame)
    assert np.array_equal(backend.read_z().view(np.uint64), g["z"].view(np.uint64))
    assert np.array_equal(backend.read_winner(), g["winner"])
    scene.close()


def test_counted_and_frame_only_frames_alternate(api):
    """Counted frames between frame-only ones (which write no counts to the tile records and count nothing in
    k_setup) report the statistics of a fresh scene's counted frame, and every frame is the same."""
    fresh = scenes.build(api, "diablo_floor_small")
    want = fresh._backend().render(fresh, counters=True).copy()
    want_stats = {k: fresh._backend().last_stats[k] for k in STAT_KEYS}
    fresh.close()
    assert want_stats["frag_tri"] > 0 and want_stats["frag_quad"] > 0 and want_stats["lit_px"] > 0
    scene = scenes.build(api, "diablo_floor_small")
    backend = scene._backend()
    for _ in range(4):
        assert np.array_equal(scene.render(), want)
        assert backend.frame_path()["full"] is False
        assert np.array_equal(backend.render(scene, counters=True), want)
        assert backend.frame_path()["full"] is True
        assert {k: backend.last_stats[k] for k in STAT_KEYS} == want_stats
    scene.close()


def test_frame_only_path_reports_overflow(api):
    """test_gpu_parity.test_work_lists_grow_on_overflow, with the kernels named: the frame-only tile kernel still
    reports a list that ran over, the lists grow, and the frame is the unconstrained one."""
    import torch
    from py_numpy_renderer_amd.multigpu import BandRenderer
    want = _both("diablo_floor_small")[0][0]

    scene = scenes.build(api, "diablo_floor_small")
    backend = scene._backend()
    backend.set_list_capacities(small_pairs=4, big_pairs=2, quads=3, work=16)
    # the capacities do constrain this scene: some tile lists more than they allow (lengths from an unconstrained scene)
    free = scenes.build(api, "diablo_floor_small")
    free.render()
    longest = free._backend().read_tile_records()[:, 5:8].max(axis=0)
    free.close()
    assert longest[0] > 4 and longest[1] > 2 and longest[2] > 3, longest
    assert np.array_equal(scene.render(), want)
    assert backend.frame_path()["full"] is False
    # ... so the overflow was reported and the lists grew: a truncated list loses triangles or quads, and the frame
    # above would not be the unconstrained one; nothing is left to report
    assert np.array_equal(backend.read_tile_records()[:, 5:8].max(axis=0), longest)
    assert not backend.overflowed()
    scene.close()

    scene = scenes.build(api, "diablo_floor_small")
    backend = scene._backend()
    backend.set_list_capacities(small_pairs=4, big_pairs=2, quads=3, work=16)
    br = BandRenderer(scene, 0, 1, shadows=True, light_timing=True, frames_in_flight=2)
    frames = [br.step() for _ in range(4)]
    assert br.verify()
    torch.cuda.synchronize()
    assert backend.frame_path()["full"] is False
    assert np.array_equal(backend.read_tile_records()[:, 5:8].max(axis=0), longest)
    for frame in frames[-2:]:
        assert np.array_equal(frame.cpu().numpy(), want)
    scene.close()


def _either_way(backend, render):
    """render() by the plan's kernels and by the general ones: (frame, path) each."""
    got = []
    for force in (False, True):
        backend.force_full(force)
        got.append((render().copy(), backend.frame_path()))
    backend.force_full(False)
    return got


def test_split_stripe_is_the_same_from_either_variant(api):
    """k_tile<1, .> : a stripe of a small scene, its heavy tiles shared out once a frame has left their classes
    (chosen as test_gpu_parity.test_split_heavy_tiles_render_the_same_rows does: some tile must qualify)."""
    scene = scenes.build(api, "dense_tile_s0")
    backend = scene._backend()
    render = lambda: backend.render(scene, counters=False, stripe=(0, 2))
    first = render().copy()
    rec = backend.read_tile_records().astype(np.int64)
    cost = 20 + 2 * rec[:, 5] + 30 * rec[:, 6] + 3 * rec[:, 7]          # kernels_tile.h tile_cost
    heavy = (cost >= 350) & (rec[:, 7] >= 32)
    assert heavy.any(), "no tile qualifies: the test would not exercise the split"
    render()                                                            # (ordered from here on: the classes are known)
    (auto, path), (forced, f_path) = _either_way(backend, render)
    assert path == dict(full=False, split=True, ss=False, ml=False, ordered=True)
    assert f_path == dict(path, full=True)
    order = backend.read_tile_order().astype(np.int64)
    assert heavy[order[:int(heavy.sum())]].all()
    assert np.array_equal(auto, forced) and np.array_equal(auto, first)
    scene.close()


def test_supersampled_frame_is_the_same_from_either_variant(api):
    scene = scenes.build(api, "diablo_floor_small")
    scene.supersample = 2
    backend = scene._backend()
    (auto, path), (forced, f_path) = _either_way(backend, lambda: backend.render(scene, counters=False))
    assert path["full"] is False and path["ss"] is True and f_path == dict(path, full=True)
    assert auto.shape == _both("diablo_floor_small")[0][0].shape
    assert np.array_equal(auto, forced)
    scene.close()


def test_row_band_is_the_same_from_either_variant(api):
    want = _both("diablo_floor_small")[0][0]
    scene = scenes.build(api, "diablo_floor_small")
    backend = scene._backend()
    band = (37, 201)
    (auto, path), (forced, f_path) = _either_way(backend, lambda: backend.render(scene, counters=False, row_band=band))
    assert path["full"] is False and f_path["full"] is True
    assert np.array_equal(auto, forced) and np.array_equal(auto, want[band[0]:band[1]])
    scene.close()


def test_lone_frame_after_overlapped_frames_is_ordered(api):
    """Frames in flight keep row-major order, and nobody reads the order k_setup leaves for them; the frame-only tile
    kernel still writes the class bytes, so the first lone frame behind them finds a history: its order is a permutation
    sorted by class, and its bytes are those of a scene that never overlapped."""
    from py_numpy_renderer_amd.multigpu import BandRenderer
    want = _both("diablo_floor_small")[0][0]
    scene = scenes.build(api, "diablo_floor_small")
    backend = scene._backend()
    br = BandRenderer(scene, 0, 1, shadows=True, frames_in_flight=2, timing_every=0)
    for _ in range(6):
        frame = br.step()
    assert br.verify()
    assert backend.frame_path()["ordered"] is False and backend.frame_path()["full"] is False
    assert np.array_equal(frame.cpu().numpy(), want)
    # (a frame counts as alone once no other stream took one of the scene's last eight: host_frame.h plan_frame)
    lone = None
    for _ in range(12):
        lone = scene.render().copy()
        assert np.array_equal(lone, want)
        if backend.frame_path()["ordered"]:
            break
    assert backend.frame_path() == dict(full=False, split=True, ss=False, ml=False, ordered=True)
    order = backend.read_tile_order().astype(np.int64)
    rec = backend.read_tile_records().astype(np.int64)
    n = len(rec)
    assert n <= 2048 and np.array_equal(np.sort(order), np.arange(n))
    cost = 20 + 2 * rec[:, 5] + 30 * rec[:, 6] + 3 * rec[:, 7]                           # kernels_tile.h tile_cost
    cls = np.digitize(-cost, [-500, -350, -250, -170, -110, -70, -40], right=True)        # 0 = heaviest
    cls = np.where((cost >= 350) & (rec[:, 7] >= 32), 0, np.maximum(cls, 1))              # (a small grid's split bar)
    cls[(rec[:, 5] == 0) & (rec[:, 6] == 0)] = 7      # a tile that lists no triangle shows the background: lightest class
    assert (np.diff(cls[order]) >= 0).all()
    assert len(np.unique(cls)) > 1, "one class only: any order would be sorted"
    scene.close()
