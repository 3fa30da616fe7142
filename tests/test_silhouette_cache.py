"""GPU: the silhouette cache (host_silcache.h, SilCache; kernels_geometry.h, quad_block and the capture epilogue of edge_block).

A frame whose light and geometry are those of the frames before reads its silhouette edges and their extruded
world-space quads back instead of testing every edge against the light.  Both paths run the same arithmetic, so
everything here is an equality: a frame that took the cached path (asserted through mr_debug_sil_cache -- a test that
cannot tell which path ran proves nothing) against the same frame rendered with MR_SIL_CACHE=0, and against the oracle.
"""
import importlib.util
import os

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

FUSED, CAPTURE, CACHED = 0, 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _views(api, scene, n):
    """n camera pairs on bench.py's swing around the scene's camera."""
    return _bench().swing_cameras(api, scene, n)


def _counted(backend, scene, face_status=False):
    """One counted frame and everything a caller can read of it."""
    out = backend.render(scene, shadows=True, keep_float=True, face_status=face_status).copy()
    got = dict(out=out, z=backend.read_z().view(np.uint64).copy(), stencil=backend.read_stencil().copy(),
               winner=backend.read_winner().copy(), frame=backend.read_frame_f32().copy(),
               frag_quad=backend.last_stats["frag_quad"], n_quads=backend.last_stats["n_quads"],
               n_quads_drawn=backend.last_stats["n_quads_drawn"],
               silhouette=set(map(tuple, backend.read_silhouette().tolist())))
    if face_status:
        got["status"] = backend.read_face_status().copy()
    return got


def _assert_same(got, want, label):
    for key, w in want.items():
        g = got[key]
        same = np.array_equal(g, w) if isinstance(w, np.ndarray) else g == w
        assert same, f"{label}: {key} differs"


def _path(backend):
    return backend.sil_cache()[0]


@pytest.mark.parametrize("name", ["c3_diablo_floor_1080p", "diablo_floor_lh_gl", "fins_nonmanifold", "torus_spot",
                                  "cube_tetra_nodepth", "c4_torus200k_1080p"])
def test_cached_frames_equal_fused_frames(api, name, monkeypatch):
    """miss -> capture -> cached -> cached, the camera moved between the frames as bench.py's swing does: every frame
    is, bit for bit, the frame of the fused path for that view."""
    scene = scenes.build(api, name)
    backend = scene._backend()
    views = _views(api, scene, 5)
    monkeypatch.setenv("MR_SIL_CACHE", "0")
    want = []
    for cam, dbg in views:
        scene.camera, scene.debug_camera = cam, dbg
        want.append(_counted(backend, scene, face_status=True))
        assert _path(backend) == FUSED
    assert backend.sil_cache()[2] == 0, "MR_SIL_CACHE=0 must not capture"
    assert want[0]["n_quads"] > 0 and len(want[0]["silhouette"]) == want[0]["n_quads"]
    monkeypatch.delenv("MR_SIL_CACHE")
    paths = []
    for k, (cam, dbg) in enumerate(views):
        scene.camera, scene.debug_camera = cam, dbg
        got = _counted(backend, scene, face_status=True)
        paths.append(_path(backend))
        _assert_same(got, want[k], f"{name} view {k} (path {paths[-1]})")
    # synchronous renders complete the capture's event before the next enqueue: the sequence is deterministic
    assert paths == [FUSED, CAPTURE, CACHED, CACHED, CACHED], paths
    assert backend.sil_cache()[1] == want[-1]["n_quads"], "the cache holds one entry per silhouette edge"
    # the frame-only mode (what bench.py times) through the cache
    scene.camera, scene.debug_camera = views[2]
    assert np.array_equal(scene.render(), want[2]["out"]) and _path(backend) == CACHED
    scene.close()


def _oracle_check(oracle_mod, backend, scene, label, want_path=None):
    out = backend.render(scene, shadows=True, keep_float=True)
    if want_path is not None:
        assert _path(backend) == want_path, f"{label}: path {_path(backend)}"
    want = oracle_mod.render(scene, shadows=True)
    assert np.array_equal(backend.read_z().view(np.uint64), want.z.view(np.uint64)), f"{label}: z"
    assert np.array_equal(backend.read_winner(), want.winner), f"{label}: winners"
    assert np.array_equal(backend.read_stencil(), want.stencil), f"{label}: stencil"
    assert np.abs(out.astype(np.int16) - want.out.astype(np.int16)).max() <= 1, f"{label}: frame"


@pytest.mark.parametrize("name", ["diablo_floor_small", "diablo_floor_lh_gl", "torus_spot"])
def test_a_moved_light_is_another_silhouette(api, oracle_mod, name):
    """The key is the light: after it moves (for the directional scene, its direction too) the frames are the
    oracle's for the new light, cached or not; moved back, the oracle's again.  A position that differs in its last
    bit is a different key."""
    scene = scenes.build(api, name)
    backend = scene._backend()
    light = scene.light
    home_pos, home_center = np.array(light.position, dtype=np.float64), np.array(light.center, dtype=np.float64)
    for _ in range(3):
        backend.render(scene, shadows=True)
    assert _path(backend) == CACHED
    light.position = home_pos + np.array((-0.7, 0.4, 0.3))
    if name == "diablo_floor_lh_gl":
        light.center = home_center + np.array((0.3, -0.2, 0.1))
    _oracle_check(oracle_mod, backend, scene, f"{name} moved, first frame", FUSED)
    _oracle_check(oracle_mod, backend, scene, f"{name} moved, second frame", CAPTURE)
    _oracle_check(oracle_mod, backend, scene, f"{name} moved, third frame", CACHED)
    light.position, light.center = home_pos.copy(), home_center.copy()
    _oracle_check(oracle_mod, backend, scene, f"{name} back home", CACHED)       # (the other buffer still holds it)
    nudged = home_pos.copy()
    nudged[0] = np.nextafter(nudged[0], np.inf)
    light.position = nudged
    _oracle_check(oracle_mod, backend, scene, f"{name} last bit", FUSED)
    _oracle_check(oracle_mod, backend, scene, f"{name} last bit, again", None)
    _oracle_check(oracle_mod, backend, scene, f"{name} last bit, third", None)
    _oracle_check(oracle_mod, backend, scene, f"{name} last bit, fourth", None)
    assert _path(backend) == CACHED, "a retired buffer must become free again and be captured into"
    scene.close()


def test_scene_edits_drop_the_cache(api, oracle_mod):
    """A model added, moved, or edited in place: the frames that follow are the oracle's (the flows of
    test_scene_changes_are_picked_up / test_in_place_edits_are_picked_up, with the cache warm in front of each edit)."""
    cam, dbg = scenes._std_cameras(api)
    tet = api.Model.load_model(scenes.bare_tetra_obj())
    sc = scenes._scene(api, cam, dbg, scenes._std_light(api), (90, 120), [tet, scenes._floor(api, textured=False)])
    backend = sc._backend()

    def warm():
        for _ in range(3):
            backend.render(sc, shadows=True)
        assert _path(backend) == CACHED

    warm()
    tet.vertices[:, :3] *= np.float32(0.7)
    _oracle_check(oracle_mod, backend, sc, "after in-place vertex edit", FUSED)
    warm()
    _oracle_check(oracle_mod, backend, sc, "in-place edit, cached", CACHED)
    sc.add_model(api.Model.load_model(scenes.bare_tetra_obj()) @ api.translation((0.5, 0.1, 0.2)))
    _oracle_check(oracle_mod, backend, sc, "after add_model", FUSED)
    warm()
    sc.models[2] = sc.models[2] @ api.translation((-0.3, 0.2, 0.0))
    _oracle_check(oracle_mod, backend, sc, "after Model @ M", FUSED)
    warm()
    _oracle_check(oracle_mod, backend, sc, "Model @ M, cached", CACHED)
    sc.close()


@pytest.mark.parametrize("depth", [3, 4])
def test_frames_in_flight_with_a_changing_light(api, depth, monkeypatch):
    """render_frames with 3 and 4 frames in flight over a sequence whose light changes at irregular intervals --
    on consecutive frames, after long runs, back to an earlier value -- while the camera swings: every frame is the
    same view and light rendered alone on the fused path.  The sequence is run once."""
    scene = scenes.build(api, "diablo_floor_small")
    backend = scene._backend()
    light = scene.light
    home = np.array(light.position, dtype=np.float64)
    spots = [home, home + (0.5, 0.0, -0.4), home + (-1.0, 0.6, 0.2), home + (0.1, 0.1, 0.1)]
    which = [0, 0, 0, 0, 0, 0, 1, 2, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 3, 3, 2, 2, 2, 2, 2, 2, 0, 1, 0, 0, 0, 0, 0, 0, 0]
    cams = _views(api, scene, 8)

    def sequence():
        for k, w in enumerate(which):
            light.position = np.array(spots[w], dtype=np.float64)
            yield cams[k % len(cams)]

    monkeypatch.setenv("MR_SIL_CACHE", "0")
    want = []
    for cam, dbg in sequence():
        scene.camera, scene.debug_camera = cam, dbg
        want.append(scene.render().copy())
    assert backend.sil_cache()[2] == 0
    monkeypatch.delenv("MR_SIL_CACHE")
    got = [f.copy() for f in scene.render_frames(sequence(), depth=depth)]
    assert len(got) == len(want)
    for k in range(len(want)):
        assert np.array_equal(got[k], want[k]), f"depth {depth}: frame {k} (light {which[k]}) differs"
    captures = backend.sil_cache()[2]
    assert captures >= 2, f"the sequence must have gone through the cache ({captures} captures)"
    scene.close()


def test_bands_and_stripes_of_a_cached_frame(api, monkeypatch):
    """The cache is per scene, not per band: row bands and tile-row stripes of cached frames assemble to the whole
    cached frame, which is the fused one."""
    import torch
    from py_numpy_renderer_amd.multigpu import stripe_rows, unstripe
    scene = scenes.build(api, "diablo_floor_small")
    backend = scene._backend()
    monkeypatch.setenv("MR_SIL_CACHE", "0")
    fused = scene.render().copy()
    monkeypatch.delenv("MR_SIL_CACHE")
    for _ in range(3):
        full = scene.render().copy()
    assert _path(backend) == CACHED and np.array_equal(full, fused)
    h = full.shape[0]
    for bands in (2, 3, 8):
        edges = [round(i * h / bands) for i in range(bands + 1)]
        parts = []
        for i in range(bands):
            parts.append(scene.render(row_band=(edges[i], edges[i + 1])).copy())
            assert _path(backend) == CACHED
        assert np.array_equal(np.concatenate(parts, axis=0), full), f"{bands} bands"
    for world in (2, 3, 8):
        parts = []
        for r in range(world):
            parts.append(backend.render(scene, counters=False, stripe=(r, world)).copy())
            assert _path(backend) == CACHED
        assert all(p.shape[0] == stripe_rows(h, world) for p in parts)
        frame = unstripe(torch.from_numpy(np.concatenate(parts, axis=0)), h, world).numpy()
        assert np.array_equal(frame, full), f"{world} stripes"
    # a band as the FIRST frames of a light: the capture of a band's frame serves the whole frame
    scene.light.position = np.array(scene.light.position, dtype=np.float64) + (0.3, 0.2, -0.5)
    monkeypatch.setenv("MR_SIL_CACHE", "0")
    fused = scene.render().copy()
    monkeypatch.delenv("MR_SIL_CACHE")
    for _ in range(3):
        scene.render(row_band=(0, h // 3))
    assert _path(backend) == CACHED
    assert np.array_equal(scene.render(), fused) and _path(backend) == CACHED
    scene.close()


@pytest.mark.parametrize("name", ["diablo_floor_small", "c4_torus200k_1080p"])
def test_the_path_bench_times_is_cached_and_right(api, name, monkeypatch):
    """BandRenderer.step() -- mr_render_device with prepared descriptors, three in flight, the eight swing views:
    after a few frames and one synchronize() the frames that follow read the cache, and are the fused frames."""
    import torch
    from py_numpy_renderer_amd._native import fill_frame_desc
    from py_numpy_renderer_amd._pack import pack_frame
    from py_numpy_renderer_amd.multigpu import BandRenderer
    scene = scenes.build(api, name)
    backend = scene._backend()
    views = _views(api, scene, 8)
    base = scene.camera, scene.debug_camera
    monkeypatch.setenv("MR_SIL_CACHE", "0")
    want = []
    for cam, dbg in views:
        scene.camera, scene.debug_camera = cam, dbg
        want.append(scene.render().copy())
    scene.camera, scene.debug_camera = base
    br = BandRenderer(scene, 0, 1, shadows=True, light_timing=True, frames_in_flight=3, timing_every=0)
    assert backend.sil_cache()[2] == 0
    monkeypatch.delenv("MR_SIL_CACHE")
    descs = []
    for cam, dbg in views:
        scene.camera, scene.debug_camera = cam, dbg
        descs.append(fill_frame_desc(pack_frame(scene, True), br.band, light_timing=True, counters=False, stripe=br.stripe))
    scene.camera, scene.debug_camera = base
    br.set_descriptors(descs)
    for _ in range(6):
        br.step()
    br.synchronize()
    br.step()                                 # (this enqueue sees the capture's event complete)
    assert _path(backend) == CACHED
    first = br.count
    frames = []
    for _ in range(16):
        view, stream = br.count % len(descs), br.lanes[br.count % len(br.lanes)][0]
        frame = br.step()
        with torch.cuda.stream(stream):           # (the copy is taken on the frame's own stream, behind its kernels)
            frames.append((view, frame.clone()))
    assert br.verify()
    torch.cuda.synchronize()
    assert _path(backend) == CACHED and br.count == first + 16
    for view, frame in frames:
        assert np.array_equal(frame.cpu().numpy(), want[view]), f"{name}: view {view} differs"
    scene.close()


def test_list_overflow_on_the_cached_path(api, monkeypatch):
    """A cached frame whose shadow-quad lists are too small reports the overflow like a fused one: the lists grow and
    the frame that follows is right.  (The library sizes the quad records for every edge of the scene, so what a
    caller can make too small are the per-tile quad lists and the work list: mr_scene_set_list_capacities.)"""
    import torch
    from py_numpy_renderer_amd.multigpu import BandRenderer
    scene = scenes.build(api, "diablo_floor_small")
    backend = scene._backend()
    monkeypatch.setenv("MR_SIL_CACHE", "0")
    want = scene.render().copy()
    monkeypatch.delenv("MR_SIL_CACHE")
    for _ in range(3):
        scene.render()
    assert _path(backend) == CACHED
    backend.set_list_capacities(quads=3, work=16)
    # the unsynchronised path first: the overflow must be REPORTED by the cached frame
    out = torch.empty(want.shape, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()
    backend.render_device(scene, out.data_ptr(), stream.cuda_stream, shadows=True)
    stream.synchronize()
    assert _path(backend) == CACHED
    assert backend.overflowed(), "the cached frame must report the overflow of its lists"
    for _ in range(6):
        backend.render_device(scene, out.data_ptr(), stream.cuda_stream, shadows=True)
        stream.synchronize()
        assert _path(backend) == CACHED
        if not backend.overflowed():
            break
    assert np.array_equal(out.cpu().numpy(), want)
    # and through mr_render, which retries by itself
    backend.set_list_capacities(quads=3, work=16)
    assert np.array_equal(scene.render(), want) and _path(backend) == CACHED
    br = BandRenderer(scene, 0, 1, shadows=True, light_timing=True, frames_in_flight=2)
    frames = [br.step() for _ in range(4)]
    assert br.verify()
    torch.cuda.synchronize()
    assert _path(backend) == CACHED
    for frame in frames[-2:]:
        assert np.array_equal(frame.cpu().numpy(), want)
    scene.close()
