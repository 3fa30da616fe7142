"""Several shadow-casting lights in one frame on the device (``Scene.add_light``; ``mr_scene_set_extra_lights``).

The expected frame is ``multilight_ref.compose``: the oracle's float frame of the scene under every light alone, added
in float32 in the order of the lights where a face covers the pixel and clamped to 1, then upstream's finalise.  Bars:
uint8 +-1 per channel (the project's); float frame n * 2e-6 + 1e-6 (the project's 2e-6 per light's frame, plus one
float32 ulp of a sum below 4); z, winner, every light's stencil, silhouette and counters exact."""
import numpy as np
import pytest

import scenes
from multilight_ref import compose, extra_lights
from supersample_ref import max_diff, pair, resolve

pytestmark = pytest.mark.gpu

SCENES = ["cube_small", "diablo_small", "diablo_floor", "diablo_floor_lh_gl", "torus_spot", "cube_skybox",
          "cube_tetra_nodepth", "kat_house", "fins_nonmanifold", "tetra_ortho", "wall_nine_materials"]
FUSED, CAPTURE, CACHED = 0, 1, 2


def _lit(api, name, n, **kw):
    scene = getattr(scenes, name)(api, **kw)
    for light in extra_lights(api)[:n - 1]:
        scene.add_light(light)
    assert len(scene.lights) == n
    return scene


def _px_differ(a, b, mask=None):
    d = (a != b).any(axis=-1)
    return int((d & mask).sum()) if mask is not None else int(d.sum())


@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("name", SCENES)
def test_frame_matches_the_composed_reference(api, oracle_mod, name, n):
    scene = _lit(api, name, n)
    ref = compose(oracle_mod, scene)
    covered = ref.winner >= 0
    n_covered = int(covered.sum())
    # -- the reference must be one that clamping, or ignoring a light, cannot pass
    saturated = int(((ref.frame == 1.0).all(axis=-1) & covered).sum())
    print(f"{name} n={n}: covered {n_covered}, saturated {saturated / max(n_covered, 1):.3f}")
    assert saturated <= 0.5 * n_covered, f"{saturated} of {n_covered} covered pixels are white"
    floor = 300 if name == "diablo_floor_lh_gl" else 1000
    for k, r in enumerate(ref.per):
        differ = _px_differ(ref.out, r.out, covered[::-1])
        print(f"  composed vs light {k} alone: {differ} covered pixels differ")
        assert differ >= floor, f"light {k} alone is the composed frame but for {differ} pixels"
    if n == 4:
        assert any((ref.stencils[a][covered] != ref.stencils[b][covered]).any() for a in range(4) for b in range(a)), \
            "every light has the same stencil at the covered pixels"

    # -- the counted frame: everything exact but the colour
    backend = scene._backend()
    out = backend.render(scene, keep_float=True)
    st = dict(backend.last_stats)
    worst, n_one = max_diff(out, ref.out)
    print(f"  uint8: max diff {worst}, {n_one} pixels off by one")
    assert worst <= 1, f"uint8 frame off by {worst}"
    frame = backend.read_frame_f32()
    err = float(np.abs(frame.astype(np.float64) - ref.frame.astype(np.float64)).max())
    print(f"  float frame: max error {err:.3g} (bound {n * 2e-6 + 1e-6:.3g})")
    assert err <= n * 2e-6 + 1e-6, f"float frame off by {err:.3g}"
    assert np.array_equal(backend.read_z().view(np.uint64), ref.z.view(np.uint64)), "z-buffer not bit-exact"
    assert np.array_equal(backend.read_winner(), ref.winner), "winner map differs"
    stencils = []
    for k, r in enumerate(ref.per):
        stencils.append(backend.read_stencil(light=k))
        assert np.array_equal(stencils[k], r.stencil), f"stencil of light {k} differs"
        sil = backend.read_silhouette(light=k)
        assert len(sil) == r.stats["n_quads"], f"silhouette of light {k}: {len(sil)} edges, oracle {r.stats['n_quads']}"
        assert set(map(tuple, sil.tolist())) == set(map(tuple, r.silhouette.tolist())), f"silhouette of light {k} differs"
    assert np.array_equal(backend.read_stencil(), stencils[0]) and len(backend.read_silhouette()) == len(backend.read_silhouette(light=0))
    assert st["frag_tri"] == ref.per[0].stats["frag_tri_pass1"]
    assert st["covered_px"] == n_covered
    for key in ("frag_quad", "n_quads", "n_quads_drawn", "stencil_updates"):
        assert st[key] == sum(r.stats[key] for r in ref.per), key
    assert st["lit_px"] == sum(int((covered & (r.stencil == 0)).sum()) for r in ref.per)

    # -- frame-only mode (how Scene.render() runs): the same frame; stencils need only agree where a face is drawn
    fast = backend.render(scene, keep_float=True, counters=False, keep_buffers=True)
    assert np.array_equal(fast, out)
    assert np.array_equal(backend.read_frame_f32().view(np.uint32), frame.view(np.uint32))
    assert np.array_equal(backend.read_z().view(np.uint64), ref.z.view(np.uint64))
    assert np.array_equal(backend.read_winner(), ref.winner)
    for k in range(n):
        assert np.array_equal(backend.read_stencil(light=k)[covered], stencils[k][covered]), f"frame-only stencil of light {k}"
    assert np.array_equal(scene.render(), out)

    # -- and it is not the device's own single-light frame
    solo = getattr(scenes, name)(api)
    assert _px_differ(out, solo.render()) > 0
    solo.close()
    scene.close()


def test_clear_lights_gives_the_plain_frame_back(api):
    a, b = _lit(api, "diablo_floor", 3), scenes.diablo_floor(api)
    lit = a.render().copy()
    a.clear_lights()
    plain = b.render()
    assert np.array_equal(a.render(), plain)
    assert _px_differ(lit, plain) > 0
    ba, bb = a._backend(), b._backend()
    fa, fb = ba.render(a, keep_float=True), bb.render(b, keep_float=True)
    assert np.array_equal(fa, fb) and np.array_equal(ba.read_frame_f32().view(np.uint32), bb.read_frame_f32().view(np.uint32))
    assert np.array_equal(ba.read_stencil(), bb.read_stencil())
    assert ba.last_stats["n_quads"] == bb.last_stats["n_quads"] and ba.last_stats["lit_px"] == bb.last_stats["lit_px"]
    a.close(), b.close()


@pytest.mark.parametrize("name", ["diablo_floor", "torus_spot"])
def test_swapping_two_lights_swaps_their_stencils(api, oracle_mod, name):
    warm, blue, _ = extra_lights(api)
    a, b = getattr(scenes, name)(api), getattr(scenes, name)(api)
    a.add_light(warm), a.add_light(blue)
    b.add_light(blue), b.add_light(warm)
    ba, bb = a._backend(), b._backend()
    fa, fb = ba.render(a), bb.render(b)
    assert np.array_equal(ba.read_stencil(light=0), bb.read_stencil(light=0))
    assert np.array_equal(ba.read_stencil(light=1), bb.read_stencil(light=2))
    assert np.array_equal(ba.read_stencil(light=2), bb.read_stencil(light=1))
    assert (ba.read_stencil(light=1) != ba.read_stencil(light=2)).any()
    assert set(map(tuple, ba.read_silhouette(light=1).tolist())) == set(map(tuple, bb.read_silhouette(light=2).tolist()))
    assert max_diff(fa, fb)[0] <= 1
    assert max_diff(fb, compose(oracle_mod, b).out)[0] <= 1
    a.close(), b.close()


def test_single_light_frames_around_a_four_light_frame(api, oracle_mod):
    """One scene handle: single-light frames, a four-light frame, single-light frames again -- the same bytes, and the
    silhouette cache (keyed on one light) still captures for and serves the single-light frames."""
    scene = scenes.diablo_floor(api)
    backend = scene._backend()
    first = scene.render().copy()
    paths = [backend.sil_cache()[0]]
    for _ in range(2):
        assert np.array_equal(scene.render(), first)
        paths.append(backend.sil_cache()[0])
    # (a first frame that outgrew a work list is rendered twice, and the repeat already captures)
    assert CAPTURE in paths and paths[-1] == CACHED, paths
    captures = backend.sil_cache()[2]
    assert captures >= 1
    for light in extra_lights(api):
        scene.add_light(light)
    four = scene.render().copy()
    assert backend.sil_cache()[:2] == (FUSED, 0), "a frame with several lights neither reads nor fills the cache"
    assert backend.sil_cache()[2] == captures
    assert max_diff(four, compose(oracle_mod, scene).out)[0] <= 1
    scene.clear_lights()
    again = scene.render()
    assert np.array_equal(again, first)
    assert backend.sil_cache()[0] == CACHED and backend.sil_cache()[1] > 0
    scene.close()
    # a scene whose first single-light frames come after a multi-light one still captures
    scene = _lit(api, "diablo_floor", 4)
    backend = scene._backend()
    assert np.array_equal(scene.render(), four)
    scene.clear_lights()
    paths = []
    for _ in range(3):
        assert np.array_equal(scene.render(), first)
        paths.append(backend.sil_cache()[0])
    assert CAPTURE in paths and paths[-1] == CACHED, paths
    scene.close()


@pytest.mark.parametrize("name", ["cube_outward", "diablo_small"])
def test_overlay_is_drawn_once_on_the_summed_frame(api, oracle_mod, name):
    scene = _lit(api, name, 3)
    plain = scene.render().copy()
    scene.draw_debug_frustum = True
    out = scene.render()
    want = compose(oracle_mod, scene, overlay=True).out
    worst, n_one = max_diff(out, want)
    assert worst <= 1, f"{name}: max diff {worst}, {n_one} pixels off by one"
    assert _px_differ(out, plain) > 0, "the overlay changed nothing"
    scene.close()


@pytest.mark.parametrize("name", ["diablo_small", "cube_skybox"])
def test_supersampled_frame_sums_per_sample(api, oracle_mod, name):
    scene, twin = pair(api, name, 2)
    for sc in (scene, twin):
        for light in extra_lights(api)[:2]:
            sc.add_light(light)
    out = scene.render()
    ref = compose(oracle_mod, twin)
    want = resolve(ref.frame, 2)
    worst, n_one = max_diff(out, want)
    assert worst <= 1, f"{name}: max diff {worst}, {n_one} pixels off by one"
    backend = scene._backend()
    backend.render(scene)                                     # the taps stay on the sample grid
    for k, r in enumerate(ref.per):
        assert np.array_equal(backend.read_stencil(light=k), r.stencil), f"stencil of light {k}"
    scene.close()


def test_render_frames_with_a_light_that_moves_every_frame(api):
    scene = _lit(api, "diablo_small", 3)
    mover = scene.lights[1]
    cams = [api.Camera((0.5 + 0.15 * np.sin(k), 1.0, 2.0 - 0.05 * k), (0, 0, 0), fovy=60, near=0.1, far=20,
                       backface_culling=True) for k in range(8)]
    dbg = scene.debug_camera

    def place(k):
        mover.set_position(np.array((-3.0 + 0.4 * k, 2.5, 1.5 - 0.2 * k)))

    def views():
        for k, cam in enumerate(cams):
            place(k)
            yield cam, dbg
    # (the synchronous frames first, as in test_silhouette_cache: they also grow the work lists, and a pipelined frame
    # that outgrows one is rendered again with the scene's lights as they are by then)
    sync = []
    for k, cam in enumerate(cams):
        place(k)
        scene.camera, scene.debug_camera = cam, dbg
        sync.append(scene.render().copy())
    piped = [f.copy() for f in scene.render_frames(views(), depth=3)]
    assert len(piped) == 8
    differ = [k for k, (p, q) in enumerate(zip(piped, sync)) if not np.array_equal(p, q)]
    assert not differ, f"frames {differ} differ"
    assert all(_px_differ(sync[0], f) > 0 for f in sync[1:])
    # the light alone moves the frame (host caches included)
    scene.camera, scene.debug_camera = cams[0], dbg
    place(0)
    a = scene.render().copy()
    place(5)
    assert _px_differ(a, scene.render()) > 0
    scene.close()


@pytest.mark.parametrize("name", ["diablo_floor", "torus_spot"])
def test_shadows_off_sums_the_lit_frames(api, oracle_mod, name):
    scene = _lit(api, name, 4)
    out = scene.render(shadows=False)
    want = compose(oracle_mod, scene, shadows=False)
    assert max_diff(out, want.out)[0] <= 1
    assert all(not s.any() for s in want.stencils)
    assert _px_differ(out, scene.render()) > 0
    scene.close()


def test_row_band(api):
    scene = _lit(api, "diablo_floor", 3)
    whole = scene.render().copy()
    h = whole.shape[0]
    for band in ((0, 96), (96, h), (48, 160)):
        assert np.array_equal(scene.render(row_band=band), whole[band[0]:band[1]]), band
    scene.close()


def test_quad_list_overflow_still_ends_in_the_right_frame(api, oracle_mod):
    scene = _lit(api, "diablo_floor", 4)
    want = compose(oracle_mod, scene)
    backend = scene._backend()
    backend.sync_scene(scene)
    backend.set_list_capacities(quads=2)                      # every tile under the shadow volumes overflows
    out = backend.render(scene)
    assert max_diff(out, want.out)[0] <= 1
    for k, r in enumerate(want.per):
        assert np.array_equal(backend.read_stencil(light=k), r.stencil), f"stencil of light {k}"
    assert np.array_equal(scene.render(), out)
    scene.close()


def test_full_size_c4_with_three_lights(api, oracle_mod):
    scene = _lit(api, "torus_floor", 3)
    out = scene.render()
    want = compose(oracle_mod, scene, want_status=False, want_silhouette=False)
    worst, n_one = max_diff(out, want.out)
    assert worst <= 1, f"c4 with three lights: max diff {worst}, {n_one} pixels off by one"
    scene.close()
