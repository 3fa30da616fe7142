"""GPU: shading inputs that the other suites hold constant -- texture shapes, the light's colour, attenuation and
ambient strength, a colour sky, the cameras' viewport offsets (scenes.py, "shading inputs").

The four captures torus_rect_maps, quad_rect_object_nm, cube_skybox_offset and torus_spot_offset_sky run through every
SMALL-parametrised suite (capture, oracle, frame-only mode, face status).  This module covers the paths where the
same inputs are handled by OTHER code: the sample grid of a supersampled frame, the multi-light instantiations, split
frames, the empty-tile fast path that writes the finalised background, the host's change detection between two frames
of one renderer, the pose pass and float64 vertices, and a seeded sweep over map shapes down to 2 x 1.

The sequential C oracle is the yardstick; the CPU suite pins it to the reference on these inputs (test_oracle_golden.py,
and a sweep of 60 seeds of ``scenes.shading_sweep`` whose outcome DESIGN.md gives).  Bars, the project's: z bits, winners
and stencil exact, float frame 2e-6 (n * 2e-6 + 1e-6 under n lights), uint8 +-1.
"""

import numpy as np
import pytest

import pose_ref
import scenes
from multilight_ref import compose
from supersample_ref import max_diff, resolve

pytestmark = pytest.mark.gpu

SWEEP_SEEDS = tuple(range(8))


def _taps(backend):
    return dict(z=backend.read_z(), winner=backend.read_winner(), stencil=backend.read_stencil(),
                frame=backend.read_frame_f32())


def assert_matches(got, out, want, label):
    """The project's bars against an oracle result."""
    bad_z = int((got["z"].view(np.uint64) != want.z.view(np.uint64)).sum())
    assert bad_z == 0, f"{label}: {bad_z} z-buffer entries not bit-exact"
    assert int((got["winner"] != want.winner).sum()) == 0, f"{label}: winner map differs"
    assert int((got["stencil"] != want.stencil).sum()) == 0, f"{label}: stencil differs"
    err = np.abs(got["frame"].astype(np.float64) - want.frame.astype(np.float64))
    print(f"{label}: float frame off by {err.max():.3g}")
    assert err.max() <= 2e-6, f"{label}: float frame off by {err.max():.3g} at {np.argwhere(err == err.max())[0]}"
    d = np.abs(out.astype(np.int16) - want.out.astype(np.int16))
    assert d.max() <= 1, f"{label}: uint8 frame off by {d.max()} ({int((d > 1).sum())} values > 1)"


def _against_oracle(oracle_mod, scene, label):
    """Counted frame against the oracle, and the frame-only mode against the counted frame."""
    backend = scene._backend()
    out = backend.render(scene, keep_float=True).copy()
    want = oracle_mod.render(scene)
    assert_matches(_taps(backend), out, want, label)
    assert np.array_equal(scene.render(), out), f"{label}: frame-only mode differs"
    return out, want


def _background_u8(colour):
    return (np.asarray(colour, dtype=np.float32) ** 0.8 * 255).astype(np.uint8)


# ---------------------------------------------------------------------------- 1. the sample grid
def _supersampled(api, fn, s):
    """(the recipe with supersample = s, its twin at (s*H, s*W) with both cameras' offsets times s)."""
    scene = fn(api)
    h, w = scene.resolution
    ox, oy = scene.camera.x_offset, scene.camera.y_offset
    assert ox and oy
    twin = fn(api, resolution=(s * h, s * w), offsets=(s * ox, s * oy))
    scene.supersample = s
    return scene, twin


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("name", ["torus_spot_offset_sky", "cube_skybox_offset"])
def test_supersampled_frame_is_the_resolved_twin(api, oracle_mod, name, s):
    """Offsets times s, the cubemap's two triangles and rays on the sample grid, background samples resolved from the
    float background: the frame is the oracle's sample grid box-filtered (+-1), and the grid's z, winners and stencil
    are the oracle's bit for bit."""
    scene, twin = _supersampled(api, getattr(scenes, name), s)
    backend = scene._backend()
    out = backend.render(scene).copy()
    r = oracle_mod.render(twin)
    worst, n_one = max_diff(out, resolve(r.frame, s))
    assert worst <= 1, f"{name} s={s}: max diff {worst}, {n_one} pixels off by one"
    assert np.array_equal(backend.read_z().view(np.uint64), r.z.view(np.uint64)), "z-buffer not bit-exact"
    assert np.array_equal(backend.read_winner(), r.winner), "winner map differs"
    assert np.array_equal(backend.read_stencil(), r.stencil), "stencil differs"
    assert np.array_equal(scene.render(), out), "frame-only mode differs"
    scene.close()


# ---------------------------------------------------------------------------- 2. more than one light
def test_rect_maps_under_three_coloured_lights(api, oracle_mod):
    """torus_rect_maps' own light plus a coloured spot light and a coloured directional light with attenuations of their
    own, against multilight_ref.compose: the multi-light instantiations of the set-up and tile kernels read every
    light's colour, ambient colour and three attenuation terms from its own record."""
    scene = scenes.torus_rect_maps(api)
    scene.add_light(api.Light((-1.2, 2.0, 1.0), light_type=api.Lightning.SPOT_LIGHTNING, center=(0, 0, 0),
                              color=(0.3, 1.0, 0.6), ambient_strength=0.15, specular_strength=0.3,
                              constant=0.8, linear=0.02, quadratic=0.21))
    scene.add_light(api.Light((0.5, 3.0, -2.0), light_type=api.Lightning.DIRECTIONAL_LIGHTNING, center=(0, 0, 0),
                              color=(0.5, 0.4, 1.0), ambient_strength=0.05, specular_strength=0.5,
                              constant=1.4, linear=0.25, quadratic=0.01))
    n = len(scene.lights)
    assert n == 3
    ref = compose(oracle_mod, scene)
    covered = ref.winner >= 0
    for k, r in enumerate(ref.per):                  # every light shows: no single one gives the composed frame
        assert int(((ref.out != r.out).any(axis=-1) & covered[::-1]).sum()) >= 1000, k
    backend = scene._backend()
    out = backend.render(scene, keep_float=True).copy()
    worst, _ = max_diff(out, ref.out)
    assert worst <= 1, f"uint8 frame off by {worst}"
    err = float(np.abs(backend.read_frame_f32().astype(np.float64) - ref.frame.astype(np.float64)).max())
    print(f"float frame: max error {err:.3g} (bound {n * 2e-6 + 1e-6:.3g})")
    assert err <= n * 2e-6 + 1e-6, f"float frame off by {err:.3g}"
    assert np.array_equal(backend.read_z().view(np.uint64), ref.z.view(np.uint64)), "z-buffer not bit-exact"
    assert np.array_equal(backend.read_winner(), ref.winner), "winner map differs"
    for k, r in enumerate(ref.per):
        assert np.array_equal(backend.read_stencil(light=k), r.stencil), f"stencil of light {k} differs"
    assert np.array_equal(scene.render(), out), "frame-only mode differs"
    scene.close()


# ---------------------------------------------------------------------------- 3. split frames
def test_bands_and_stripes_of_a_shifted_frame(api):
    """Three row bands cut off the tile grid and three tile-row stripes of torus_spot_offset_sky, assembled: exactly the
    single-device frame (the offsets enter every device's pixel boxes and cluster records, the sky colour its
    background)."""
    import torch
    from py_numpy_renderer_amd.multigpu import stripe_rows, unstripe
    scene = scenes.build(api, "torus_spot_offset_sky")
    backend = scene._backend()
    full = scene.render().copy()
    h = full.shape[0]
    cuts = (0, 53, 121, h)
    parts = [scene.render(row_band=(cuts[i], cuts[i + 1])).copy() for i in range(3)]
    assert np.array_equal(np.concatenate(parts, axis=0), full), "row bands"
    parts = [backend.render(scene, counters=False, stripe=(r, 3)).copy() for r in range(3)]
    assert all(p.shape[0] == stripe_rows(h, 3) for p in parts)
    frame = unstripe(torch.from_numpy(np.concatenate(parts, axis=0)), h, 3).numpy()
    assert np.array_equal(frame, full), "stripes"
    scene.close()


# ---------------------------------------------------------------------------- 4. the background
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("sky", [(0.9, 0.3, 0.1), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.25, 0.5, 0.75)])
def test_colour_sky_is_uniform(api, sky, s):
    """Every pixel no face covers has one and the same uint8 value -- no seam between the tiles nothing is binned to,
    which take the finalised background from the host, and the uncovered pixels of tiles that are shaded -- and that
    value is upstream's ``(float32(colour) ** 0.8 * 255).astype(uint8)`` within 1.  With supersample = 2 a pixel counts
    as uncovered when its four samples are."""
    scene = scenes.torus_spot_offset_sky(api, sky=sky)
    scene.supersample = s
    backend = scene._backend()
    counted = backend.render(scene).copy()
    winner = backend.read_winner()
    h, w = scene.resolution
    assert winner.shape == (s * h, s * w)
    empty = (winner.reshape(h, s, w, s) < 0).all(axis=(1, 3))               # rows bottom-up like the buffers
    tiles = empty[:h // 16 * 16, :w // 16 * 16].reshape(h // 16, 16, w // 16, 16)
    empty = empty[::-1]                                                       # rows top-down like the frame
    assert tiles.all(axis=(1, 3)).any() and (tiles.any(axis=(1, 3)) & ~tiles.all(axis=(1, 3))).any(), \
        "the frame needs both empty tiles and partly covered ones"
    want = _background_u8(sky)
    for label, frame in (("counted", counted), ("frame-only", scene.render())):
        values = np.unique(frame[empty].reshape(-1, 3), axis=0)
        assert len(values) == 1, f"{label}: {len(values)} different background colours, e.g. {values[:4].tolist()}"
        assert np.abs(values[0].astype(int) - want.astype(int)).max() <= 1, (label, values[0].tolist(), want.tolist())
    scene.close()


# ---------------------------------------------------------------------------- 5. changes between two frames
def _overlay_expected(oracle_mod, scene):
    from py_numpy_renderer_amd.frustums import draw_view_frustum
    r = oracle_mod.render(scene)
    frame, z = r.frame.copy(), r.z.copy()
    draw_view_frustum(frame, scene.camera, scene.debug_camera, z, scene.system)
    return oracle_mod.finalise(frame), oracle_mod.finalise(r.frame)


def test_changed_inputs_reach_the_device(api, oracle_mod):
    """One renderer, one input changed per frame, every frame against the oracle: a map replaced by the array of its
    transpose's shape (the same bytes and byte count), the light's colour, linear <-> quadratic, the viewport offsets (the
    cameras stay the same objects) with and without the debug-frustum overlay, the sky colour, and the sky going from a
    colour to none, to the cubemap and back.  Each frame must differ from the one before it: a cached frame constant,
    texture header or overlay list that survived the change would show the old frame."""
    scene = scenes.torus_rect_maps(api, resolution=(136, 152))
    torus = scene.models[0].materials["default"]
    frames = [_against_oracle(oracle_mod, scene, "first frame")[0]]

    def step(label):
        out, _ = _against_oracle(oracle_mod, scene, label)
        assert not np.array_equal(out, frames[-1]), f"{label}: the frame did not change"
        frames.append(out)

    assert torus.map_Kd.shape == (40, 96, 3)
    torus.map_Kd = torus.map_Kd.reshape(96, 40, 3)
    step("diffuse map (40, 96, 3) -> (96, 40, 3)")
    torus.norm = torus.norm.reshape(40, 96, 3)
    assert torus.is_tangent_space("norm")
    step("normal map (96, 40, 3) -> (40, 96, 3)")
    scene.light.color = np.array((0.2, 0.6, 1.0))
    step("light.color")
    scene.light.linear, scene.light.quadratic = scene.light.quadratic, scene.light.linear
    step("linear <-> quadratic")
    scene.light.ambient = np.array((0.05, 0.3, 0.1))
    step("light.ambient")
    cameras = (scene.camera, scene.debug_camera)
    for cam in cameras:
        cam.x_offset, cam.y_offset = -31, -17
    step("offsets")
    assert (scene.camera, scene.debug_camera) == cameras
    # the overlay's lines go through camera.viewport: first drawn under these offsets, then under others
    scene.draw_debug_frustum = True
    for offsets in ((-31, -17), (-12, -40)):
        for cam in cameras:
            cam.x_offset, cam.y_offset = offsets
        out = scene.render().copy()
        with_lines, plain = _overlay_expected(oracle_mod, scene)
        assert (with_lines != plain).any(), "the overlay drew nothing"
        worst, _ = max_diff(out, with_lines)
        assert worst <= 1, f"overlay under offsets {offsets}: max diff {worst}"
    scene.draw_debug_frustum = False
    step("offsets again")
    scene.skybox = (0.1, 0.8, 0.4)
    step("sky: none -> colour")
    scene.skybox = (0.8, 0.1, 0.4)
    step("sky: another colour")
    scene.skybox = None
    step("sky: colour -> none")
    scene.skybox = scenes._cubemap(api)
    step("sky: none -> cubemap")
    scene.skybox = [0.8, 0.1, 0.4]
    step("sky: cubemap -> colour")
    scene.close()


# ---------------------------------------------------------------------------- 6. model state
def test_pose_and_f64_vertices_under_rect_maps(api, oracle_mod):
    """torus_rect_maps with its torus posed (the pose pass writes float64 positions; texel look-ups keep the maps'
    shapes) against the oracle of the twin, and with float64 vertices (``Model @`` a float64 matrix) against the oracle."""
    recipe = (lambda a: scenes.torus_rect_maps(a, resolution=(136, 152)), 0)
    matrix = pose_ref.matrices(api)["product"]
    scene, index = pose_ref.build(api, recipe)
    backend = scene._backend()
    plain = backend.render(scene, keep_float=True).copy()
    scene.models[index].pose = matrix
    out = backend.render(scene, keep_float=True).copy()
    taps = _taps(backend)
    assert not np.array_equal(out, plain), "the pose changed nothing"
    twin = pose_ref.twin(api, recipe, matrix)
    assert_matches(taps, out, oracle_mod.render(twin), "posed torus")
    assert np.array_equal(scene.render(), out)
    scene.close(), twin.close()

    scene = scenes.torus_rect_maps(api, resolution=(136, 152))
    moved = scene.models[0] @ (api.rotate_xyz((3.0, -2.0, 1.5)) @ api.scale(1.0))
    assert moved.vertices.dtype == np.float64 and moved.materials["default"].map_Kd.shape == (40, 96, 3)
    scene.models[0] = moved
    _against_oracle(oracle_mod, scene, "float64 torus")
    scene.close()


# ---------------------------------------------------------------------------- 7. seeded sweep
@pytest.mark.parametrize("seed", SWEEP_SEEDS)
def test_sweep_seed_matches_oracle(api, oracle_mod, seed):
    """scenes.shading_sweep: map shapes from 2 x 1 to 97 x 97 texels (2 x N, N x 1 and 2 x 1 among them), a light kind,
    colour and attenuation, offsets within half the frame, a sky colour in [0, 1]."""
    scene = scenes.shading_sweep(api, seed)
    p = scenes.shading_sweep_parameters(seed)
    _, want = _against_oracle(oracle_mod, scene, f"sweep seed {seed} {p['shapes']} offsets {p['offsets']}")
    assert (want.winner >= 0).sum() >= 500, "next to nothing of the scene is in the frame"
    scene.close()

