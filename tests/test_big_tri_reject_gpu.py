"""GPU: ``MR_BIG_TRI_REJECT=0 | 1`` -- ``k_bin_work`` lists a large triangle in every tile of its box, or only in the
tiles it can cover (``tri_touches_tile``, csrc/tri_reject.h; test_big_tri_reject_cpu.py holds the rule itself to the
coverage test sample by sample).  A rejected (triangle, tile) pair held no covered sample, so the two settings must be
indistinguishable but for the lists' lengths: the uint8 frame, z, winner and stencil equal bit for bit and every counted
statistic equal except ``tri_bin_entries``, which is smaller by exactly ``mr_debug_big_tri_rejects`` -- and strictly
smaller wherever a floor is drawn, whose two triangles are listed on the wrong side of their shared diagonal otherwise.

The variable is looked up for every frame, so one process renders both.  Small scenes with large triangles:
diablo_floor at 270x480, torus_spot at 180x320, cube_outward at 120x160 and a synthetic one at 240x320: a fan of long
thin triangles across one diagonal, a second fan of a ``depth_test=False`` model across the other, three triangles with
a corner behind the camera (``TF_CLIP``) and the two-triangle floor.  The synthetic scene is also rendered as a row band,
as stripe (1, 3), supersampled 2x and under two lights.
"""
import os

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

SWITCH = "MR_BIG_TRI_REJECT"
SCENES = ["diablo_floor_small", "torus_spot", "cube_outward", "fans"]
VARIANTS = ["band", "stripe", "ss2", "two_lights"]


def _camera_point(x, y, d):
    """World position *d* along the standard camera's axis, *x* to its right and *y* up (the camera of _std_cameras)."""
    eye = np.array([0.5, 1.0, 2.0])
    fwd = -eye / np.linalg.norm(eye)
    right = np.cross(fwd, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    return eye + fwd * d + right * x + up * y


def _obj(name, triangles):
    lines = []
    for tri in triangles:
        for p in tri:
            lines.append("v %.6f %.6f %.6f" % tuple(p))
    lines += ["vt 0 0", "vt 1 0", "vt 0.5 1"]
    for i in range(len(triangles)):
        lines.append("f %d/1/ %d/2/ %d/3/" % (3 * i + 1, 3 * i + 2, 3 * i + 3))
    return scenes._write_if_changed(os.path.join(scenes.GENERATED, name), "\n".join(lines) + "\n")


def fans(api, resolution=(240, 320)):
    """At depth 2.3 the frame spans about +-1.77 x +-1.33 camera units."""
    fan = []                 # bottom left to top right, each a few pixels wide and some twenty tiles long
    apex = _camera_point(-1.6, -1.15, 2.3)
    for i in range(10):
        a = np.deg2rad(18 + 4.5 * i)
        end = _camera_point(-1.6 + 3.6 * np.cos(a), -1.15 + 3.6 * np.sin(a), 2.0 + 0.08 * i)
        end2 = _camera_point(-1.6 + 3.6 * np.cos(a + 0.012), -1.15 + 3.6 * np.sin(a + 0.012), 2.0 + 0.08 * i)
        fan.append((apex, end, end2))
    ghost = []               # top left to bottom right: tested against z, never written to it
    apex = _camera_point(-1.5, 1.2, 2.6)
    for i in range(4):
        a = np.deg2rad(-25 - 6 * i)
        end = _camera_point(-1.5 + 3.4 * np.cos(a), 1.2 + 3.4 * np.sin(a), 2.2)
        end2 = _camera_point(-1.5 + 3.4 * np.cos(a - 0.02), 1.2 + 3.4 * np.sin(a - 0.02), 2.2)
        ghost.append((apex, end, end2))
    behind = []              # one corner behind the camera: the per-fragment clip test, TF_CLIP
    for i in range(3):
        behind.append((_camera_point(-1.0 + 0.5 * i, 0.9, 2.0), _camera_point(-0.85 + 0.5 * i, 0.8, 2.0),
                       _camera_point(0.3 + 0.2 * i, -0.3, -0.5)))
    cam, dbg = scenes._std_cameras(api, backface_culling=False)
    m_fan = api.Model.load_model(_obj("reject_fan.obj", fan))
    m_ghost = api.Model.load_model(_obj("reject_ghost.obj", ghost))
    m_ghost.depth_test = False
    m_behind = api.Model.load_model(_obj("reject_behind.obj", behind))
    return scenes._scene(api, cam, dbg, scenes._std_light(api), resolution,
                         [m_fan, m_ghost, m_behind, scenes._floor(api, textured=False)])


def _build(api, name):
    return fans(api) if name == "fans" else scenes.build(api, name)


def _counted(backend, scene, **kw):
    got = dict(out=backend.render(scene, shadows=True, **kw).copy(), z=backend.read_z().view(np.uint64),
               winner=backend.read_winner(), stencil=backend.read_stencil())
    stats = {k: v for k, v in backend.last_stats.items() if not k.startswith("gpu_ms")}
    return got, stats, backend.big_tri_rejects()


def _both(scene, **kw):
    """The same counted frame with the switch off and on: ((buffers, stats, rejects) off, (...) on)."""
    backend = scene._backend()
    before = os.environ.get(SWITCH)
    try:
        pair = []
        for value in ("0", "1"):
            os.environ[SWITCH] = value
            pair.append(_counted(backend, scene, **kw))
        return pair
    finally:
        if before is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = before


def _compare(label, off, on, floor=True):
    (buf0, st0, rej0), (buf1, st1, rej1) = off, on
    print(f"{label}: tri_bin_entries {st0['tri_bin_entries']} -> {st1['tri_bin_entries']}, rejected pairs {rej0} -> {rej1}, "
          f"frag_tri {st0['frag_tri']}, covered_px {st0['covered_px']}")
    assert buf0["out"].size and buf0["out"].max() > buf0["out"].min(), f"{label}: an empty frame"
    for key in buf0:
        assert np.array_equal(buf0[key], buf1[key]), f"{label}: {key} differs"
    for key in st0:
        if key != "tri_bin_entries":
            assert st0[key] == st1[key], f"{label}: {key} {st0[key]} -> {st1[key]}"
    assert st0["frag_tri"] > 0 and st0["covered_px"] > 0, label
    assert rej0 == 0, f"{label}: {rej0} pairs rejected with the switch off"
    assert st0["tri_bin_entries"] - st1["tri_bin_entries"] == rej1, f"{label}: the lists shrank by another number than was counted"
    if floor:
        assert st1["tri_bin_entries"] < st0["tri_bin_entries"], f"{label}: nothing rejected"


@pytest.mark.parametrize("name", SCENES)
def test_whole_frames_do_not_depend_on_the_switch(api, name):
    scene = _build(api, name)
    try:
        off, on = _both(scene)
        _compare(name, off, on)
        # the frame-only kernels (every scene but the one with a depth_test=False model takes them here)
        backend = scene._backend()
        frames = []
        for value in ("0", "1"):
            os.environ[SWITCH] = value
            frames.append(backend.render(scene, shadows=True, counters=False).copy())
        os.environ.pop(SWITCH, None)
        assert np.array_equal(frames[0], frames[1]), f"{name}: the frame-only frames differ"
        assert np.array_equal(frames[0], off[0]["out"]), f"{name}: frame-only and counted frames differ"
    finally:
        os.environ.pop(SWITCH, None)
        scene.close()


@pytest.mark.parametrize("what", VARIANTS)
def test_partial_supersampled_and_two_light_frames(api, what):
    scene = fans(api)
    try:
        h = int(scene.resolution[0])
        kw = {}
        if what == "band":
            kw["row_band"] = (h // 3, 2 * h // 3)
        elif what == "stripe":
            kw["stripe"] = (1, 3)
        elif what == "ss2":
            scene.supersample = 2
        else:
            scene.add_light(api.Light((-2, 3, 1), ambient_strength=0.1, specular_strength=0.1))
        off, on = _both(scene, **kw)
        _compare(f"fans {what}", off, on)
    finally:
        scene.close()
