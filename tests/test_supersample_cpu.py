"""Supersampled anti-aliasing (``Scene.supersample``), host side: the setting, the frame constants of the sample
grid, the ABI flags, the refusals that need no device, and the NumPy resolve the GPU tests compare against."""
import os
import re

import numpy as np
import pytest

import scenes
from supersample_ref import pair, resolve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("s", [1, 2, 4])
def test_supersample_accepts_1_2_4(api, s):
    assert api.Scene(supersample=s).supersample == s
    scene = api.Scene()
    scene.supersample = s
    assert scene.supersample == s


def test_supersample_defaults_to_1(api):
    assert api.Scene().supersample == 1


@pytest.mark.parametrize("bad", [0, 3, 8, 2.0, "2", -2, True, None])
def test_supersample_rejects_other_values(api, bad):
    with pytest.raises(ValueError):
        api.Scene(supersample=bad)
    scene = api.Scene()
    with pytest.raises(ValueError):
        scene.supersample = bad
    assert scene.supersample == 1


def _fields(pf):
    from dataclasses import fields
    return {f.name: getattr(pf, f.name) for f in fields(pf) if f.name != "supersample"}


def _assert_same_frame(a, b):
    fa, fb = _fields(a), _fields(b)
    assert fa.keys() == fb.keys()
    for k in fa:
        va, vb = fa[k], fb[k]
        if isinstance(va, np.ndarray) or isinstance(vb, np.ndarray):
            assert va is not None and vb is not None, k
            assert va.dtype == vb.dtype and np.array_equal(va, vb), k
        else:
            assert va == vb, k


@pytest.mark.parametrize("name,offsets", [("cube_small", (0, 0)), ("cube_small", (7, -3)), ("cube_skybox", (0, 0)),
                                          ("cube_skybox", (5, 2)), ("diablo_floor_lh_gl", (3, 4))])
def test_pack_frame_is_the_sample_grid_twin(api, name, offsets):
    """pack_frame at (H, W) with s = 2 equals pack_frame of the twin at (2H, 2W) with doubled offsets, field for field,
    and so does the frame descriptor, apart from its flags."""
    from py_numpy_renderer_amd import _native
    from py_numpy_renderer_amd._pack import pack_frame
    scene, twin = pair(api, name, 2, offsets)
    a, b = pack_frame(scene), pack_frame(twin)
    assert (a.supersample, b.supersample) == (2, 1)
    assert (a.height, a.width) == (2 * scene.resolution[0], 2 * scene.resolution[1])
    _assert_same_frame(a, b)
    if name == "cube_skybox":
        assert a.sky_tri is not None and a.sky_rays is not None
    da, db = _native.fill_frame_desc(a), _native.fill_frame_desc(b)
    assert da.flags == db.flags | _native.FRAME_SUPERSAMPLE2
    db.flags = da.flags
    assert bytes(da) == bytes(db)
    # the user's objects are left alone
    assert tuple(scene.resolution) == tuple(np.array(twin.resolution) // 2)
    assert np.array_equal(scene.camera.viewport[:2, :2] * 2, twin.camera.viewport[:2, :2])


def test_row_band_counts_output_rows(api):
    from py_numpy_renderer_amd import _native
    from py_numpy_renderer_amd._pack import pack_frame
    scene, _ = pair(api, "cube_small", 4)
    d = _native.fill_frame_desc(pack_frame(scene), row_band=(30, 60))
    assert (d.row_begin, d.row_end, d.height) == (120, 240, 480)
    assert d.flags & _native.FRAME_SUPERSAMPLE4 and not d.flags & _native.FRAME_SUPERSAMPLE2


def _header_frame_flags():
    with open(os.path.join(ROOT, "include", "mi355rast.h")) as fh:
        text = fh.read()
    body = re.search(r"/\* mr_frame_desc\.flags \*/\s*enum \{(.*?)\};", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return {k: int(v) for k, v in re.findall(r"\b(MR_FRAME_\w+)\s*=\s*(\d+)", body)}


def test_header_declares_disjoint_supersample_flags():
    from py_numpy_renderer_amd import _native
    flags = _header_frame_flags()
    assert flags["MR_FRAME_SUPERSAMPLE2"] == _native.FRAME_SUPERSAMPLE2 == 512
    assert flags["MR_FRAME_SUPERSAMPLE4"] == _native.FRAME_SUPERSAMPLE4 == 1024
    others = 0
    for k, v in flags.items():
        assert v and v & (v - 1) == 0, k                 # one bit each
        if k not in ("MR_FRAME_SUPERSAMPLE2", "MR_FRAME_SUPERSAMPLE4"):
            others |= v
    assert not others & (_native.FRAME_SUPERSAMPLE2 | _native.FRAME_SUPERSAMPLE4)
    # every flag the binding names is the header's
    for k, v in flags.items():
        assert getattr(_native, k[3:]) == v, k


def test_band_renderer_refuses_supersampling(api):
    """A split frame with supersampling is out of scope: refused before any device work."""
    pytest.importorskip("torch")
    from py_numpy_renderer_amd import multigpu
    scene = scenes.cube_small(api)
    scene.supersample = 2
    with pytest.raises(ValueError, match="supersample"):
        multigpu.BandRenderer(scene, rank=0, world=2)
    assert scene._renderer is None


def test_numpy_resolve_of_uniform_blocks_is_exact(api, oracle_mod):
    """The expected-frame helper on the oracle's sample grid of cube_small at (2H, 2W): blocks of four equal samples
    give exactly that colour, finalised like upstream (the background among them); the shape is the output's."""
    scene, twin = pair(api, "cube_small", 2)
    r = oracle_mod.render(twin, shadows=True)
    f = r.frame
    h, w = scene.resolution
    assert f.shape == (2 * h, 2 * w, 3) and f.dtype == np.float32
    out = resolve(f, 2)
    assert out.shape == (h, w, 3) and out.dtype == np.uint8
    blocks = f.reshape(h, 2, w, 2, 3)
    uniform = (blocks == blocks[:, :1, :, :1]).all(axis=(1, 3, 4))
    assert uniform.mean() > 0.5 and (~uniform).any()            # background and interior, and some edges
    want = (blocks[:, 0, :, 0][::-1] ** 0.8 * 255).astype(np.uint8)
    assert np.array_equal(out[uniform[::-1]], want[uniform[::-1]])
    # the same as upstream's finalise (the oracle's) of the uniform samples themselves
    fin = oracle_mod.finalise(f)[::-1][::2, ::2][::-1]
    assert np.array_equal(out[uniform[::-1]], fin[uniform[::-1]])
    # s = 1 is the identity before the finalise
    assert np.array_equal(resolve(f, 1), (f[::-1] ** 0.8 * 255).astype(np.uint8))
