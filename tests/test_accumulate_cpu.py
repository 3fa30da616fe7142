"""CPU suite: the accumulation's host mirror (``mr_host_accum``) against its NumPy restatement (accumulate_ref.py), what
the library and the Python layer refuse, and the bindings.  No device is touched."""
import numpy as np
import pytest

import accumulate_ref as ref
import scenes

WEIGHTS = (0.5, 0.3, 0.2, 0.7, 1.25)                   # (0.3, 0.2 and 0.7 round as float32)
SHAPES = [((16, 16), 0), ((16, 16), 1), ((16, 16), 2), ((37, 41), 0), ((24, 40), 0), ((24, 40), 1), ((24, 40), 2)]


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as entry
    entry.build_native()
    from py_numpy_renderer_amd import _native
    _native.load_library()
    return _native


def _frames(n, shape, seed):
    rng = np.random.default_rng(20261020 + seed)
    return rng.random((n, shape[0], shape[1], 3), dtype=np.float32)


@pytest.mark.parametrize("shape, shift", SHAPES)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_host_mirror_is_the_numpy_definition(native, shape, shift, n):
    """The sum bit for bit; the bytes within one step (the host's powf against NumPy's power)."""
    frames, weights = _frames(n, shape, n), WEIGHTS[:n]
    scale = ref.default_scale(weights)
    acc, rgb = native.host_accum(frames, weights, shift=shift, scale=float(scale))
    want_acc, want_rgb = ref.result(frames, weights, s=1 << shift)
    assert acc.shape == shape + (3,) and rgb.shape == (shape[0] >> shift, shape[1] >> shift, 3) and rgb.dtype == np.uint8
    assert np.array_equal(acc.view(np.uint32), want_acc.view(np.uint32))
    diff = np.abs(rgb.astype(np.int16) - want_rgb.astype(np.int16)).max()
    print(f"{shape} shift {shift} n {n}: bytes differ by at most {diff}")
    assert diff <= 1


def test_either_output_may_be_left_out(native):
    frames = _frames(2, (16, 16), 7)
    acc, rgb = native.host_accum(frames, (0.5, 0.5), shift=1)
    only_acc, none = native.host_accum(frames, (0.5, 0.5), shift=1, want_rgb=False)
    none_too, only_rgb = native.host_accum(frames, (0.5, 0.5), shift=1, want_acc=False)
    assert none is None and none_too is None
    assert np.array_equal(only_acc, acc) and np.array_equal(only_rgb, rgb)


@pytest.mark.parametrize("shift", [0, 1, 2])
def test_splitting_one_frame_changes_no_byte(native, shift):
    """0.25 F + 0.25 F + 0.5 F is F exactly (powers of two), so the bytes are those of F alone."""
    frame = _frames(1, (24, 40), 11)
    _, one = native.host_accum(frame, (1.0,), shift=shift, scale=1.0)
    acc, three = native.host_accum(np.repeat(frame, 3, axis=0), (0.25, 0.25, 0.5), shift=shift, scale=1.0)
    assert np.array_equal(acc, frame[0])
    assert np.array_equal(three, one)


def test_the_clamp(native):
    """A sum above 1 finalises as 1: 255."""
    frames = np.full((2, 16, 16, 3), 0.75, dtype=np.float32)
    _, rgb = native.host_accum(frames, (1.0, 1.0), scale=1.0)
    assert (rgb == 255).all()
    assert np.array_equal(rgb, ref.result(frames, (1.0, 1.0), scale=1.0)[1])


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf"), -float("inf"), 1e-60, 1e60])
def test_the_library_refuses_bad_factors(native, bad):
    """Not finite or not > 0 -- as float32: 1e-60 is 0 there and 1e60 is inf."""
    frames = _frames(2, (16, 16), 3)
    with pytest.raises(ValueError, match="weight"):
        native.host_accum(frames, (1.0, bad))
    with pytest.raises(ValueError, match="scale"):
        native.host_accum(frames, (1.0, 1.0), scale=bad)


def test_the_library_refuses_bad_shapes(native):
    frames = _frames(1, (24, 40), 5)
    with pytest.raises(ValueError, match="shift"):
        native.host_accum(frames, (1.0,), shift=3)
    with pytest.raises(ValueError, match="shift"):
        native.host_accum(frames, (1.0,), shift=-1)
    with pytest.raises(ValueError, match="multiples"):
        native.host_accum(_frames(1, (37, 41), 5), (1.0,), shift=1)
    with pytest.raises(ValueError, match="multiples"):
        native.host_accum(_frames(1, (24, 42), 5), (1.0,), shift=2)
    lib = native.load_library()
    weights = np.ones(1)
    assert lib.mr_host_accum(frames.ctypes.data, weights.ctypes.data, 0, 24, 40, 0, 1.0, None, None) == native.MR_E_INVALID
    assert lib.mr_host_accum(None, weights.ctypes.data, 1, 24, 40, 0, 1.0, None, None) == native.MR_E_INVALID


def test_symbols_are_bound_and_the_abi_stays(native):
    lib = native.load_library()
    for name in ("mr_accum_begin", "mr_accum_add", "mr_accum_resolve", "mr_accum_read_f32", "mr_debug_accum",
                 "mr_debug_accum_times", "mr_host_accum"):
        assert name in native.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    assert lib.mr_abi_version() == native.ABI_VERSION == 4
    handle = lib.mr_scene_create()
    out = np.zeros(4, np.int32)
    assert lib.mr_accum_begin(handle) == 0
    assert lib.mr_debug_accum(handle, out.ctypes.data) == 0 and out.tolist() == [0, 0, 0, 0]
    rgb = np.zeros(3, np.uint8)
    assert lib.mr_accum_resolve(handle, 1.0, rgb.ctypes.data) == native.MR_E_INVALID and b"nothing accumulated" in lib.mr_last_error()
    assert lib.mr_accum_read_f32(handle, np.zeros(3, np.float32).ctypes.data) == native.MR_E_INVALID
    assert lib.mr_debug_accum_times(handle, (native.C.c_float * 2)()) == native.MR_E_INVALID
    assert lib.mr_accum_add(handle, None, 1.0) == native.MR_E_INVALID
    lib.mr_scene_destroy(handle)


def test_exported_from_the_package():
    import py_numpy_renderer_amd as pkg
    from py_numpy_renderer_amd.core import Accumulation
    assert "Accumulation" in pkg.__all__ and pkg.Accumulation is Accumulation
    assert callable(pkg.Scene.accumulate) and callable(pkg.Scene.render_mean)


def test_python_checks_come_before_any_device_call(api):
    """Weights and scales are refused in Python, and so is ``result()`` before an ``add()``: none of this needs a device
    (there is none in this suite, and ``Scene.accumulate`` creates no renderer)."""
    scene = scenes.cube_small(api, resolution=(16, 16))
    acc = scene.accumulate()
    assert scene._renderer is None and acc.count == 0 and acc.weight_sum == 0.0
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), 1e-60, 1e60, "1", None, True):
        with pytest.raises(ValueError, match="weight"):
            acc.add(bad)
    for bad in (0, -2.0, float("nan"), float("inf"), 1e60, "1"):
        with pytest.raises(ValueError, match="scale"):
            acc.result(scale=bad)
    with pytest.raises(RuntimeError, match="nothing accumulated"):
        acc.result()
    with pytest.raises(RuntimeError, match="nothing accumulated"):
        acc.result(scale=1.0)
    with pytest.raises(RuntimeError, match="nothing accumulated"):
        acc.float_frame()
    with pytest.raises(RuntimeError, match="open accumulation"):
        scene.accumulate()
    acc.close()
    with pytest.raises(RuntimeError, match="closed"):
        acc.add(1.0)
    with scene.accumulate() as again:
        assert again is not acc
    with pytest.raises(ValueError, match="n >= 1"):
        scene.render_mean(0, lambda k: None)
    assert scene._renderer is None
    scene.accumulate().close()


def test_default_scale_is_the_float32_of_the_float64_quotient():
    from py_numpy_renderer_amd._pack import default_accum_scale
    for weights in ((0.5, 0.3, 0.2), (1.0, 1.0, 1.0), (0.1,) * 7):
        total = 0.0
        for w in weights:
            total += w
        assert default_accum_scale(total) == float(np.float32(1.0 / total))
    assert default_accum_scale(3.0) == float(ref.default_scale((1.0, 1.0, 1.0)))
