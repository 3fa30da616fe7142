"""GPU: the light shafts' three kernels on the synthetic fields of shafts_fields.py, through ``mr_debug_light_shafts_post``,
at d = 1, 2, 3 and 4.

The yardstick is the host mirror ``mr_host_light_shafts``, which tests/test_shafts_cpu.py holds to the NumPy restatement on
the same fields: the float frame, the march's source S and its result R, bit for bit.  Every output is handed over between
guard floats that must come back untouched (``_native._shafts_call``), and on the device the frame, the z-buffer, S and R
each lie between sentinel bytes that the entry checks itself."""
import numpy as np
import pytest

import shafts_fields as sf

pytestmark = pytest.mark.gpu

CASES = sf.cases()


@pytest.fixture(scope="module")
def native():
    from py_numpy_renderer_amd import _native
    _native.load_library()
    return _native


@pytest.fixture(scope="module")
def handle(native):
    lib = native.load_library()
    h = lib.mr_scene_create()
    assert h
    yield h
    lib.mr_scene_destroy(h)


def _counts(native, handle):
    out = np.zeros(4, np.int32)
    assert native.load_library().mr_debug_light_shafts(handle, out.ctypes.data) == 0
    return out.tolist()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_the_kernels_are_the_mirror_on_every_field(native, handle, case):
    changed = 0
    for levels in sf.LEVELS:
        at = case.at(levels)
        want = at.mirror(native)
        changed += sf.bits(want[0], at.frame)
        got = at.device(native, handle)                          # (raises where a guard float or a sentinel byte changed)
        out, source, march = sf.all_bits(got, want)
        print(f"{at!r}: {out} of {want[0].size} floats of the frame, {source} of {want[1].size} of S and {march} of R differ from the mirror")
        assert source == 0, f"{at!r}: {source} floats of S are not mr_host_light_shafts's"
        assert march == 0, f"{at!r}: {march} floats of R are not mr_host_light_shafts's"
        assert out == 0, f"{at!r}: {out} of {want[0].size} floats of the frame are not mr_host_light_shafts's"
    assert (changed > 0) != (case.name in ("below the threshold", "mask none")), "the kernels were shown nothing"
    assert _counts(native, handle) == [0] * 4, "the entry moved the scene's counters"


def test_the_frame_alone_is_handed_out_without_the_levels(native, handle):
    case = sf.field("no levels", (17, 33), "comb")
    out = native.debug_light_shafts_post(handle, case.frame, case.zbuf, case.desc(native))
    assert sf.bits(out, case.mirror(native)[0]) == 0


def test_the_known_answers_hold_on_the_device(native, handle):
    for levels in sf.LEVELS:
        case = sf.below().at(levels)
        out, S, R = case.device(native, handle)
        assert sf.bits(out, case.frame) == 0 and not S.view(np.uint32).any() and not R.view(np.uint32).any()
        case = sf.uniform(levels=levels)
        out, S, R = case.device(native, handle)
        assert (S == np.float32(0.375)).all() and (R == R[0, 0]).all() and (out == out[0, 0, 0]).all() and out[0, 0, 0] > 0.75


def test_refusals_touch_no_device_and_the_scene_stays_as_it_was(native, handle):
    lib = native.load_library()
    case = sf.cases()[3]
    bad = case.desc(native)
    bad.halvings = 5
    with pytest.raises(ValueError, match="halvings"):
        native.debug_light_shafts_post(handle, case.frame, case.zbuf, bad)
    assert _counts(native, handle) == [0] * 4, "the entry moved the scene's counters"
    ms = np.zeros(3, np.float32)
    assert lib.mr_debug_light_shafts_times(handle, ms.ctypes.data_as(native.C.POINTER(native.C.c_float))) == native.MR_E_INVALID, "the entry left the scene marks"
    z = np.zeros((4, 4), np.float64)
    assert lib.mr_read_z(handle, z.ctypes.data) == native.MR_E_INVALID, "the entry left the scene a frame slot with a frame"
