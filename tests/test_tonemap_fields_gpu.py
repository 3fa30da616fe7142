"""GPU: the tone mapping's three kernels on the synthetic fields of tonemap_fields.py, through ``mr_debug_tone_map_post`` --
at grid caps 1, 2, 3 of ``k_lum_hist`` (the stride loop, a few slab rows) and the library's default, both forms of the
kernel in one process whatever MR_TONEMAP_HIST says, all three operators, a fixed and a metered exposure, with and without
a previous exposure.

The yardstick is the host mirror ``mr_host_tone_map``, which tests/test_tonemap_cpu.py holds to the NumPy restatement on the
same fields: the float frame, the 256 counts, the exposure cell and the state cell a scene would adopt, bit for bit.  Every
output is handed over between guard words that must come back untouched (``_native._tone_map_call``); on the device the
frame, the slot's words and the state cells lie between sentinel bytes that the entry checks itself, and the slab is
sentinel before ``k_lum_hist`` writes it, as it is never cleared in a frame either."""
import numpy as np
import pytest

import tonemap_fields as tf
import tonemap_ref as ref

pytestmark = pytest.mark.gpu

CASES = tf.cases()


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
    out = np.zeros(6, np.int32)
    assert native.load_library().mr_debug_tone_map(handle, out.ctypes.data) == 0
    return out.tolist()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_the_kernels_are_the_mirror_on_every_field(native, handle, case):
    runs = 0
    for operator in ref.OPERATORS:
        for e_prev in sorted({-1.0, case.e_prev or 3.0}):
            at = case.at(e_prev=None if e_prev < 0 else e_prev, operator=operator, exposure=None)
            want = at.mirror(native)
            for cap in tf.GRID_CAPS:
                for form in (0, 1):
                    got = at.device(native, handle, cap, form)       # (raises where a guard word or a sentinel byte changed)
                    label = f"{at!r}, grid cap {cap}, form {form}"
                    assert tf.same(got[:3], want) == (0, 0, 0), f"{label}: (frame floats, counts, exposure) that are not the mirror's: {tf.same(got[:3], want)}"
                    assert tf.bits(np.asarray([got[3]], np.float32), np.asarray([want[2]], np.float32)) == 0, f"{label}: the state cell"
                    runs += 1
        fixed = case.at(operator=operator, exposure=case.params.exposure or 0.37)
        got, want = fixed.device(native, handle), fixed.mirror(native)
        assert tf.same(got[:3], want) == (0, 0, 0) and got[3] == want[2], f"{fixed!r}: {tf.same(got[:3], want)}"
    assert runs == 3 * 2 * 4 * 2
    assert _counts(native, handle) == [0] * 6, "the entry moved the scene's counters"


def test_the_default_cap_gives_the_large_field_many_rows(native, handle):
    case = next(c for c in CASES if c.shape == tf.LARGE)
    n4 = case.shape[0] * case.shape[1] // 4
    assert -(-n4 // 256) == 17, "seventeen workgroups under the default cap: seventeen slab rows"
    want = case.mirror(native)
    for cap in (0, 16, 17, 1024):
        assert tf.same(case.device(native, handle, cap, 0)[:3], want) == (0, 0, 0), cap


def test_refusals_touch_no_device_and_the_scene_stays_as_it_was(native, handle):
    lib = native.load_library()
    case = CASES[3]
    for cap in (-1, 1025):
        with pytest.raises(ValueError, match="grid cap"):
            case.device(native, handle, cap, 0)
    for form in (-2, 2):
        with pytest.raises(ValueError, match="form"):
            case.device(native, handle, 0, form)
    with pytest.raises(ValueError, match="previous exposure"):
        case.at(e_prev=float("nan")).device(native, handle)
    with pytest.raises(ValueError, match="speed"):
        case.at(speed=0.0).device(native, handle)
    assert _counts(native, handle) == [0] * 6, "the entry moved the scene's counters"
    ms = np.zeros(3, np.float32)
    assert lib.mr_debug_tone_map_times(handle, ms.ctypes.data_as(native.C.POINTER(native.C.c_float))) == native.MR_E_INVALID, "the entry left the scene marks"
    e = np.zeros(1, np.float32)
    assert lib.mr_read_exposure(handle, e.ctypes.data) == native.MR_E_INVALID, "the entry left the scene a frame slot with a frame"
