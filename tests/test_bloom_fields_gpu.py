"""GPU: the bloom's three kernels on the synthetic fields of bloom_fields.py, through ``mr_debug_bloom_post`` -- every
workgroup shape in one process, whatever MR_BLOOM_TILE says, at 1, 2, 3 and 8 levels.

The yardstick is the host mirror ``mr_host_bloom``, which tests/test_bloom_cpu.py holds to the NumPy restatement on the same
fields: the float frame and the pyramid (D_1 .. D_L, U_{L-1} .. U_1), bit for bit, at every shape.  Both outputs are handed
over between guard floats that must come back untouched (``_native._bloom_call``), and on the device the frame and the
pyramid lie between sentinel bytes that the entry checks itself."""
import numpy as np
import pytest

import bloom_fields as bf

pytestmark = pytest.mark.gpu

CASES = bf.cases()


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
    assert native.load_library().mr_debug_bloom(handle, out.ctypes.data) == 0
    return out.tolist()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_the_kernels_are_the_mirror_on_every_field(native, handle, case):
    changed = 0
    for levels in bf.LEVELS:
        at = case.at(levels)
        want = at.mirror(native)
        changed += bf.bits(want[0], at.frame)
        for shape in range(3):
            got = at.device(native, handle, shape)               # (raises where a guard float or a sentinel byte changed)
            frame, pyramid = bf.all_bits(got, want)
            label = f"{at!r}, shape {shape}"
            assert frame == 0, f"{label}: {frame} of {want[0].size} floats of the frame are not mr_host_bloom's"
            assert pyramid == 0, f"{label}: {pyramid} floats of the pyramid are not mr_host_bloom's"
    assert changed > 0 or case.name == "below the threshold", "no level count changed a float: the kernels were shown nothing"
    assert _counts(native, handle) == [0] * 4, "the entry moved the scene's counters"


def test_the_frame_alone_is_handed_out_without_a_pyramid(native, handle):
    case = bf.Case("no pyramid", bf.seeded((17, 33)), levels=3)
    out = native.debug_bloom_post(handle, case.frame, case.desc(native), shape=1)
    assert bf.bits(out, case.mirror(native)[0]) == 0


def test_refusals_touch_no_device_and_the_scene_stays_as_it_was(native, handle):
    lib = native.load_library()
    case = bf.cases()[3]
    for shape in (3, -1):
        with pytest.raises(ValueError, match="shape"):
            case.device(native, handle, shape)
    assert _counts(native, handle) == [0] * 4, "the entry moved the scene's counters"
    ms = np.zeros(3, np.float32)
    assert lib.mr_debug_bloom_times(handle, ms.ctypes.data_as(native.C.POINTER(native.C.c_float))) == native.MR_E_INVALID, "the entry left the scene marks"
    z = np.zeros((4, 4), np.float64)
    assert lib.mr_read_z(handle, z.ctypes.data) == native.MR_E_INVALID, "the entry left the scene a frame slot with a frame"
