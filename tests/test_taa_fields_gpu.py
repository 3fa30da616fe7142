"""GPU: ``k_taa`` on the synthetic cases of taa_fields.py, through ``mr_debug_taa_post`` -- every workgroup shape in one
process, whatever MR_TAA_TILE says.

The yardstick is the host mirror ``mr_host_taa``, which tests/test_taa_cpu.py holds to the NumPy restatement on the same
cases: the float frame and the new history, both bit for bit, at every shape; and the sentinel bytes the entry keeps round
both outputs on the device must be untouched."""
import numpy as np
import pytest

import taa_fields as tf

pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize("size", tf.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_kernel_is_the_mirror_on_every_case(native, handle, size):
    changed = 0
    for case in tf.cases(size):
        want = case.mirror(native)
        changed += tf.bits(want, case.frame)
        for shape in range(3):
            out, hist, guard = case.device(native, handle, shape)
            label = f"{case!r}, shape {shape}"
            assert guard == 0, f"{label}: {guard} sentinel bytes round the outputs changed"
            assert tf.bits(out, want) == 0, f"{label}: {tf.bits(out, want)} of {want.size} floats of the frame are not mr_host_taa's"
            assert tf.bits(hist, want) == 0, f"{label}: {tf.bits(hist, want)} of {want.size} floats of the history are not mr_host_taa's"
    assert changed > 0 or size == (1, 1), "no case changed a float: the kernel was shown nothing"


def test_refusals_touch_no_device(native, handle):
    lib = native.load_library()
    case = tf.cases((4, 4))[0]
    for shape in (3, -1):
        with pytest.raises(ValueError, match="shape"):
            case.device(native, handle, shape)
    out = np.zeros(6, np.int32)
    assert lib.mr_debug_taa(handle, out.ctypes.data) == 0 and out.tolist() == [0] * 6, "the entry moved the scene's counters"
    hist = np.zeros((4, 4, 3), np.float32)
    assert lib.mr_read_history(handle, hist.ctypes.data) == native.MR_E_INVALID, "the entry left the scene a history"
