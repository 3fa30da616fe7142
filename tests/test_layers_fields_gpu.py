"""GPU: ``k_layers`` on the synthetic fields of layers_fields.py, through ``mr_debug_layers_post`` -- both record types, both
handednesses and the orthographic camera, winner maps whose widths are no multiple of the workgroup -- with every single
layer, with all of them and with a subset.

The yardstick is the host mirror ``mr_host_layers``, which tests/test_layers_cpu.py holds to the NumPy restatement and to
exact arithmetic on the same fields: every layer bit for bit.  On the device every layer's buffer lies between sentinel bytes
and starts as sentinel: no guard byte may change, and a layer the mask does not name must come back as sentinel."""
import numpy as np
import pytest

import layers_fields as lf
import layers_ref as ref

pytestmark = pytest.mark.gpu

FIELDS = lf.fields()
ALL = 0x1ff
MASKS = [1 << i for i in range(9)] + [ALL, (1 << 1) | (1 << 4) | (1 << 7)]


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


def _check(native, handle, field, S, mask, want):
    got, guard = native.debug_layers_post(handle, field.winner, field.pos, field.attr, field.face_off, field.desc(S, mask))
    assert guard == 0, f"{field!r}, mask {mask:#x}: {guard} guard bytes changed"
    for i, name in enumerate(ref.NAMES):
        if mask >> i & 1:
            assert lf.same_bits(got[name], want[name]) == 0, f"{field!r}, mask {mask:#x}: {lf.same_bits(got[name], want[name])} words of {name} are not the mirror's"
        else:
            assert (got[name].view(np.uint8) == native.LAYERS_SENTINEL).all(), f"{field!r}, mask {mask:#x}: {name} was not asked for and was written"


@pytest.mark.parametrize("field", FIELDS, ids=lambda f: f.name)
def test_the_kernel_is_the_mirror_on_every_field(native, handle, field):
    for kind, masks in ((None, MASKS), ("ortho", [ALL])):
        S = field.camera(kind)
        want, _ = native.host_layers(field.winner, field.pos, field.attr, field.face_off, field.desc(S))
        for mask in masks:
            _check(native, handle, field, S, mask, want)
    counts = np.zeros(4, np.int32)
    assert native.load_library().mr_debug_layers(handle, counts.ctypes.data) == 0
    assert counts.tolist() == [0, 0, 0, 0], "the entry moved the scene's counters"


def test_a_seeded_camera_and_the_timed_entry(native, handle):
    field = next(f for f in FIELDS if f.shape == (3, 257) and f.pos32)
    S = lf.seeded_camera(9)
    want, _ = native.host_layers(field.winner, field.pos, field.attr, field.face_off, field.desc(S))
    got, guard, ms = native.debug_layers_post(handle, field.winner, field.pos, field.attr, field.face_off, field.desc(S), times=True)
    assert guard == 0 and ms > 0
    for name in ref.NAMES:
        assert lf.same_bits(got[name], want[name]) == 0, name


def test_refusals_touch_no_device_and_the_scene_stays_as_it_was(native, handle):
    lib = native.load_library()
    field = FIELDS[-1]
    S = field.camera()
    with pytest.raises(ValueError, match="mask"):
        native.debug_layers_post(handle, field.winner, field.pos, field.attr, field.face_off, field.desc(S, 0))
    bad = S.copy()
    bad[0, 0] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        native.debug_layers_post(handle, field.winner, field.pos, field.attr, field.face_off, field.desc(bad))
    too_far = field.winner.copy()
    too_far[-1, -1] = len(field.pos)
    with pytest.raises(ValueError, match="not a face"):
        native.debug_layers_post(handle, too_far, field.pos, field.attr, field.face_off, field.desc(S))
    ms = np.zeros(1, np.float32)
    assert lib.mr_debug_layers_times(handle, ms.ctypes.data_as(native.C.POINTER(native.C.c_float))) == native.MR_E_INVALID, "the entry left the scene marks"
    out = np.zeros(4, np.float32)
    assert lib.mr_read_layers(handle, 4, out.ctypes.data) == native.MR_E_INVALID, "the entry left the scene a frame slot with a frame"
