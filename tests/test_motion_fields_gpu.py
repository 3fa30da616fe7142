"""GPU: ``k_velocity`` and ``k_mblur`` on the synthetic fields of motion_fields.py, through ``mr_debug_motion_post`` -- every
workgroup shape of ``k_mblur`` in one process, whatever MR_MBLUR_TILE says.

The yardsticks are the host mirrors (``mr_host_velocity``, ``mr_host_motion_blur``), which tests/test_motion_cpu.py holds to
the NumPy restatement on the same fields: the velocity buffer and the blurred frame bit for bit, at every shape."""
import numpy as np
import pytest

import motion_fields as mf

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


def _hold(native, handle, field):
    """The field through every workgroup shape; returns the mirror's (U, F')."""
    want_u, want_f = field.mirror(native)
    for shape in range(3):
        got_u, got_f = field.device(native, handle, shape)
        label = f"{field!r}, shape {shape}"
        assert mf.bits(got_u, want_u) == 0, f"{label}: {mf.bits(got_u, want_u)} of {want_u.size} velocity floats are not mr_host_velocity's"
        assert mf.bits(got_f, want_f) == 0, f"{label}: {mf.bits(got_f, want_f)} of {want_f.size} floats are not mr_host_motion_blur's"
    return want_u, want_f


@pytest.mark.parametrize("size", mf.GPU_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_both_kernels_are_the_mirrors_on_every_field(native, handle, size):
    bounds = {tile: set() for tile in set(mf.MBLUR_TILES)}
    samples = 0
    for field in mf.gpu_cases(size):
        u, f = _hold(native, handle, field)
        samples += u.shape[0] * u.shape[1]
        for tile in bounds:
            bounds[tile] |= {mf.bound_of(h) for h in mf.h_max(field, tile).ravel()}
        if field.name == "rest":
            # ((x * Z) / Z is x to within an ulp of float64, so U is zero or a few 1e-14: far below half a sample)
            assert np.abs(u).max() < 1e-9 and mf.bits(f, field.frame) == 0, "a frame at rest is not its input, bit for bit"
            assert all(mf.bound_of(h) == 0 for h in mf.h_max(field, 16).ravel())
        if field.name.startswith("clamp"):
            assert {mf.bound_of(h) for h in mf.h_max(field, 16).ravel()} == {16}
        if field.name == "behind" and size[1] > 21:
            assert not u[:, 21:].any() and u[:, :21].all(axis=-1).any(), "U behind the previous camera is not (0, 0)"
    print(f"{size}: {samples} samples per shape; loop bounds met: " + ", ".join(f"{t} x {t}: {sorted(b)}" for t, b in sorted(bounds.items())))


def test_the_owner_of_every_face_of_the_offset_table(native, handle):
    """One sample per winner value -- -1, the first and the last face of each model, the single-face model -- on a row: the
    class each takes shows in U, which the shifts make exact."""
    z, _, frame = mf.plane((1, 6), 9)
    winner = np.array([[-1, 0, 6, 7, 8, 11]], dtype=np.int32)
    field = mf.Field("owner_row", z, winner, frame, face_off=mf.THREE_MODELS, class_of_model=(0, 2, 1),
                     matrices=(mf.IDENTITY_T, mf.shift_t(5.0, -3.0), mf.shift_t(-9.5, 0.25)))
    u, _ = _hold(native, handle, field)
    assert u[0].tolist() == [[0, 0], [0, 0], [0, 0], [-9.5, 0.25], [5.0, -3.0], [5.0, -3.0]]


def test_refusals_touch_no_device(native, handle):
    lib = native.load_library()
    field = mf.at_rest((4, 4))
    with pytest.raises(ValueError, match="shape"):
        field.device(native, handle, 3)
    with pytest.raises(ValueError, match="shape"):
        field.device(native, handle, -1)
    out = np.zeros(3, np.int32)
    assert lib.mr_debug_motion(handle, out.ctypes.data) == 0 and out.tolist() == [0, 0, 0], "the entry moved the scene's counter"
