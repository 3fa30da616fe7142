"""GPU: ``k_face_homography`` and ``k_velocity_faces`` on the synthetic inputs of motion_faces_fields.py, through
``mr_debug_motion_faces_post``.

The yardsticks are the host mirrors (``mr_host_face_homographies``, ``mr_host_velocity_faces``), which
tests/test_motion_faces_cpu.py holds to the NumPy restatement on the same inputs: the face records and the velocity buffer
bit for bit.  The velocity buffer goes in filled with a sentinel pattern, so a sample the pass must not touch shows; on the
device both output buffers lie between guards of sentinel bytes, which the entry reads back."""
import numpy as np
import pytest

import motion_faces_fields as ff

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
    want_h, want_u = field.mirror(native)
    got_h, got_u, guard = field.device(native, handle)
    assert guard == 0, f"{field!r}: {guard} guard bytes round the output buffers changed"
    assert got_h.shape == want_h.shape and ff.bits64(got_h, want_h) == 0, f"{field!r}: {ff.bits64(got_h, want_h)} of {want_h.size} doubles of H are not the mirror's"
    assert ff.bits32(got_u, want_u) == 0, f"{field!r}: {ff.bits32(got_u, want_u)} of {want_u.size} velocity floats are not the mirror's"
    untouched = ~field.touched()
    assert ff.bits32(got_u[untouched], field.velocity[untouched]) == 0, f"{field!r}: a sample outside the flagged models was written"
    return got_h, got_u


@pytest.mark.parametrize("n_faces", ff.FACE_COUNTS)
def test_every_face_count_is_the_mirror(native, handle, n_faces):
    h, u = _hold(native, handle, ff.counted(n_faces, seed=n_faces))
    assert len(h) == n_faces
    for i, name in enumerate(ff.KINDS[:n_faces]):
        if name in ("zero_area", "nan_previous"):
            assert not h[i].any(), f"{name}: H is not zero"


@pytest.mark.parametrize("size", ff.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_flag_pattern_is_the_mirror(native, handle, size):
    for flags in ff.ALL_FLAGS:
        h, u = _hold(native, handle, ff.three_models(size, flags, seed=size[1]))
        assert len(h) == sum(n for n, f in zip((7, 1, 4), flags) if f)


def test_two_models_of_256_faces_meet_at_a_workgroup_edge(native, handle):
    """Records 0 .. 255 and 256 .. 511 belong to models 0 and 2, the unflagged model between them owns 65 faces: the
    range search of k_face_homography and the offset table of k_velocity_faces at their seams."""
    now, prev, corners = ff.seeded_faces(577, seed=9)
    face_off = (0, 256, 321)
    field = ff.FaceField("seam", now, prev, corners, face_off, (1, 0, 1), ff.camera_s(), ff.camera_s(eye=(0.05, -0.02, 0.1), yaw=0.01),
                         ff.winner_map((45, 70), 577, face_off, 9))
    h, _ = _hold(native, handle, field)
    assert len(h) == 512


def test_refusals_touch_no_device_state(native, handle):
    lib = native.load_library()
    field = ff.three_models((4, 5), (1, 1, 1))
    beyond = field.winner.copy()
    beyond[0, 0] = 12
    bad = ff.FaceField("beyond", field.verts_now, field.verts_prev, field.corners, field.face_off, field.deforming, field.s_now, field.s_prev, beyond)
    with pytest.raises(ValueError, match="has no record"):
        bad.device(native, handle)
    out = np.zeros(4, np.int32)
    assert lib.mr_debug_motion_faces(handle, out.ctypes.data) == 0 and out.tolist() == [0, 0, 0, 0], "the entry moved the scene's counters"
