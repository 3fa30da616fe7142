"""CPU: the data layers' host mirror ``mr_host_layers`` against the NumPy restatement layers_ref.py, bit for bit on every
layer of every field of layers_fields.py; against exact arithmetic -- equal after the one rounding where float64 is exact,
within the error bound csrc/layers_def.h derives elsewhere --; the mutants of the definition, each told apart by some layer;
which samples are degenerate; what the library and ``Layers`` refuse; the packer's matrix.  No device is touched."""
from fractions import Fraction

import numpy as np
import pytest

import layers_fields as lf
import layers_ref as ref
import scenes

FIELDS = lf.fields()


@pytest.fixture(scope="module")
def native():
    from py_numpy_renderer_amd import _native
    _native.load_library()
    return _native


# ---------------------------------------------------------------------------- 1. the mirror is the definition
@pytest.mark.parametrize("field", FIELDS, ids=lambda f: f.name)
def test_the_mirror_is_the_reference_on_every_layer(native, field):
    for kind in (None, "ortho"):
        for jitter in ((0.0, 0.0), lf.JITTER):
            S = field.camera(kind, jitter)
            got, n_degenerate = native.host_layers(field.winner, field.pos, field.attr, field.face_off, field.desc(S))
            want, degenerate = ref.layers(field.winner, field.pos, field.attr, field.face_off, S)
            assert sorted(got) == sorted(ref.NAMES)
            differ = {name: lf.same_bits(got[name], want[name]) for name in ref.NAMES}
            assert not any(differ.values()), f"{field!r}, camera {kind}, jitter {jitter}: words that differ: {differ}"
            # only the samples of the faces made to be degenerate are, and they keep their ids
            assert n_degenerate == int(degenerate.sum()) == field.degenerate_samples(), (field, kind, jitter)
            assert (got["model"][degenerate] >= 0).all() and np.isinf(got["depth"][degenerate]).all()
            assert not got["position"][degenerate].any() and not got["barycentric"][degenerate].any()


def test_the_fields_cover_what_they_are_named_for():
    assert {f.shape for f in FIELDS} == {(1, 1), (1, 256), (3, 257), (5, 67)}
    assert {f.pos32 for f in FIELDS} == {True, False} and {f.lh for f in FIELDS} == {True, False}
    big = [f for f in FIELDS if f.winner.size > 256]
    assert big
    for f in big:
        n = len(f.kinds)
        assert f.face_off.tolist() == [0, n // 2, n // 2], "an empty model in the middle"
        flat = f.winner.ravel()
        assert {-1, 0, n // 2 - 1, n // 2, n - 1} <= set(flat[:8].tolist()) and (flat[251:256] >= -1).all()
        assert {-1, 0, n // 2 - 1, n // 2, n - 1} <= set(flat[256:264].tolist()), "each side of a block edge"
        assert set(flat.tolist()) >= set(range(n)), "every face shows somewhere"
        assert f.degenerate_samples() > 0
        model = ref.model_of(f.face_off, flat[flat >= 0])
        assert set(model.tolist()) == {0, 2}, "no sample belongs to the empty model"
    straddling = FIELDS[-1].pos["v"][FIELDS[-1].kinds.index("straddling")][:, :3].astype(np.float64)
    w = np.c_[straddling, np.ones(3)] @ FIELDS[-1].camera()[:, 2]
    assert w.min() < 0 < w.max(), "a face on both sides of the camera plane"


# ---------------------------------------------------------------------------- 2. against exact arithmetic
def _exact(field, S, f, x, y):
    return ref.exact_sample(field.pos["v"][f][:, :3], field.attr["uv"][f], S, x, y)


@pytest.mark.parametrize("field", [f for f in FIELDS if f.shape == (5, 67)], ids=lambda f: f.name)
def test_dyadic_faces_equal_exact_arithmetic_after_the_one_rounding(native, field):
    checked = 0
    for kind in (None, "ortho"):
        S = field.camera(kind)
        got, _ = native.host_layers(field.winner, field.pos, field.attr, field.face_off, field.desc(S))
        for y, x in zip(*np.nonzero(field.winner >= 0)):
            f = int(field.winner[y, x])
            if field.kinds[f] != "dyadic":
                continue
            e = _exact(field, S, f, int(x), int(y))
            want = {"barycentric": e["lam"], "depth": [e["depth"]], "position": e["position"], "uv": e["uv"]}
            for name, values in want.items():
                have = np.atleast_1d(got[name][y, x])
                for v in values:
                    assert Fraction(float(v)) == v, "float64 holds the exact value: one rounding, to float32, remains"
                assert [np.float32(float(v)) for v in values] == have.tolist(), (field, kind, name, x, y)
            checked += 1
    assert checked >= 10


@pytest.mark.parametrize("field", [f for f in FIELDS if f.shape == (5, 67) and not f.lh], ids=lambda f: f.name)
def test_seeded_faces_stay_within_the_derived_bound_of_exact_arithmetic(native, field):
    """The bound is layers_def.h's, from the operation counts and each sample's conditioning kappa (layers_ref.bounds)."""
    S = lf.seeded_camera(5)
    winner = field.without(lf.DEGENERATE_KINDS)
    got, n_degenerate = native.host_layers(winner, field.pos, field.attr, field.face_off, field.desc(S))
    assert n_degenerate == 0
    bounded, unbounded, worst = 0, 0, {}
    for y, x in zip(*np.nonzero(winner >= 0)):
        f = int(winner[y, x])
        e = _exact(field, S, f, int(x), int(y))
        assert e is not None
        b = ref.bounds(e)
        if b is None:
            unbounded += 1
            continue
        bounded += 1
        want = {"barycentric": (e["lam"], b["lam"]), "depth": ([e["depth"]], [b["depth"]]), "position": (e["position"], b["position"])}
        if field.pos["flags"][f] & lf.FF_HAS_UV:
            want["uv"] = (e["uv"], b["uv"])
        for name, (values, limits) in want.items():
            for have, value, limit in zip(np.atleast_1d(got[name][y, x]), values, limits):
                assert np.isfinite(have), (name, x, y, field.kinds[f])
                err = abs(Fraction(float(have)) - value)
                assert err <= limit, f"{field!r} {field.kinds[f]} {name} at ({x}, {y}): error {float(err):.3e} over the bound {float(limit):.3e}"
                share = float(err / limit) if limit else 0.0
                worst[name] = max(worst.get(name, 0.0), share)
    print(f"{field!r}: {bounded} samples bounded, {unbounded} without a bound; largest error / bound: {worst}")
    assert bounded >= 200 and unbounded <= bounded // 20
    assert all(share <= 1.0 for share in worst.values())


# ---------------------------------------------------------------------------- 3. the mutants
@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_mutant_is_told_apart(mutant):
    field = next(f for f in FIELDS if f.shape == (5, 67) and not f.pos32 and not f.lh)
    S, plain = field.camera(jitter=lf.JITTER), field.camera(jitter=(0.0, 0.0))
    want, _ = ref.layers(field.winner, field.pos, field.attr, field.face_off, S)
    got, _ = ref.layers(field.winner, field.pos, field.attr, field.face_off, S, mutant=mutant, S_plain=plain)
    differ = {name: lf.same_bits(got[name], want[name]) for name in ref.NAMES}
    expected = {"unjittered": "barycentric", "screen_linear": "barycentric", "w_as_depth": None, "winding": "face_normal",
                "unnormalised": "normal", "face_global": "face", "boundary": "model"}[mutant]
    if mutant == "w_as_depth":            # (w IS the eye depth under the perspective cameras: the orthographic one tells them apart)
        S = field.camera("ortho")
        want, _ = ref.layers(field.winner, field.pos, field.attr, field.face_off, S)
        got, _ = ref.layers(field.winner, field.pos, field.attr, field.face_off, S, mutant=mutant)
        differ = {name: lf.same_bits(got[name], want[name]) for name in ref.NAMES}
        expected = "depth"
    assert differ[expected] > 0, (mutant, differ)


# ---------------------------------------------------------------------------- 4. refusals
def test_the_library_refuses_before_it_computes(native):
    field = next(f for f in FIELDS if f.shape == (5, 67))
    S = field.camera()
    call = lambda **kw: native.host_layers(kw.get("winner", field.winner), field.pos, field.attr, kw.get("face_off", field.face_off),
                                           kw.get("desc", field.desc(S)))
    for mask in (0, 1 << 9, -1):
        with pytest.raises(ValueError, match="mask"):
            call(desc=field.desc(S, mask))
    bad = S.copy()
    bad[2, 1] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        call(desc=field.desc(bad))
    with pytest.raises(ValueError, match="at least one model"):
        call(desc=native.fill_layers_desc(S, 1, 0))
    for face_off in ([1, 3, 3], [0, 5, 4], [0, 5, len(field.pos) + 1]):
        with pytest.raises(ValueError, match="ascend"):
            call(face_off=face_off)
    too_far = field.winner.copy()
    too_far[0, 0] = len(field.pos)
    with pytest.raises(ValueError, match="not a face"):
        call(winner=too_far)
    lib = native.load_library()
    table = (native.C.c_void_p * 9)()
    assert lib.mr_host_layers(field.winner.ctypes.data, 5, 67, field.pos.ctypes.data, int(field.pos32), field.attr.ctypes.data, len(field.pos),
                              field.face_off.ctypes.data, native.C.byref(field.desc(S, 16)), table, None) == native.MR_E_INVALID
    assert b"no array" in lib.mr_last_error()
    assert lib.mr_host_layers(field.winner.ctypes.data, 0, 67, field.pos.ctypes.data, int(field.pos32), field.attr.ctypes.data, len(field.pos),
                              field.face_off.ctypes.data, native.C.byref(field.desc(S, 16)), table, None) == native.MR_E_INVALID
    for name in ("mr_scene_set_layers", "mr_read_layers", "mr_host_layers", "mr_debug_layers", "mr_debug_layers_times", "mr_debug_layers_post",
                 "mr_debug_read_face_records"):
        assert name in native.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    assert lib.mr_abi_version() == 4, "additions only"


def test_a_mask_computes_its_layers_only(native):
    field = next(f for f in FIELDS if f.shape == (3, 257))
    S = field.camera()
    full, _ = native.host_layers(field.winner, field.pos, field.attr, field.face_off, field.desc(S))
    for mask in (1 << 4, (1 << 0) | (1 << 7) | (1 << 8)):
        part, _ = native.host_layers(field.winner, field.pos, field.attr, field.face_off, field.desc(S, mask))
        assert sorted(part) == sorted(n for i, n in enumerate(ref.NAMES) if mask >> i & 1)
        for name, a in part.items():
            assert lf.same_bits(a, full[name]) == 0, name


def test_layers_validates_its_names():
    import py_numpy_renderer_amd as pkg
    from py_numpy_renderer_amd import _pack
    api = scenes.product_api()
    api.Layers = pkg.Layers
    assert "Layers" in pkg.__all__
    assert api.Layers(("depth", "normal")).names == ("depth", "normal")
    assert api.Layers(list(ref.NAMES)).names == ref.NAMES == _pack.LAYER_NAMES
    assert _pack.layer_mask(("model", "uv")) == 1 | 256 and _pack.layer_mask(ref.NAMES) == 0x1ff
    for bad in ((), []):
        with pytest.raises(ValueError, match="at least one"):
            api.Layers(bad)
    with pytest.raises(ValueError, match="unknown layer"):
        api.Layers(("depth", "albedo"))
    with pytest.raises(ValueError, match="twice"):
        api.Layers(("depth", "uv", "depth"))
    for bad in ("depth", None, 3, (3,), (b"depth",)):
        with pytest.raises(TypeError):
            api.Layers(bad)
    layers = api.Layers(("depth",))
    with pytest.raises(AttributeError, match="read-only"):
        layers.names = ("uv",)
    assert repr(layers) == "Layers(('depth',))"
    scene = scenes.cube_small(api, resolution=(48, 64))
    assert scene.layers is None
    with pytest.raises(TypeError, match="Layers"):
        scene.layers = ("depth",)
    scene.layers = layers
    assert scene.layers is layers
    with pytest.raises(ValueError, match="accumulate"):
        scene.accumulate()
    scene.layers = None
    with pytest.raises(ValueError, match="nothing rendered"):
        scene.read_layers()


# ---------------------------------------------------------------------------- 5. the packer's matrix
@pytest.mark.parametrize("recipe, supersample", [("cube_small", 1), ("cube_small", 2), ("tetra_ortho", 1), ("diablo_floor_lh_gl", 1)])
def test_layer_matrix_lands_where_the_frame_puts_a_point(recipe, supersample):
    from py_numpy_renderer_amd import _pack
    api = scenes.product_api()
    scene = getattr(scenes, recipe)(api, resolution=(48, 64))
    scene.supersample = supersample
    points = np.c_[np.random.default_rng(3).uniform(-0.5, 0.5, (16, 3)), np.ones(16)]
    cam = scene.camera
    for jitter in (None, (0.25, -0.375)):
        scene.__dict__["_sample_jitter"] = jitter
        try:
            pf = _pack.pack_frame(scene)
            S = _pack.layer_matrix(scene)
        finally:
            scene.__dict__.pop("_sample_jitter", None)
        framed = points @ pf.mvp @ pf.viewport
        mine = points @ S
        # (the frame multiplies by the two matrices one after the other, S by their product: equal to float64 rounding)
        assert np.allclose(mine[:, :3], framed[:, (0, 1, 3)], rtol=1e-12, atol=1e-12), "x, y, w are the frame's"
        plain = points @ np.asarray(cam.MVP, dtype=np.float64) @ np.asarray(_pack.sample_grid(scene)[3], dtype=np.float64)
        shift = mine[:, :2] / mine[:, 2:3] - plain[:, :2] / plain[:, 3:4]
        assert np.allclose(shift, (0.0, 0.0) if jitter is None else jitter, atol=1e-9)
        # column e: the distance along the view axis, > 0 for what the camera looks at, for the orthographic camera too
        axis = np.asarray(cam.center, dtype=np.float64) - np.asarray(cam.position, dtype=np.float64)
        along = (points[:, :3] - np.asarray(cam.position, dtype=np.float64)) @ (axis / np.linalg.norm(axis))
        assert np.allclose(mine[:, 3], along, atol=1e-6) and (mine[:, 3] > 0).all(), (mine[:, 3], along)
        # and depth_map's reading of the frame's own z agrees with it
        m = _pack.depth_map(scene, cam)
        scr_z = framed[:, 2] / framed[:, 3]
        n, f = float(cam.near), float(cam.far)
        Z = 2 * n * f / ((f + n) - scr_z * (f - n))
        assert np.allclose((m[0] * Z + m[1]) / (m[2] * Z + m[3]), mine[:, 3], rtol=1e-6, atol=1e-6)
