"""GPU: ``k_ao``, ``k_dof``, ``k_accum_add`` and ``k_accum_resolve`` on the synthetic fields of post_fields.py, through
``mr_debug_post`` -- every workgroup shape of a kernel in one process, whatever MR_AO_TILE and MR_DOF_TILE say.

The yardstick is the host mirror (``mr_host_ao``, ``mr_host_dof``, ``mr_host_accum``), which tests/test_post_fields_cpu.py
holds to the NumPy restatements on the same fields: the float output bit for bit (a NaN where the mirror has one), the bytes
byte for byte wherever the mirror's cast is defined, the shapes of a kernel against each other.  The beacons' counts of
changed samples, derived from the definition, are asserted on the device's output too."""
import itertools

import numpy as np
import pytest

import post_fields as pf
import scenes

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


def _hold(native, handle, case, tally):
    """The case through every workgroup shape of the kernels it runs; returns {(ao shape, dof shape): float output}."""
    want, want_rgb = pf.mirror(native, case)
    outs = {}
    for ao_shape, dof_shape in itertools.product(range(3) if case.ao else (0,), range(3) if case.dof else (0,)):
        label = f"{case.name}, k_ao shape {ao_shape}, k_dof shape {dof_shape}"
        got, rgb = pf.device(native, handle, case, ao_shape, dof_shape)
        bad, compared, nans = pf.float_mismatches(got, want)
        assert bad == 0, f"{label}: {bad} of {compared + nans} floats are not the mirror's"
        bad_bytes, n_bytes = pf.byte_mismatches(rgb, want_rgb, want, case.shift)
        assert bad_bytes == 0, f"{label}: {bad_bytes} of {n_bytes} bytes are not mr_host_accum's"
        outs[ao_shape, dof_shape] = got
        for kernel, shape in (("k_ao", ao_shape if case.ao else None), ("k_dof", dof_shape if case.dof else None),
                              ("k_accum_add", 0 if case.weights is not None else None), ("k_accum_resolve", 0)):
            if shape is not None:
                t = tally.setdefault((kernel, shape), [0, 0, 0])
                t[0] += 1
                t[1] += n_bytes // 3 if kernel == "k_accum_resolve" else case.z.size * len(case.frames)
                t[2] += compared
    first = next(iter(outs.values()))
    for shapes, got in outs.items():                                 # (the mirror's NaNs carry no bits: the shapes among themselves do)
        assert pf.float_mismatches(got, first)[0] == 0, f"{case.name}: shapes {shapes} and (0, 0) differ"
    return outs


def _report(tally):
    for (kernel, shape), (runs, samples, floats) in sorted(tally.items()):
        print(f"{kernel} shape {shape}: {runs} runs, {samples} samples, {floats} floats compared bit for bit")


def test_k_ao_on_every_field(native, handle):
    tally = {}
    cases = pf.ao_cases()
    for case in cases:
        _hold(native, handle, case, tally)
    _report(tally)
    assert all(tally["k_ao", shape][0] == len(cases) for shape in range(3))


def test_k_dof_on_every_field(native, handle):
    tally = {}
    cases = pf.dof_cases()
    for case in cases:
        _hold(native, handle, case, tally)
    _report(tally)
    assert all(tally["k_dof", shape][0] == len(cases) for shape in range(3))


def test_k_dof_beacons_change_the_samples_the_definition_names(native, handle):
    tally, bounds = {}, {tile: set() for tile in pf.DOF_TILES}
    cases = pf.dof_beacon_cases()
    for case, mask in cases:
        for shapes, got in _hold(native, handle, case, tally).items():
            changed = pf.changed(got, case.frames[0])
            assert np.array_equal(changed, mask), f"{case.name}, k_dof shape {shapes[1]}: {int(changed.sum())} samples changed, {int(mask.sum())} derived"
        for tile in bounds:
            bounds[tile] |= pf.dof_bounds(pf.circle(case), tile)
    _report(tally)
    print("loop bounds met: " + ", ".join(f"{tile} x {tile}: {sorted(b)}" for tile, b in bounds.items()))
    assert all(b == set(range(17)) for b in bounds.values())
    counts = {float(case.name.split("c=")[1]): int(mask.sum()) for case, mask in cases if case.shape == pf.BEACON_FRAME}
    assert all(counts[c] == n for c, n in pf.BEACON_COUNTS.items())


def test_k_ao_then_k_dof_in_one_call(native, handle):
    tally = {}
    case = pf.composition_case()
    outs = _hold(native, handle, case, tally)
    assert len(outs) == 9
    darkened = pf.mirror(native, pf.Case("ao alone", case.z, case.frames, ao=case.ao))[0]
    assert pf.changed(darkened, case.frames[0]).any() and pf.changed(outs[0, 0], darkened).any()
    _report(tally)


def test_the_step_function_at_every_threshold(native, handle):
    tally = {}
    for case in pf.step_cases(native):
        _hold(native, handle, case, tally)
    _report(tally)
    # the bytes of the values themselves, spelled out: k - 1, k - 1, k, k, k round every threshold
    case = pf.step_cases(native)[0]
    rgb = pf.device(native, handle, case)[1].reshape(-1)
    ks = np.arange(1, 256)
    assert np.array_equal(rgb[:1275].reshape(255, 5), np.stack([ks - 1, ks - 1, ks, ks, ks], axis=1))
    assert rgb[1275:1283].tolist() == [0, 0, 254, 255, 255, 255, 255, 255]


def test_the_sum_at_every_tail(native, handle):
    tally = {}
    for case in pf.sum_cases():
        _hold(native, handle, case, tally)
    _report(tally)


def test_the_sum_takes_a_second_grid_trip(native, handle):
    tally = {}
    case = pf.sum_big_case()
    got = _hold(native, handle, case, tally)[0, 0]
    assert case.frames[0].size // 4 > pf.ACCUM_GRID_LANES and case.frames[0].size % 4 == 2
    assert pf.float_mismatches(pf.sum_one_trip(case.frames, case.weights), got)[0] == 4 * (case.frames[0].size // 4 - pf.ACCUM_GRID_LANES)
    _report(tally)


def test_the_entry_leaves_a_live_scene_alone(api, native):
    """A scene with obscurance and depth of field renders the same bytes before and after the entry ran on its handle, and
    the kernels' counters move by the renders only."""
    from py_numpy_renderer_amd import AmbientOcclusion, DepthOfField
    scene = scenes.cube_outward(api, resolution=(37, 41))
    scene.ambient_occlusion = AmbientOcclusion(radius=2.0)
    scene.depth_of_field = DepthOfField(lens_radius=0.215)
    before = scene.render().copy()
    backend = scene._backend()
    frame, z = backend.read_frame_f32().copy(), backend.read_z().copy()
    counters = backend.ao_debug(), backend.dof_debug(), backend.accum_debug()
    assert counters[0] == (1, 37, 41) and counters[1] == (1, 37, 41)
    for case in (pf.composition_case(), pf.sum_cases()[-1]):
        want, want_rgb = pf.mirror(native, case)
        got, rgb = pf.device(native, backend.handle, case, 1, 2)
        assert pf.float_mismatches(got, want)[0] == 0 and pf.byte_mismatches(rgb, want_rgb, want, case.shift)[0] == 0
    assert (backend.ao_debug(), backend.dof_debug(), backend.accum_debug()) == counters, "the entry moved a counter"
    assert pf.float_mismatches(backend.read_frame_f32(), frame)[0] == 0, "the entry touched the scene's float frame"
    assert np.array_equal(backend.read_z().view(np.uint64), z.view(np.uint64)), "the entry touched the scene's z-buffer"
    after = scene.render().copy()
    assert np.array_equal(after, before), f"{int((after != before).sum())} bytes differ after the entry ran"
    assert backend.ao_debug() == (2, 37, 41) and backend.dof_debug() == (2, 37, 41) and backend.accum_debug() == counters[2]
    scene.close()
