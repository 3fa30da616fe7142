"""CPU: the synthetic fields of post_fields.py without a device -- the host mirrors against the NumPy restatements on every
field (bit for bit), the properties the cases were made for (the code paths of k_ao, k_dof and k_accum_add they reach,
restated in a few lines of Python), NumPy mutants of the definitions that the fields must tell from the definitions, and
what ``mr_debug_post`` refuses before it touches a device.  tests/test_post_fields_gpu.py runs the same cases through the
kernels."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import accumulate_ref
import ao_ref
import dof_ref
import post_fields as pf

F32 = np.float32
MR_E_DEVICE = -2                                 # include/mi355rast.h


@pytest.fixture(scope="module")
def native():
    from py_numpy_renderer_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        pytest.fail("libmi355rast.so is not built: run __graft_entry__.build()")
    return _native


@pytest.fixture(scope="module")
def ao_cases():
    return pf.ao_cases()


@pytest.fixture(scope="module")
def dof_cases():
    return pf.dof_cases()


@pytest.fixture(scope="module")
def beacons():
    return pf.dof_beacon_cases()


def _hold(native, case):
    """The mirror's float frame is the reference's bit for bit (a NaN where that has one); its bytes are NumPy's within one
    step wherever they are defined (the host's powf against NumPy's power, as in test_accumulate_cpu.py).  Returns the
    mirror's (float frame, bytes)."""
    want, want_rgb = pf.reference(case)
    got, got_rgb = pf.mirror(native, case)
    bad, compared, nans = pf.float_mismatches(got, want)
    assert bad == 0, f"{case.name}: {bad} of {compared + nans} floats of the mirror are not the reference's"
    mask = pf.byte_mask(got, case.shift)
    steps = np.abs(got_rgb.astype(np.int16) - want_rgb.astype(np.int16))[mask]
    assert steps.size == 0 or steps.max() <= 1, f"{case.name}: the mirror's bytes are {steps.max()} steps from NumPy's"
    return got, got_rgb


# ---------------------------------------------------------------------------- 1. the mirrors against NumPy
def test_the_ao_mirror_is_the_reference_on_every_field(native, ao_cases):
    darkened = 0
    for case in ao_cases + [pf.composition_case()]:
        got, _ = _hold(native, case)
        hole = ~np.isfinite(ao_ref.eye_depth(case.z, case.ao["m"]))
        if case.dof is None:
            assert pf.float_mismatches(got[hole], np.where(np.isnan(case.frames[0]), np.nan, case.frames[0])[hole])[0] == 0, case.name
        darkened += int(pf.changed(got, case.frames[0]).any())
    print(f"{len(ao_cases) + 1} cases, {darkened} of them change a sample")
    assert darkened >= len(ao_cases) // 2


def test_the_dof_mirror_is_the_reference_on_every_field(native, dof_cases):
    for case in dof_cases:
        got, _ = _hold(native, case)
        blurred = pf.changed(got, case.frames[0]).any()
        sharp = case.dof["kf"] in (0.1, 1e-45)                       # c < 0.5 everywhere, the sky too
        if case.shape != (5, 7):
            assert blurred != sharp, case.name


def test_the_poisoned_cases_keep_half_of_their_output_finite(native, ao_cases, dof_cases):
    """So the comparison on the device cannot go empty."""
    found = 0
    for case in ao_cases + dof_cases:
        if "poisoned" in case.name or "NaN" in case.name:
            got, _ = pf.mirror(native, case)
            share = float(np.isfinite(got).mean())
            print(f"{case.name}: {share:.1%} of the mirror's floats are finite, {int(np.isnan(got).sum())} are NaN")
            assert share >= 0.5, case.name
            assert not np.isfinite(got).all(), f"{case.name}: nothing of the poison reached the output"
            if "NaN" in case.name:
                assert np.isnan(got).any()
            else:
                assert not np.isnan(case.frames).any(), "NaN has a case of its own"
                for value in pf.POISON:
                    assert (case.frames.view(np.uint32) == F32(value).view(np.uint32)).any(), (case.name, value)
            found += 1
    assert found == 4


def test_the_beacon_counts_hold(native, beacons):
    """A single foreground beacon changes exactly the lattice points within its rr, and not itself; one behind the plane
    changes nothing.  The counts are derived, not measured."""
    table = {}
    for case, mask in beacons:
        got, _ = _hold(native, case)
        assert np.array_equal(pf.changed(got, case.frames[0]), mask), case.name
        if case.shape == pf.BEACON_FRAME:
            table[float(case.name.split("c=")[1])] = int(mask.sum())
        if "behind" in case.name:
            assert not mask.any()
    for c, n in pf.BEACON_COUNTS.items():
        assert table[c] == n, f"c = {c}: {table[c]} samples change, the lattice count is {n}"
    # the beacon on the last sample of workgroup (0, 0): most of its disc lies in other workgroups
    for tile in (32, 16):
        at = (tile - 1, tile - 1)
        ys, xs = np.nonzero(pf.beacon_disc(pf.BEACON_BIG, at, 16.0))
        assert len(ys) == (796 if tile == 32 else 794)               # (at (15, 15) the frame's edge cuts off two samples)
        assert int(((ys >= tile) | (xs >= tile)).sum()) == 581 and int(((ys >= tile) & (xs >= tile)).sum()) == 183


def test_the_sums(native):
    for case in pf.sum_cases() + [pf.sum_big_case()]:
        got, _ = _hold(native, case)
        assert np.isfinite(got).all()
    n = int(np.prod(pf.SUM_BIG)) * 3
    assert n == 2_100_210 and n // 4 == 525_052 > pf.ACCUM_GRID_LANES == 524_288 and n % 4 == 2
    assert sorted(int(np.prod(s)) * 3 % 4 for s in pf.SUM_SMALL) == [0, 1, 2, 3, 3] and 3 // 4 == 0
    assert max(pf.SUM_WEIGHTS) > 1 and min(pf.SUM_WEIGHTS) < 1e-20


def test_the_threshold_frame(native):
    """For every k a float finalised to k - 1 lies next to one finalised to k, with two floats on either side."""
    v = pf.step_values(native)
    assert len(v) == 255 * 5 + len(pf.STEP_EXTRAS)
    b = pf._bytes_of(native, v)
    around, bytes_around = v[:1275].reshape(255, 5), b[:1275].reshape(255, 5)
    assert (np.diff(around.view(np.uint32).astype(np.int64), axis=1) == 1).all(), "not neighbouring floats"
    ks = np.arange(1, 256)
    assert (bytes_around[:, :2] == (ks - 1)[:, None]).all() and (bytes_around[:, 2:] == ks[:, None]).all()
    assert b[1275:].tolist() == [0, 0, 254, 255, 255, 255, 255, 255]
    for case in pf.step_cases(native):
        got, rgb = _hold(native, case)
        assert rgb.shape == (1, 428, 3) and case.shape == (1 << case.shift, 428 << case.shift)
        if case.shift == 0 or "one sample" in case.name:             # (a uniform block's mean may lie a few floats off its value)
            assert np.array_equal(rgb.reshape(-1)[:len(b)], b), case.name


# ---------------------------------------------------------------------------- 2. the cases reach the code they were made for
@pytest.mark.parametrize("shape", [0, 1, 2])
def test_ao_rows_start_at_every_alignment_behind_the_first_workgroup_column(shape):
    tw = pf.AO_SHAPES[shape][0]
    rows = [r for size in pf.AO_SIZES for r in pf.ao_row_split(size[0], size[1], tw)]
    later = [(head, n4, tail) for x0, head, n4, tail in rows if x0 > 0]
    heads, tails = {h for h, _, _ in later}, {t for _, _, t in later}
    both = {(h, t) for h, _, t in later if h and t}
    print(f"k_ao shape {shape} ({tw} samples wide): behind the first column heads {sorted(heads)}, tails {sorted(tails)}, "
          f"{sum(n4 == 0 for _, n4, _ in later)} rows without a 16-byte piece, head and tail together {sorted(both)}")
    assert heads == {0, 1, 2, 3} and tails == {0, 1, 2, 3}
    assert any(n4 == 0 for _, n4, _ in later), "no last column of 1 to 3 samples"
    assert both, "no row with a head and a tail behind the first workgroup column"
    assert all(head + 4 * n4 + tail == 3 * min(tw, w - x0) for h, w in pf.AO_SIZES for x0, head, n4, tail in pf.ao_row_split(h, w, tw))
    for size in pf.AO_SIZES[3:]:                                     # two or more workgroup columns, partial workgroups
        assert size[1] > 2 * 64 and size[1] % 64 in (1, 2, 3, 4)


def test_ao_ties_and_range_edges_occur():
    for case in pf.ao_tie_cases():
        covered = int(np.isfinite(ao_ref.eye_depth(case.z, case.ao["m"])).sum())
        ties = pf.ao_ties(case)
        print(f"{case.name}: {ties} exact ties over {covered} covered samples")
        assert ties == 2 * covered > 0                               # the taps (1, 0) and (0, 1)
    assert pf.ao_ties(pf.ao_cases()[0]) == 0                         # (a perspective footprint meets none)
    at_edge, beyond = pf.ao_range_steps(pf.ao_range_case())
    print(f"ao range edge: {at_edge} steps of exactly the range, {beyond} of the float after it")
    assert at_edge > 100 and beyond > 100
    assert F32(3) - F32(1) == F32(2) and F32(pf.RANGE_LEVELS[2]) - F32(1) == np.nextafter(F32(2), F32(3))


@pytest.mark.parametrize("shape", [0, 1, 2])
def test_dof_beacons_set_every_loop_bound_and_some_from_the_halo_alone(beacons, shape):
    tile = pf.DOF_TILES[shape]
    bounds, from_halo = set(), 0
    for case, _ in beacons:
        s = pf.circle(case)
        with_halo, body = pf.dof_r2(s, tile), pf.dof_r2(s, tile, halo=False)
        bounds |= {math.isqrt(r2) for r2 in with_halo.values()}
        from_halo += sum(math.isqrt(with_halo[wg]) > math.isqrt(body[wg]) for wg in with_halo)
    print(f"k_dof shape {shape} ({tile} x {tile}): loop bounds {sorted(bounds)}, {from_halo} workgroups take theirs from the halo alone")
    assert bounds == set(range(17))
    assert from_halo > 0


def test_dof_fields_hold_what_they_were_made_for(dof_cases):
    by_name = {c.name: c for c in dof_cases}
    s = pf.circle(by_name["dof signed zeroes"])
    assert (s == 0).all() and np.signbit(s).any() and not np.signbit(s).all(), "no +0 beside -0"
    s = pf.circle(by_name["dof plateaus"])
    assert len(np.unique(s)) == 5 and (s[:6, :6] == s[0, 0]).all()
    sparse = by_name["dof sparse beacons (70, 101)"]
    s = pf.circle(sparse)
    share = float((s < -2.0).mean())
    assert 0.01 < share < 0.04 and all(s[at] == -20.0 for at in pf.PARKING)
    for tile, waves in ((32, 16), (16, 4)):                          # a parking cell is global (y0 - 16, x0 - 16 + i), i < waves
        assert any((y + 16) % tile == 0 and (x + 16) % tile < waves and y + 16 < 70 and x - (x + 16) % tile + 16 < 101 for y, x in pf.PARKING)
    low, high = [], []
    for case in dof_cases:
        if "hills (70, 101)" in case.name:
            c = np.abs(pf.circle(case))[np.isfinite(case.z)]
            low.append(float(c.min())), high.append(float(c.max()))
    assert min(low) < 0.01 and max(high) > 2 * dof_ref.MAX_RADIUS


# ---------------------------------------------------------------------------- 3. the fields tell plausible mistakes apart
def _catches(name, cases, true_of, mutant_of):
    caught = [c.name for c in cases if pf.float_mismatches(mutant_of(c), true_of(c))[0] > 0]
    print(f"mutant '{name}': caught by {len(caught)} of {len(cases)} fields: {caught[:6]}{' ...' if len(caught) > 6 else ''}")
    assert caught, f"no field tells '{name}' from the definition"
    return caught


def test_the_variants_without_hooks_are_the_definitions(ao_cases, dof_cases):
    for case in ao_cases[::7]:
        assert pf.float_mismatches(pf.ao_variant(case.z, case.frames[0], case.ao), pf.reference(case, False)[0])[0] == 0, case.name
    for case in dof_cases[::9]:
        assert pf.float_mismatches(pf.dof_variant(pf.circle(case), case.frames[0]), pf.reference(case, False)[0])[0] == 0, case.name


def test_a_gather_bounded_by_the_staged_rectangle_changes_no_bit_and_one_without_the_halo_is_caught(beacons, dof_cases):
    cases = [c for c, _ in beacons if c.shape == pf.BEACON_BIG] + [c for c in dof_cases if "sparse" in c.name]
    for tile in (32, 16):
        for case in cases[:2] + cases[-1:]:
            s = pf.circle(case)
            assert pf.float_mismatches(pf.dof_variant(s, case.frames[0], r2_limit=pf.dof_r2_map(s, tile)), pf.reference(case, False)[0])[0] == 0
        caught = _catches(f"gather bounded by the workgroup's own {tile} x {tile} samples", cases, lambda c: pf.reference(c, False)[0],
                          lambda c: pf.dof_variant(pf.circle(c), c.frames[0], r2_limit=pf.dof_r2_map(pf.circle(c), tile, halo=False)))
        assert any("beacon" in name for name in caught)
    # the samples a body-only bound loses for the beacon on the last sample of workgroup (0, 0)
    case = next(c for c, _ in beacons if c.name.startswith("dof beacon (70, 101) at (31, 31) c=16.0") and "behind" not in c.name)
    s = pf.circle(case)
    lost = pf.changed(pf.dof_variant(s, case.frames[0], r2_limit=pf.dof_r2_map(s, 32, halo=False)), pf.reference(case, False)[0])
    assert int(lost.sum()) == 581


def test_ties_away_from_zero_are_caught():
    _catches("ties rounded away from zero", pf.ao_tie_cases(), lambda c: pf.reference(c, False)[0],
             lambda c: pf.ao_variant(c.z, c.frames[0], c.ao, rint=pf.rint_away))


def test_a_pair_judged_tap_by_tap_is_caught(ao_cases):
    caught = _catches("a pair judged tap by tap", ao_cases[15:25] + [pf.ao_range_case()], lambda c: pf.reference(c, False)[0],
                      lambda c: pf.ao_variant(c.z, c.frames[0], c.ao, per_tap=True))
    assert "ao range edge" in caught


def test_behind_tested_the_wrong_way_is_caught_and_ge_is_the_definition(dof_cases):
    """``behind`` tested with >= cannot be told from the definition by any field: it differs from > only where s_q == s_p,
    and rr is a function of |s|, so there rr_q == rr_p and min(rr_q, rr_p) is rr_q either way (+0 and -0 compare equal and
    have the same rr).  The tie fields show exactly that; the mistake next to it that does change bits, the comparison
    turned round, is caught."""
    cases = [c for c in dof_cases if "plateaus" in c.name or "signed" in c.name or "hills (47, 49)" in c.name]
    assert len(cases) == 7
    for case in cases:
        s = pf.circle(case)
        rr = dof_ref.squared_radius(s)
        assert (rr[:, 1:][s[:, 1:] == s[:, :-1]] == rr[:, :-1][s[:, 1:] == s[:, :-1]]).all()
        assert pf.float_mismatches(pf.dof_variant(s, case.frames[0], behind_ge=True), pf.reference(case, False)[0])[0] == 0, case.name
    print("mutant 'behind tested with >=': equivalent to the definition, caught by no field (equal s have equal rr)")
    caught = _catches("behind tested with <", cases, lambda c: pf.reference(c, False)[0],
                      lambda c: pf.dof_variant(-pf.circle(c), c.frames[0]))
    assert "dof plateaus" in caught


def test_a_step_function_one_float_off_is_caught(native):
    case = pf.step_cases(native)[0]
    acc, rgb = pf.mirror(native, case)
    off = pf.step_off_by_one(native, acc)
    differ = int((off != rgb).sum())
    print(f"mutant 'thresholds one float too high': caught by '{case.name}' at {differ} bytes")
    assert differ == 256                                             # each threshold -- 1.0 is the last and one of STEP_EXTRAS too -- and nothing else
    # uniform colours do not see it: that is the gap these values close
    plain = pf.Case("uniform", np.zeros((16, 16)), np.random.default_rng(1).random((16, 16, 3), dtype=np.float32))
    acc, rgb = pf.mirror(native, plain)
    assert np.array_equal(pf.step_off_by_one(native, acc), rgb)


def test_a_sum_of_one_grid_trip_is_caught():
    big = pf.sum_big_case()
    want = accumulate_ref.accumulate(big.frames, big.weights)
    bad = pf.float_mismatches(pf.sum_one_trip(big.frames, big.weights), want)[0]
    print(f"mutant 'a sum that skips the floats past the first grid trip': caught by '{big.name}' at {bad} floats")
    assert bad == 4 * (525_052 - 524_288)
    for case in pf.sum_cases():                                      # (the largest frame of the older suites, 240 x 320 x 3, is as blind)
        assert pf.float_mismatches(pf.sum_one_trip(case.frames, case.weights), accumulate_ref.accumulate(case.frames, case.weights))[0] == 0
    assert 240 * 320 * 3 // 4 < pf.ACCUM_GRID_LANES


# ---------------------------------------------------------------------------- 4. what the entry refuses, no device
def test_the_entry_is_bound_and_the_abi_stays(native):
    lib = native.load_library()
    assert "mr_debug_post" in native.EXPORTED_SYMBOLS and lib.mr_debug_post is not None
    assert lib.mr_abi_version() == native.ABI_VERSION == 4
    assert lib.mr_abi_struct_size(7) == -1, "the struct-size table grew"


def test_the_entry_refuses_before_any_device_call(native):
    lib = native.load_library()
    handle = lib.mr_scene_create()
    h, w = 4, 8
    frames, z = np.ones((2, h, w, 3), np.float32), np.full((h, w), 2.0)
    weights = np.array([0.5, 0.5])
    out, rgb = np.empty((h, w, 3), np.float32), np.empty((h, w, 3), np.uint8)
    ao = native.fill_ao_desc(pf.SimpleNamespace(**ao_ref.params()), pf.IDENTITY, 9.0, 1)
    dof = native.fill_dof_desc(pf.IDENTITY, 2.0, 1, 3.0)

    def call(**o):
        a = dict(sc=handle, frames=frames.ctypes.data, z=z.ctypes.data, n=2, h=h, w=w, ao=C.byref(ao), ao_shape=0, dof=C.byref(dof),
                 dof_shape=0, weights=weights.ctypes.data, shift=0, scale=1.0, out=out.ctypes.data, rgb=rgb.ctypes.data)
        a.update(o)
        return lib.mr_debug_post(a["sc"], a["frames"], a["z"], a["n"], a["h"], a["w"], a["ao"], a["ao_shape"], a["dof"], a["dof_shape"],
                                 a["weights"], a["shift"], a["scale"], a["out"], a["rgb"])

    bad_ao = native.fill_ao_desc(pf.SimpleNamespace(**ao_ref.params(strength=9.0)), pf.IDENTITY, 9.0, 1)
    bad_dof = native.fill_dof_desc(pf.IDENTITY, 0.0, 1, 3.0)
    tiny = np.array([0.5, 1e-46])
    refused = [("NULL", dict(sc=None)), ("NULL", dict(frames=None)), ("NULL", dict(z=None)), ("NULL", dict(out=None)),
               ("n must", dict(n=0)), ("resolution", dict(h=0)), ("resolution", dict(w=-3)), ("resolution", dict(h=32768)),
               ("resolution", dict(w=40000)), ("need weights", dict(weights=None)),
               ("shape of k_ao", dict(ao_shape=3)), ("shape of k_ao", dict(ao_shape=-1)), ("shape of k_dof", dict(dof_shape=3)),
               ("shape of k_dof", dict(dof_shape=-1)), ("shift is", dict(shift=3)), ("shift is", dict(shift=-1)),
               ("multiples", dict(h=3, shift=1)), ("multiples", dict(w=6, shift=2)),
               ("scale", dict(scale=0.0)), ("scale", dict(scale=float("nan"))), ("scale", dict(scale=1e39)),
               ("weight", dict(weights=tiny.ctypes.data)), ("weight", dict(weights=np.array([1.0, -1.0]).ctypes.data)),
               ("strength", dict(ao=C.byref(bad_ao))), ("kf must", dict(dof=C.byref(bad_dof)))]
    for word, over in refused:
        assert call(**over) == native.MR_E_INVALID, over
        assert word.encode() in lib.mr_last_error(), (over, lib.mr_last_error())
    # a shape is looked at only with its description; nothing above reached a device, and the scene's counters stand
    for name in ("mr_debug_ao", "mr_debug_dof"):
        counters = np.full(3, -1, np.int32)
        assert getattr(lib, name)(handle, counters.ctypes.data) == 0 and counters.tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="need weights"):
        native.debug_post(handle, frames, z)
    with pytest.raises(ValueError, match="frames must be"):
        native.debug_post(handle, frames, z[:2])
    with pytest.raises(ValueError, match="2 frames and 3 weights"):
        native.debug_post(handle, frames, z, weights=[1.0, 1.0, 1.0])
    if not lib.mr_device_available():
        assert call() == MR_E_DEVICE                          # a valid call gets as far as the device, and no further
        assert call(ao=None, ao_shape=7, dof=None, dof_shape=-2) == MR_E_DEVICE
    lib.mr_scene_destroy(handle)
