"""CPU: the tile-level depth rule of a shadow quad (csrc/quad_reject.h) -- ``quad_tile_bound``, the float ``k_bin_work``
leaves beside a listed (quad, tile) pair, and ``quad_tile_none``, by which ``k_tile`` drops the quad before it stages it
-- compiled for the host and held to the strip rule and to the per-sample rule by ``tools/host_quad_cull_check.cpp`` (a
stand-alone program, no HIP runtime, ``-ffp-contract=off``).

Over a million seeded cases (planes from flat to steep, both systems, five near / far pairs, the plane's zero line out
to 8 192 pixels from the tile, tiny ``nz``, terms that are not finite, the bound rounded to float32): whenever the tile
rule culls at a limit, ``quad_depth_pass`` is false at all 256 samples against that limit and its two float64
neighbours, and -- where the denominators are positive, the only case the strip rule knows -- the strip rule rejects the
quad in each of the four strips at every limit no more favourable; and so that the rule cannot pass by culling nothing, a
quad whose exact depth loses at every sample by a relative 1e-6 on a sane tile must be culled.

A third of the cases lie beyond the pole of the depth, where every denominator is negative: the frames of a right-handed
camera are of that kind (z is negative there), the strip rule's ``sane`` fails for them and it keeps such a quad for the
walk to find every sample failing.  The tile rule's mirrored comparison (a negative bound) therefore has no strip verdict
to be held to; it is held to the samples alone, and the counts say how many culls were of either kind.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tools", "host_quad_cull_check.cpp")
CSRC = os.path.join(ROOT, "py-numpy-renderer_amd", "csrc")


def _compiler():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    return cxx


def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    got = subprocess.run([_compiler(), "-std=c++17", "-ffp-contract=off", *flags, "-I", CSRC, SOURCE, "-o", exe],
                         capture_output=True, text=True, timeout=300)
    assert got.returncode == 0, got.stderr[-3000:]
    return exe


def test_a_culled_quad_is_rejected_by_every_strip_and_passes_at_no_sample(tmp_path):
    exe = _build(tmp_path, "host_quad_cull_check", ["-O2"])
    got = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(got.stdout)
    assert got.returncode == 0 and "host_quad_cull_check: ok" in got.stdout, got.stdout[-3000:] + got.stderr[-2000:]
    m = re.search(r"(\d+) cases \((\d+) with nz == 0 or a term that is not finite\), (\d+) sane tiles, (\d+) limits tried, "
                  r"(\d+) culls checked against the strips and the samples, (\d+) of them with negative denominators \(the samples "
                  r"alone\), (\d+) vacuity cases, (\d+) failures", got.stdout)
    cases, wild, sane, limits, culls, culls_neg, vacuity, failures = (int(v) for v in m.groups())
    assert cases >= 10 ** 6 and failures == 0
    assert wild > 0 and culls >= cases and vacuity > cases // 2 and sane < cases
    assert culls_neg > cases // 4 and culls - culls_neg > cases // 4          # both kinds of cull, in numbers


def test_the_check_is_clean_under_the_sanitizers(tmp_path):
    """The same program (its own ``main``, nothing loaded into Python) under AddressSanitizer and UBSan, on fewer cases."""
    probe = subprocess.run([_compiler(), "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")],
                           input="int main() { return 0; }\n", capture_output=True, text=True, timeout=120)
    if probe.returncode != 0:
        pytest.skip("this compiler has no sanitizer runtime")
    exe = _build(tmp_path, "host_quad_cull_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    got = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=300)
    assert got.returncode == 0 and "host_quad_cull_check: ok" in got.stdout, got.stdout[-3000:] + got.stderr[-3000:]


def test_the_kernels_use_the_checked_functions():
    """k_bin_work and k_tile compile the very header the program checks, the bound travels beside the quad list, and the
    switch reaches k_tile as a kernel argument."""
    text = lambda name: open(os.path.join(CSRC, name)).read()
    assert '#include "quad_reject.h"' in text("kernels_bin.h")
    assert "a.quad_bound[(size_t)tile * a.cap[2] + pos] = quad_tile_bound(" in text("kernels_bin.h")
    tile = text("kernels_tile.h")
    assert "quad_tile_none(ta.quad_bound[(size_t)tile * ta.cap[2] + qbase + lane]" in tile
    assert "quad_rect_verdict(" in tile and "bool quad_depth_pass(" not in tile      # one copy of each rule, in the header
    assert "MR_QUAD_TILE_CULL" in text("host_env.h") and "p.env.quad_tile_cull" in text("host_frame.h")
