"""CPU: ``tri_touches_tile`` (csrc/tri_reject.h), the rule by which ``k_bin_work`` leaves a large triangle out of the
list of a tile it cannot cover, compiled for the host and held to the kernels' own float32 coverage test by
``tools/host_tri_reject_check.cpp`` (a stand-alone program, no HIP runtime, ``-ffp-contract=off``).

The program builds set-up records from seeded triangles (well-shaped, slivers, near-degenerate, far off the screen, and
c4's two floor triangles from the capture's matrices) and walks all 256 samples of every tile of their boxes: no
rejected tile may hold a covered sample, over more than a million (triangle, tile) pairs; and so that the rule cannot
pass by rejecting nothing, every tile of a triangle with smallest angle >= 5 degrees and corners within +-8192 whose
samples all lie more than a pixel outside one edge must be rejected.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tools", "host_tri_reject_check.cpp")
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


def test_no_rejected_tile_holds_a_covered_sample(tmp_path):
    exe = _build(tmp_path, "host_tri_reject_check", ["-O2"])
    got = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(got.stdout)
    assert got.returncode == 0 and "host_tri_reject_check: ok" in got.stdout, got.stdout[-3000:] + got.stderr[-2000:]
    pairs, rejected, must = (int(v) for v in re.search(r"total (\d+) pairs, (\d+) rejected, (\d+) had to be rejected", got.stdout).groups())
    assert pairs >= 10 ** 6 and rejected >= must > 0
    # c4's floor: about half of the (floor triangle, tile) pairs of the two boxes go
    floor = re.search(r"c4 floor\s+2 triangles \(0 dropped by the set-up\),\s+(\d+) pairs,\s+(\d+) rejected", got.stdout)
    assert floor and int(floor.group(2)) * 3 > int(floor.group(1))


def test_the_check_is_clean_under_the_sanitizers(tmp_path):
    """The same program (its own ``main``, nothing loaded into Python) under AddressSanitizer and UBSan, on fewer
    triangles."""
    probe = subprocess.run([_compiler(), "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(tmp_path / "probe")],
                           input="int main() { return 0; }\n", capture_output=True, text=True, timeout=120)
    if probe.returncode != 0:
        pytest.skip("this compiler has no sanitizer runtime")
    exe = _build(tmp_path, "host_tri_reject_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    got = subprocess.run([exe, "30"], capture_output=True, text=True, timeout=300)
    assert got.returncode == 0 and "host_tri_reject_check: ok" in got.stdout, got.stdout[-3000:] + got.stderr[-3000:]


def test_the_kernel_uses_the_checked_function():
    """k_bin_work compiles the very header the program checks, and the switch reaches it as a kernel argument."""
    text = lambda name: open(os.path.join(CSRC, name)).read()
    assert '#include "tri_reject.h"' in text("kernels_bin.h")
    assert "tri_touches_tile(a.tris[id], tx * TILE_W, tile_row_frame(fc, ty) * TILE_H)" in text("kernels_bin.h")
    assert "MR_BIG_TRI_REJECT" in text("host_env.h") and "p.env.big_tri_reject" in text("host_frame.h")
