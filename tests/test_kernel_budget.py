"""CPU: the register, scratch, occupancy and LDS budgets of ``k_tile`` and ``k_setup``, read from the compiler's listing.

The single-light tile kernel runs six wavefronts per SIMD only while it fits 80 vector registers without scratch
(kernels_tile.h, ``K_TILE_WAVES_1L``); a register more and the frame is some 10 % slower with no test failing.  The
library is compiled once for gfx950 with ``--save-temps`` and only the "Kernel info" comment block of every instantiation
is read.  Skipped where there is no hipcc.
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry          # noqa: E402

KEYS = ("NumVgprs", "ScratchSize", "Occupancy", "LDSByteSize")


def _hipcc():
    return os.environ.get("HIPCC") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc"))


@pytest.fixture(scope="module")
def kernel_info(tmp_path_factory):
    """mangled name -> {key: value} for every k_tile / k_setup instantiation."""
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("no hipcc")
    work = tmp_path_factory.mktemp("listing")
    cmd = [hipcc, *entry.HIPCC_FLAGS, "--save-temps", "-o", str(work / "lib.so"), os.path.join(entry.CSRC, "mi355rast.hip")]
    got = subprocess.run(cmd, cwd=work, capture_output=True, text=True)
    assert got.returncode == 0, got.stderr[-3000:]
    listing = [f for f in os.listdir(work) if f.endswith("gfx950.s")]
    assert len(listing) == 1, os.listdir(work)
    text = (work / listing[0]).read_text()
    info = {}
    for m in re.finditer(r"^(_ZN2mr(?:6k_tile|7k_setup)I\w+):", text, re.M):
        block = re.search(r"^; Kernel info:\n((?:;.*\n)+)", text[m.end():], re.M)
        assert block, m.group(1)
        vals = {k: int(re.search(r"^; %s: (\d+)" % k, block.group(1), re.M).group(1)) for k in KEYS}
        info[m.group(1)] = vals
    return info


def _pick(info, kernel, flags):
    """the instantiation kernel<flags...>"""
    want = kernel + "I" + "".join("Lb%dE" % f for f in flags) + "E"
    names = [n for n in info if want in n]
    assert len(names) == 1, (want, sorted(info))
    return info[names[0]]


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("ss", [0, 1])
def test_single_light_tile_kernel_keeps_six_wavefronts(kernel_info, split, ss):
    k = _pick(kernel_info, "6k_tile", (split, ss, 0))
    print(f"k_tile<{split}, {ss}, false>: {k}")
    assert k["NumVgprs"] <= 80 and k["ScratchSize"] == 0 and k["Occupancy"] == 6 and k["LDSByteSize"] <= 17896, k


@pytest.mark.parametrize("pre", [0, 1])
def test_single_light_setup_kernel(kernel_info, pre):
    k = _pick(kernel_info, "7k_setup", (pre, 0))
    print(f"k_setup<{pre}, false>: {k}")
    assert k["NumVgprs"] <= 96 and k["ScratchSize"] == 0 and k["Occupancy"] == 5, k


def test_multi_light_kernels_are_no_worse(kernel_info):
    picks = [_pick(kernel_info, "6k_tile", (0, ss, 1)) for ss in (0, 1)] + [_pick(kernel_info, "7k_setup", (pre, 1)) for pre in (0, 1)]
    for k in picks:
        print(k)
        assert k["NumVgprs"] <= 96 and k["ScratchSize"] <= 100 and k["Occupancy"] >= 5, k
