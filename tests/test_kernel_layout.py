"""CPU: the two variants of ``k_tile`` and ``k_setup`` in the compiler's listing.

``k_tile<SPLIT, SS, ML>`` / ``k_setup<PRE_XFORM, ML>`` are the frame-only kernels (tests/test_kernel_budget.py holds their
registers); ``k_tile_full`` / ``k_setup_full`` are the general ones, the code both names had before the split.  Here: the
general kernels keep the budgets the one kernel had, and the frame-only ones are smaller than it was.  (Cold-block
markers were built and measured -- profiles/frame_only_path_ab.txt section 5 -- and are not in the tree.)  The library is
compiled once for gfx950 with ``--save-temps``, like test_kernel_budget.py, and only the "Kernel info" comment blocks are
read.  Skipped where there is no hipcc.
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

KEYS = ("codeLenInByte", "NumVgprs", "ScratchSize", "Occupancy", "LDSByteSize")
# codeLenInByte of the one k_tile<0, 0, 0> / k_setup<0, 0> before there were two variants (same compiler, same flags)
PARENT_TILE_BYTES, PARENT_SETUP_BYTES = 46944, 41684


def _hipcc():
    return os.environ.get("HIPCC") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc"))


@pytest.fixture(scope="module")
def kernel_info(tmp_path_factory):
    """mangled name -> {key: value} for every instantiation of the four kernels."""
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("no hipcc")
    work = tmp_path_factory.mktemp("layout")
    cmd = [hipcc, *entry.HIPCC_FLAGS, "--save-temps", "-o", str(work / "lib.so"), os.path.join(entry.CSRC, "mi355rast.hip")]
    got = subprocess.run(cmd, cwd=work, capture_output=True, text=True)
    assert got.returncode == 0, got.stderr[-3000:]
    listing = [f for f in os.listdir(work) if f.endswith("gfx950.s")]
    assert len(listing) == 1, os.listdir(work)
    text = (work / listing[0]).read_text()
    info = {}
    for m in re.finditer(r"^(_ZN2mr(?:6k_tile|11k_tile_full|7k_setup|12k_setup_full)I\w+):", text, re.M):
        block = re.search(r"^; Kernel info:\n((?:;.*\n)+)", text[m.end():], re.M)
        assert block, m.group(1)
        info[m.group(1)] = {k: int(re.search(r"^; %s *[:=] *(\d+)" % k, block.group(1), re.M).group(1)) for k in KEYS}
    return info


def _pick(info, kernel, flags):
    """the instantiation kernel<flags...>"""
    want = "_ZN2mr" + kernel + "I" + "".join("Lb%dE" % f for f in flags) + "E"
    names = [n for n in info if n.startswith(want)]
    assert len(names) == 1, (want, sorted(info))
    return info[names[0]]


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("ss", [0, 1])
def test_general_single_light_tile_kernel_keeps_six_wavefronts(kernel_info, split, ss):
    k = _pick(kernel_info, "11k_tile_full", (split, ss, 0))
    print(f"k_tile_full<{split}, {ss}, false>: {k}")
    assert k["NumVgprs"] <= 80 and k["ScratchSize"] == 0 and k["Occupancy"] == 6 and k["LDSByteSize"] <= 17896, k


@pytest.mark.parametrize("pre", [0, 1])
def test_general_single_light_setup_kernel(kernel_info, pre):
    k = _pick(kernel_info, "12k_setup_full", (pre, 0))
    print(f"k_setup_full<{pre}, false>: {k}")
    assert k["NumVgprs"] <= 96 and k["ScratchSize"] == 0 and k["Occupancy"] == 5, k


def test_multi_light_kernels_are_no_worse(kernel_info):
    picks = [_pick(kernel_info, t, (0, ss, 1)) for t in ("6k_tile", "11k_tile_full") for ss in (0, 1)]
    picks += [_pick(kernel_info, s, (pre, 1)) for s in ("7k_setup", "12k_setup_full") for pre in (0, 1)]
    for k in picks:
        print(k)
        assert k["NumVgprs"] <= 96 and k["ScratchSize"] <= 100 and k["Occupancy"] >= 5, k


def test_frame_only_kernels_are_smaller_than_the_one_kernel_was(kernel_info):
    tile, setup = _pick(kernel_info, "6k_tile", (0, 0, 0)), _pick(kernel_info, "7k_setup", (0, 0))
    print(f"k_tile<0, 0, 0>: {tile['codeLenInByte']} B (was {PARENT_TILE_BYTES}); k_setup<0, 0>: {setup['codeLenInByte']} B (was {PARENT_SETUP_BYTES})")
    assert tile["codeLenInByte"] < PARENT_TILE_BYTES
    assert setup["codeLenInByte"] < PARENT_SETUP_BYTES
    # and no frame-only instantiation is larger than its general twin
    for flags in ((0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 0), (0, 0, 1), (0, 1, 1)):
        assert _pick(kernel_info, "6k_tile", flags)["codeLenInByte"] < _pick(kernel_info, "11k_tile_full", flags)["codeLenInByte"], flags
    for flags in ((0, 0), (1, 0), (0, 1), (1, 1)):
        assert _pick(kernel_info, "7k_setup", flags)["codeLenInByte"] < _pick(kernel_info, "12k_setup_full", flags)["codeLenInByte"], flags

