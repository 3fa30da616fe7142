"""CPU: the scratch and LDS budgets of the bloom's kernels, read from the compiler's listing.

``bloom.hip`` is compiled once for gfx950 with ``--save-temps``, the way test_taa_layout.py compiles ``taa.hip``, and only
the "Kernel info" comment block of every instantiation is read: no scratch anywhere, no more LDS in ``k_bloom_down`` than
csrc/kernels_bloom.h states for that workgroup shape -- the staged source rectangle, (2 TW + 2) * (2 TH + 2) * 12 bytes --
and none in ``k_bloom_up`` and ``k_bloom_composite``.  Skipped where there is no hipcc.
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

import bloom_fields as bf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry          # noqa: E402

KEYS = ("NumVgprs", "ScratchSize", "Occupancy", "LDSByteSize")
# what kernels_bloom.h states, shape by shape (its table holds the same figures, spelled with a thin gap)
STATED = {(32, 8): 14256, (64, 4): 15600, (16, 16): 13872}


def _hipcc():
    return os.environ.get("HIPCC") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc"))


@pytest.fixture(scope="module")
def kernel_info(tmp_path_factory):
    """mangled kernel name -> {key: value} for every kernel of bloom.hip."""
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("no hipcc")
    work = tmp_path_factory.mktemp("listing")
    cmd = [hipcc, *entry.HIPCC_FLAGS, "--save-temps", "-o", str(work / "lib.so"), os.path.join(entry.CSRC, "bloom.hip")]
    got = subprocess.run(cmd, cwd=work, capture_output=True, text=True)
    assert got.returncode == 0, got.stderr[-3000:]
    listing = [f for f in os.listdir(work) if f.endswith("gfx950.s")]
    assert len(listing) == 1, os.listdir(work)
    text = (work / listing[0]).read_text()
    info = {}
    for m in re.finditer(r"^(_ZN2mr\d+k_bloom_\w+):", text, re.M):
        block = re.search(r"^; Kernel info:\n((?:;.*\n)+)", text[m.end():], re.M)
        assert block, m.group(1)
        info[m.group(1)] = {k: int(re.search(r"^; %s: (\d+)" % k, block.group(1), re.M).group(1)) for k in KEYS}
    return info


def test_the_header_states_the_rectangles_bytes():
    header = open(os.path.join(entry.CSRC, "kernels_bloom.h")).read()
    assert "(2 * tw + 2) * (2 * th + 2) * 3 * (int)sizeof(float)" in header
    for (tw, th), stated in STATED.items():
        assert stated == (2 * tw + 2) * (2 * th + 2) * 12
        assert re.search(r"%d x +%d samples, 256 threads +%s bytes" % (tw, th, f"{stated:,}".replace(",", " ")), header), (tw, th)
    assert set(STATED) == set(bf.BLOOM_TILES), "the shapes the fields are sized for"


def test_every_instantiation_keeps_to_its_budget(kernel_info):
    down = {}
    for name, k in kernel_info.items():
        m = re.match(r"_ZN2mr12k_bloom_downILb([01])ELi(\d+)ELi(\d+)ELi(\d+)E", name)
        if m:
            down[tuple(int(m.group(i)) for i in (1, 2, 3, 4))] = k
    assert set(down) == {(first, tw, th, tw * th) for tw, th in STATED for first in (0, 1)}, sorted(kernel_info)
    for (first, tw, th, block), k in sorted(down.items()):
        print(f"k_bloom_down<{bool(first)}, {tw}, {th}, {block}>: {k}")
        assert k["ScratchSize"] == 0, (first, tw, th, k)
        assert 0 < k["LDSByteSize"] <= STATED[(tw, th)], (first, tw, th, k)
    others = {name: k for name, k in kernel_info.items() if "k_bloom_down" not in name}
    assert len(others) == 2 and any("k_bloom_up" in n for n in others) and any("k_bloom_composite" in n for n in others), sorted(others)
    for name, k in sorted(others.items()):
        print(f"{name}: {k}")
        assert k["ScratchSize"] == 0 and k["LDSByteSize"] == 0, (name, k)
    assert len(kernel_info) == 8
