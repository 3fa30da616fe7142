"""CPU: the scratch and LDS budgets of ``k_taa``, read from the compiler's listing.

``taa.hip`` is compiled once for gfx950 with ``--save-temps``, the way test_kernel_budget.py compiles ``mi355rast.hip``, and
only the "Kernel info" comment block of every instantiation is read: no scratch, and no more LDS than csrc/kernels_taa.h
states for that workgroup shape -- the staged rectangle and its one-sample halo, (TW + 2) * (TH + 2) * 12 bytes.  Skipped
where there is no hipcc.
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

import taa_fields as tf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry          # noqa: E402

KEYS = ("NumVgprs", "ScratchSize", "Occupancy", "LDSByteSize")
# what kernels_taa.h states, shape by shape (its table holds the same figures, spelled with a thin gap)
STATED = {(32, 8): 4080, (64, 4): 4752, (16, 16): 3888}


def _hipcc():
    return os.environ.get("HIPCC") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc"))


@pytest.fixture(scope="module")
def kernel_info(tmp_path_factory):
    """(TW, TH, BLOCK) -> {key: value} for every k_taa instantiation."""
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("no hipcc")
    work = tmp_path_factory.mktemp("listing")
    cmd = [hipcc, *entry.HIPCC_FLAGS, "--save-temps", "-o", str(work / "lib.so"), os.path.join(entry.CSRC, "taa.hip")]
    got = subprocess.run(cmd, cwd=work, capture_output=True, text=True)
    assert got.returncode == 0, got.stderr[-3000:]
    listing = [f for f in os.listdir(work) if f.endswith("gfx950.s")]
    assert len(listing) == 1, os.listdir(work)
    text = (work / listing[0]).read_text()
    info = {}
    for m in re.finditer(r"^(_ZN2mr5k_taaILi(\d+)ELi(\d+)ELi(\d+)E\w+):", text, re.M):
        block = re.search(r"^; Kernel info:\n((?:;.*\n)+)", text[m.end():], re.M)
        assert block, m.group(1)
        info[tuple(int(m.group(k)) for k in (2, 3, 4))] = {k: int(re.search(r"^; %s: (\d+)" % k, block.group(1), re.M).group(1)) for k in KEYS}
    return info


def test_the_header_states_the_rectangles_bytes():
    header = open(os.path.join(entry.CSRC, "kernels_taa.h")).read()
    assert "(tw + 2) * (th + 2) * 3 * (int)sizeof(float)" in header
    for (tw, th), stated in STATED.items():
        assert stated == (tw + 2) * (th + 2) * 12
        assert re.search(r"%d x +%d samples, 256 threads +%s bytes" % (tw, th, f"{stated:,}".replace(",", " ")), header), (tw, th)
    assert set(STATED) == set(tf.TAA_TILES), "the shapes the fields are sized for"


def test_every_instantiation_keeps_to_its_budget(kernel_info):
    assert set(kernel_info) == {(tw, th, tw * th) for tw, th in STATED}, sorted(kernel_info)
    for (tw, th, block), k in sorted(kernel_info.items()):
        print(f"k_taa<{tw}, {th}, {block}>: {k}")
        assert k["ScratchSize"] == 0, (tw, th, k)
        assert k["LDSByteSize"] <= STATED[(tw, th)], (tw, th, k)
