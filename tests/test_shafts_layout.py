"""CPU: the scratch, LDS and register budgets of the light shafts' kernels, read from the compiler's listing.

``shafts.hip`` is compiled once for gfx950 with ``--save-temps``, the way test_bloom_layout.py compiles ``bloom.hip``, and
only the "Kernel info" comment block of every kernel is read: no scratch and no LDS anywhere -- nothing is staged, the
march's source lies in L2 -- and no more registers than csrc/kernels_shafts.h and DESIGN.md 6o state: the tree of
``k_shaft_source<D>`` stays in registers at every D.  Skipped where there is no hipcc.
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
# what kernels_shafts.h and DESIGN.md 6o state: k_shaft_source<1 .. 4>, and the two others by name
SOURCE_VGPRS = {1: 26, 2: 68, 3: 76, 4: 80}
OTHERS_VGPRS = {"k_shaft_march": 36, "k_shaft_composite": 28}


def _hipcc():
    return os.environ.get("HIPCC") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc"))


@pytest.fixture(scope="module")
def kernel_info(tmp_path_factory):
    """mangled kernel name -> {key: value} for every kernel of shafts.hip."""
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("no hipcc")
    work = tmp_path_factory.mktemp("listing")
    cmd = [hipcc, *entry.HIPCC_FLAGS, "--save-temps", "-o", str(work / "lib.so"), os.path.join(entry.CSRC, "shafts.hip")]
    got = subprocess.run(cmd, cwd=work, capture_output=True, text=True)
    assert got.returncode == 0, got.stderr[-3000:]
    listing = [f for f in os.listdir(work) if f.endswith("gfx950.s")]
    assert len(listing) == 1, os.listdir(work)
    text = (work / listing[0]).read_text()
    info = {}
    for m in re.finditer(r"^(_ZN2mr\d+k_shaft_\w+):", text, re.M):
        block = re.search(r"^; Kernel info:\n((?:;.*\n)+)", text[m.end():], re.M)
        assert block, m.group(1)
        info[m.group(1)] = {k: int(re.search(r"^; %s: (\d+)" % k, block.group(1), re.M).group(1)) for k in KEYS}
    return info


def test_the_header_states_the_registers():
    header = open(os.path.join(entry.CSRC, "kernels_shafts.h")).read()
    stated = ", ".join(str(SOURCE_VGPRS[d]) for d in (1, 2, 3)) + f" and {SOURCE_VGPRS[4]} registers at D = 1 .. 4"
    assert stated in header and "No LDS, no scratch, no atomics." in header
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design.split("## 6o.")[1].split("\n## ")[0]
    assert "26, 68, 76 and 80 VGPRs" in section
    assert f"{OTHERS_VGPRS['k_shaft_march']} VGPRs" in section.split("`k_shaft_march`:")[1].split("\n- ")[0]
    assert f"{OTHERS_VGPRS['k_shaft_composite']} VGPRs" in section.split("`k_shaft_composite`:")[1].split("\n\n")[0]


def test_every_kernel_keeps_to_its_budget(kernel_info):
    source = {}
    for name, k in kernel_info.items():
        m = re.match(r"_ZN2mr14k_shaft_sourceILi(\d)EE", name)
        if m:
            source[int(m.group(1))] = k
    assert set(source) == {1, 2, 3, 4}, sorted(kernel_info)
    for d, k in sorted(source.items()):
        print(f"k_shaft_source<{d}>: {k}")
        assert k["ScratchSize"] == 0 and k["LDSByteSize"] == 0, (d, k)
        assert k["NumVgprs"] <= SOURCE_VGPRS[d], (d, k)
        assert k["Occupancy"] >= 6, (d, k)
    others = {name: k for name, k in kernel_info.items() if "k_shaft_source" not in name}
    assert len(others) == 2, sorted(others)
    for short, stated in OTHERS_VGPRS.items():
        (name, k), = [(n, k) for n, k in others.items() if short in n]
        print(f"{name}: {k}")
        assert k["ScratchSize"] == 0 and k["LDSByteSize"] == 0, (name, k)
        assert k["NumVgprs"] <= stated and k["Occupancy"] == 8, (name, k)
    assert len(kernel_info) == 6
