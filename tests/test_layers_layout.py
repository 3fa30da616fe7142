"""CPU: the scratch and LDS budgets of ``k_layers``, read from the compiler's listing.

``layers.hip`` is compiled once for gfx950 with ``--save-temps``, the way test_tonemap_layout.py compiles ``tonemap.hip``, and
only the "Kernel info" comment block of the two instantiations is read: no scratch, no LDS, and the register counts, which
csrc/kernels_layers.h records, within the 64 of eight wavefronts a SIMD.  Skipped where there is no hipcc.
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
    """mangled kernel name -> {key: value} for every kernel of layers.hip."""
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("no hipcc")
    work = tmp_path_factory.mktemp("listing")
    cmd = [hipcc, *entry.HIPCC_FLAGS, "--save-temps", "-o", str(work / "lib.so"), os.path.join(entry.CSRC, "layers.hip")]
    got = subprocess.run(cmd, cwd=work, capture_output=True, text=True)
    assert got.returncode == 0, got.stderr[-3000:]
    listing = [f for f in os.listdir(work) if f.endswith("gfx950.s")]
    assert len(listing) == 1, os.listdir(work)
    text = (work / listing[0]).read_text()
    info = {}
    for m in re.finditer(r"^(_ZN2mr\d+k_layers\w*):", text, re.M):
        block = re.search(r"^; Kernel info:\n((?:;.*\n)+)", text[m.end():], re.M)
        assert block, m.group(1)
        info[m.group(1)] = {k: int(re.search(r"^; %s: (\d+)" % k, block.group(1), re.M).group(1)) for k in KEYS}
    return info


def _recorded():
    """The register counts csrc/kernels_layers.h records: {'true': vgprs, 'false': vgprs}."""
    header = open(os.path.join(entry.CSRC, "kernels_layers.h")).read()
    found = dict(re.findall(r"k_layers<(true|false)>: (\d+) VGPRs", header))
    return {k: int(v) for k, v in found.items()}


def test_the_header_records_the_register_counts():
    assert sorted(_recorded()) == ["false", "true"]
    assert "No LDS, no scratch, no atomics, no memset." in open(os.path.join(entry.CSRC, "kernels_layers.h")).read()


def test_both_instantiations_keep_to_their_budget(kernel_info):
    recorded = _recorded()
    for name, k in sorted(kernel_info.items()):
        print(f"{name}: {k}")
    assert sorted(re.search(r"k_layersILb([01])E", n).group(1) for n in kernel_info) == ["0", "1"], sorted(kernel_info)
    for name, k in kernel_info.items():
        which = "true" if "ILb1E" in name else "false"
        assert k["ScratchSize"] == 0, (name, k)
        assert k["LDSByteSize"] == 0, (name, k)
        # (the recorded count is this compiler's; what must hold under any is the budget of eight wavefronts a SIMD)
        assert recorded[which] <= 64 and k["NumVgprs"] <= 64, f"{name}: {k['NumVgprs']} VGPRs, csrc/kernels_layers.h records {recorded[which]}"
        assert k["Occupancy"] == 8, (name, k)
