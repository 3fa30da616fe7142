"""CPU: the scratch and LDS budgets of the tone mapping's kernels, read from the compiler's listing.

``tonemap.hip`` is compiled once for gfx950 with ``--save-temps``, the way test_bloom_layout.py compiles ``bloom.hip``, and
only the "Kernel info" comment block of every instantiation is read: no scratch anywhere, no more LDS in ``k_lum_hist`` (both
forms) and ``k_exposure`` than csrc/kernels_tonemap.h states -- 256 bins of four bytes; those, and 256 pairs of int64 -- none
in ``k_tone_apply``, and six instantiations in all.  Skipped where there is no hipcc.
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
STATED = {"TONE_HIST_LDS": 1024, "TONE_EXPOSURE_LDS": 5120}


def _hipcc():
    return os.environ.get("HIPCC") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc"))


@pytest.fixture(scope="module")
def kernel_info(tmp_path_factory):
    """mangled kernel name -> {key: value} for every kernel of tonemap.hip."""
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("no hipcc")
    work = tmp_path_factory.mktemp("listing")
    cmd = [hipcc, *entry.HIPCC_FLAGS, "--save-temps", "-o", str(work / "lib.so"), os.path.join(entry.CSRC, "tonemap.hip")]
    got = subprocess.run(cmd, cwd=work, capture_output=True, text=True)
    assert got.returncode == 0, got.stderr[-3000:]
    listing = [f for f in os.listdir(work) if f.endswith("gfx950.s")]
    assert len(listing) == 1, os.listdir(work)
    text = (work / listing[0]).read_text()
    info = {}
    for m in re.finditer(r"^(_ZN2mr\d+k_(?:lum_hist|exposure|tone_apply)\w*):", text, re.M):
        block = re.search(r"^; Kernel info:\n((?:;.*\n)+)", text[m.end():], re.M)
        assert block, m.group(1)
        info[m.group(1)] = {k: int(re.search(r"^; %s: (\d+)" % k, block.group(1), re.M).group(1)) for k in KEYS}
    return info


def test_the_header_states_the_bytes():
    header = open(os.path.join(entry.CSRC, "kernels_tonemap.h")).read()
    assert "constexpr int TONE_HIST_LDS = TONE_BINS * 4;" in header
    assert "constexpr int TONE_EXPOSURE_LDS = TONE_BINS * (4 + 8 + 8);" in header
    assert "constexpr int TONE_BINS = 256;" in open(os.path.join(entry.CSRC, "tonemap_def.h")).read()
    assert STATED == {"TONE_HIST_LDS": 256 * 4, "TONE_EXPOSURE_LDS": 256 * 20}
    assert "1 024 bytes" in header and "5 120 bytes" in header, "the comment states the same figures"


def test_every_instantiation_keeps_to_its_budget(kernel_info):
    for name, k in sorted(kernel_info.items()):
        print(f"{name}: {k}")
        assert k["ScratchSize"] == 0, (name, k)
    hist = {name: k for name, k in kernel_info.items() if "k_lum_hist" in name}
    assert sorted(re.search(r"k_lum_histILb([01])E", n).group(1) for n in hist) == ["0", "1"], sorted(kernel_info)
    for name, k in hist.items():
        assert 0 < k["LDSByteSize"] <= STATED["TONE_HIST_LDS"], (name, k)
    exposure = [k for name, k in kernel_info.items() if "k_exposure" in name]
    assert len(exposure) == 1 and 0 < exposure[0]["LDSByteSize"] <= STATED["TONE_EXPOSURE_LDS"], exposure
    apply = {name: k for name, k in kernel_info.items() if "k_tone_apply" in name}
    assert sorted(re.search(r"k_tone_applyILi(\d)E", n).group(1) for n in apply) == ["0", "1", "2"], sorted(kernel_info)
    for name, k in apply.items():
        assert k["LDSByteSize"] == 0, (name, k)
    assert len(kernel_info) == 6
