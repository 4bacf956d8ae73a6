"""Register budget of the database pass over several tables (scan_mfma_runs_kernel, scan_mfma.hip): every instantiation
shares its body with a scan_mfma_kernel twin and must keep the twin's caps -- 8-wave workgroups run two waves per SIMD:
at most 256 registers per wave, no scratch (tests/test_isa_budget.py holds the twins to the same).  No GPU needed: hipcc
cross-compiles gfx950 here."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN_SRC = os.path.join(ROOT, "pir_amd", "csrc", "scan_mfma.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

VARIANTS = [(5, 1), (5, 2), (5, 3), (6, 1), (6, 2), (7, 1), (7, 2)]


@pytest.fixture(scope="module")
def scan_isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "scan.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only", "-S", SCAN_SRC,
                    "-o", str(out)], check=True, capture_output=True, timeout=600)
    return out.read_text().split("\n")


def _descriptor(isa, kernel, L, KS, top4, f64_fold):
    name = "_ZN6pirgpu%d%sILi%dELi%dELi8ELb%dELb%dEEE" % (len(kernel), kernel, L, KS, 1 if top4 else 0, 1 if f64_fold else 0)
    i = next(i for i, l in enumerate(isa) if ".amdhsa_kernel " + name in l)
    block = "\n".join(isa[i:i + 45])
    get = lambda key: int(re.search(r"\.amdhsa_%s (\d+)" % key, block).group(1))
    return get("next_free_vgpr"), get("private_segment_fixed_size"), get("group_segment_fixed_size")


# (the nibble form of the top digit is not built for L = 7)
CASES = [(L, KS, top4, fold) for L, KS in VARIANTS for top4 in ((True, False) if L <= 6 else (False,)) for fold in (True, False)]


@pytest.mark.parametrize("L,KS,top4,f64_fold", CASES)
def test_runs_kernel_keeps_its_twins_budget(scan_isa, L, KS, top4, f64_fold):
    total, scratch, lds = _descriptor(scan_isa, "scan_mfma_runs_kernel", L, KS, top4, f64_fold)
    assert total <= 256 and scratch == 0, (L, KS, top4, f64_fold, total, scratch)
    _, _, twin_lds = _descriptor(scan_isa, "scan_mfma_kernel", L, KS, top4, f64_fold)
    assert lds == twin_lds, (lds, twin_lds)


def test_every_built_runs_variant_is_listed_here(scan_isa):
    built = set()
    for l in scan_isa:
        m = re.search(r"\.amdhsa_kernel _ZN6pirgpu21scan_mfma_runs_kernelILi(\d)ELi(\d)ELi(\d)E", l)
        if m:
            built.add((int(m.group(1)), int(m.group(2)), int(m.group(3))))
    assert built == {(L, KS, 8) for L, KS in VARIANTS}
