"""Register, scratch and LDS budgets of the paired scan kernels (pir_amd/csrc/scan_mfma_pair.hip), and the single kernels'
descriptors they must leave alone (no GPU needed: hipcc cross-compiles gfx950, as tests/test_isa_budget.py does).

A pair kernel is one 8-wave workgroup per CU: two waves per SIMD get 256 registers each, the second group's selector tiles
(8 x KS x L KiB) and the result staging (36 KiB) share the CU's 160 KiB of LDS."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pir_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
STAGING = 2 * 16 * 16 * 9 * 8


def _isa(tmp_path_factory, source):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / (source + ".s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only", "-S",
                    os.path.join(CSRC, source), "-o", str(out)], check=True, capture_output=True, timeout=600)
    return out.read_text().split("\n")


@pytest.fixture(scope="module")
def pair_isa(tmp_path_factory):
    return _isa(tmp_path_factory, "scan_mfma_pair.hip")


@pytest.fixture(scope="module")
def scan_isa(tmp_path_factory):
    return _isa(tmp_path_factory, "scan_mfma.hip")


def _descriptor(isa, name):
    i = next(i for i, l in enumerate(isa) if ".amdhsa_kernel " + name in l)
    block = "\n".join(isa[i:i + 40])
    get = lambda key: int(re.search(r"\.amdhsa_%s (\d+)" % key, block).group(1))
    return get("next_free_vgpr"), get("private_segment_fixed_size"), get("group_segment_fixed_size")


@pytest.mark.parametrize("f64_fold", [True, False])
@pytest.mark.parametrize("top4", [True, False])
@pytest.mark.parametrize("KS", [1, 2, 3])
def test_pair_kernels_fit_two_waves_per_simd_and_the_lds(pair_isa, KS, top4, f64_fold):
    name = "_ZN6pirgpu21scan_mfma_pair_kernelILi5ELi%dELb%dELb%dEEE" % (KS, top4, f64_fold)
    vgprs, scratch, lds = _descriptor(pair_isa, name)
    assert vgprs <= 256 and scratch == 0 and lds <= 163840, (KS, top4, f64_fold, vgprs, scratch, lds)
    assert lds == 8 * KS * 5 * 1024 + STAGING, lds      # the selector tiles are stored expanded: L KiB per k-step and wave


def test_every_instantiated_pair_kernel_is_covered(pair_isa):
    names = [l for l in pair_isa if ".amdhsa_kernel " in l and "scan_mfma_pair_kernel" in l]
    assert len(names) == 12, names


@pytest.mark.parametrize("f64_fold,vgprs", [(True, 226), (False, 230)])
def test_single_kernels_of_the_headline_shape_are_unchanged(scan_isa, f64_fold, vgprs):
    """scan_mfma_kernel<5, 3, 8, true, *>: the pair kernel has a body of its own, so these compile to what they did."""
    name = "_ZN6pirgpu16scan_mfma_kernelILi5ELi3ELi8ELb1ELb%dEEE" % f64_fold
    assert _descriptor(scan_isa, name) == (vgprs, 0, STAGING)
