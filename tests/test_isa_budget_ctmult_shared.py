"""Build-quality guard for the kernels of the shared-selector path of the ciphertext-multiplication mode
(pir_amd/csrc/ctmult_shared.hip; no GPU needed: hipcc cross-compiles gfx950 here), in the manner of
tests/test_isa_budget_ctmult_deferred.py: the file holds exactly the lift of single polynomials for k = 1 .. 6 and ONE
instantiation of each tensor kernel (the modulus comes from blockIdx, not from a template); every one of them runs
without scratch and without LDS in at most 128 VGPRs."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pir_amd", "csrc", "ctmult_shared.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

LIFTS = ["ctm_lift_polys_kernelILi%dEE" % k for k in range(1, 7)]
KERNELS = LIFTS + ["ctm_tensor_sel_kernelE", "ctm_tensor_rowsum_sel_kernelE"]


@pytest.fixture(scope="module")
def descriptors(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "ctmult_shared.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only", "-S", SRC,
                    "-o", str(out)], check=True, capture_output=True, timeout=600)
    isa = out.read_text().split("\n")
    found = {}
    for i, l in enumerate(isa):
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", l)
        if m:
            block = "\n".join(isa[i:i + 40])
            found[m.group(1)] = (int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", block).group(1)),
                                 int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", block).group(1)),
                                 int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", block).group(1)))
    return found


def test_every_kernel_of_the_file_is_listed(descriptors):
    assert len(descriptors) == len(KERNELS), sorted(descriptors)


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_no_lds_and_four_waves_per_simd(descriptors, kernel):
    names = [n for n in descriptors if kernel in n]
    assert len(names) == 1, (kernel, names)
    vgprs, scratch, lds = descriptors[names[0]]
    assert scratch == 0, "%s spills %d bytes per lane" % (kernel, scratch)
    assert lds == 0, "%s uses %d bytes of LDS" % (kernel, lds)
    assert vgprs <= 128, "%s needs %d VGPRs" % (kernel, vgprs)
