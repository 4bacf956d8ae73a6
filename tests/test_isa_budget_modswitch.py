"""Build-quality guard for mod_switch_kernel (no GPU needed: hipcc cross-compiles gfx950 here).

The kernel keeps the k residues of its two coefficients in registers through the k - r drop steps (DESIGN.md section
6.4): the residue array is indexed with compile-time constants only.  An edit that indexes it with a run-time value sends
it to scratch memory -- still correct, several times slower, and no other test would notice.  Both store forms (in place
with stride k, compact) must use no scratch and stay a small kernel."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pir_amd", "csrc", "kernels.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "kernels.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only", "-S", SRC,
                    "-o", str(out)], check=True, capture_output=True, timeout=600)
    return out.read_text().split("\n")


def _descriptor(isa, prefix):
    i = next(i for i, l in enumerate(isa) if ".amdhsa_kernel " + prefix in l)
    block = "\n".join(isa[i:i + 40])
    return (int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", block).group(1)),
            int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", block).group(1)),
            int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", block).group(1)))


@pytest.mark.parametrize("form,kernel", [("compact", "_ZN6pirgpu17mod_switch_kernelILb1EE"),
                                         ("in place", "_ZN6pirgpu17mod_switch_kernelILb0EE")])
def test_mod_switch_kernel_uses_no_scratch(isa, form, kernel):
    vgprs, scratch, lds = _descriptor(isa, kernel)
    print("mod_switch_kernel (%s): %d VGPRs, %d bytes of scratch, %d bytes of LDS" % (form, vgprs, scratch, lds))
    assert scratch == 0, "mod_switch_kernel (%s) spills %d bytes per lane" % (form, scratch)
    assert lds == 0
    # 8 residues x 2 coefficients x 2 dwords = 32 VGPRs of data; with 128 or fewer the kernel keeps 4 waves per SIMD
    assert vgprs <= 128, "mod_switch_kernel (%s) needs %d VGPRs" % (form, vgprs)
