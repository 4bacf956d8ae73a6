"""Register budget of the seed expansion kernel (seed_expand_kernel, seed_expand.hip): BLAKE2b's sixteen 64-bit state
words and sixteen message words must stay in registers -- no scratch -- which holds only while every index into them
is a literal.  The build of this kernel reports 81 VGPRs (no AGPRs, no scratch, 5 waves per SIMD); the cap is that
count rounded up to the allocation granule of 8: 88.  No GPU needed: hipcc cross-compiles gfx950 here."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pir_amd", "csrc", "seed_expand.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
VGPR_CAP = 88


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "seed_expand.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only", "-S", SRC,
                    "-o", str(out)], check=True, capture_output=True, timeout=600)
    return out.read_text().split("\n")


def _descriptor(isa, kernel):
    i = next(i for i, l in enumerate(isa) if re.search(r"\.amdhsa_kernel _ZN6pirgpu%d%sE" % (len(kernel), kernel), l))
    block = "\n".join(isa[i:i + 45])
    get = lambda key: int(re.search(r"\.amdhsa_%s (\d+)" % key, block).group(1))
    return get("next_free_vgpr"), get("private_segment_fixed_size"), get("group_segment_fixed_size")


def test_seed_expand_kernel_keeps_its_budget(isa):
    vgprs, scratch, lds = _descriptor(isa, "seed_expand_kernel")
    assert scratch == 0, scratch
    assert vgprs <= VGPR_CAP, vgprs
    assert lds <= 40 * 1024, lds          # the window of root hashes: 512 x 64 bytes, and the prefix sum's words


def test_it_is_the_only_kernel_of_the_file(isa):
    assert len([l for l in isa if ".amdhsa_kernel " in l]) == 1
