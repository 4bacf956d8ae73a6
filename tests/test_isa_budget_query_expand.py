"""Register and scratch budget of the compact-query unpack kernel (pir_amd/csrc/query_expand.hip; no GPU needed: hipcc
cross-compiles gfx950, as tests/test_isa_budget_scan_pair.py does).  One thread owns one coefficient and keeps two source
words in registers: no scratch, and far below the 128 registers at which a SIMD still holds four waves."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pir_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "query_expand.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only", "-S",
                    os.path.join(CSRC, "query_expand.hip"), "-o", str(out)], check=True, capture_output=True, timeout=600)
    return out.read_text().split("\n")


def test_query_unpack_kernel_has_no_scratch_and_at_most_128_vgprs(isa):
    heads = [i for i, l in enumerate(isa) if ".amdhsa_kernel " in l]
    assert len(heads) == 1 and "query_unpack_kernel" in isa[heads[0]], [isa[i] for i in heads]
    block = "\n".join(isa[heads[0]:heads[0] + 40])
    get = lambda key: int(re.search(r"\.amdhsa_%s (\d+)" % key, block).group(1))
    assert get("next_free_vgpr") <= 128 and get("private_segment_fixed_size") == 0 and get("group_segment_fixed_size") == 0


def test_the_file_is_built_into_the_library():
    from pir_amd import build
    assert "query_expand.hip" in build.SOURCES
