"""Build-quality guard for reply_pack_kernel (no GPU needed: hipcc cross-compiles gfx950 here).

The kernel builds one output word per thread in registers: one accumulator, one coefficient, the
widths and offsets read from its by-value argument block with a workgroup-uniform index.  An edit that copies that
block to a lane-private array, or indexes it per lane, sends it to scratch memory -- still correct, slower, and no
other test would notice.  The VGPR cap is what the build reports today: a regression guard, not a target."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pir_amd", "csrc", "reply_pack.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "reply_pack.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only", "-S", SRC,
                    "-o", str(out)], check=True, capture_output=True, timeout=600)
    return out.read_text().split("\n")


def test_reply_pack_kernel_uses_no_scratch(isa):
    i = next(i for i, l in enumerate(isa) if ".amdhsa_kernel _ZN6pirgpu17reply_pack_kernelE" in l)
    block = "\n".join(isa[i:i + 40])
    vgprs = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", block).group(1))
    scratch = int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", block).group(1))
    lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", block).group(1))
    print("reply_pack_kernel: %d VGPRs, %d bytes of scratch, %d bytes of LDS" % (vgprs, scratch, lds))
    assert scratch == 0, "reply_pack_kernel spills %d bytes per lane" % scratch
    assert lds == 0
    assert vgprs <= 12, "reply_pack_kernel needs %d VGPRs (12 when this guard was written)" % vgprs


def test_the_library_is_built_from_this_file():
    from pir_amd import build
    assert "reply_pack.hip" in build.SOURCES and "reply_pack.h" in build.HEADERS and "reply_pack.h" in build.CLIENT_HEADERS
