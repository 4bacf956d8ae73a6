"""Build-quality guard for the band kernel of the streamed database load (db_pack_band_kernel, scan_mfma.hip; no GPU
needed: hipcc cross-compiles gfx950 here).

The kernel holds the L x 16 digit bytes of one (slot, row) in registers between its 16 loads and its L stores.  Indexed
dynamically that array would live in scratch: every instantiation must report a private segment of 0 bytes, and stay
within 128 VGPRs (256-thread workgroups, four waves per SIMD: the loads of one tile row are all a wave has in flight).
Only the code object's metadata is read.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pir_amd", "csrc", "scan_mfma.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# every (digits, top digit as a nibble) the scan has (mfma_geometry: the nibble form is not built for L = 7)
VARIANTS = [(5, True), (5, False), (6, True), (6, False), (7, False)]


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_db_stream") / "scan.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only", "-S", SRC,
                    "-o", str(out)], check=True, capture_output=True, timeout=600)
    return out.read_text()


def _descriptors(text):
    """kernel symbol -> (next_free_vgpr, private_segment_fixed_size)"""
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        body = m.group(2)
        out[m.group(1)] = (int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)),
                           int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)))
    return out


def test_every_instantiation_exists_exactly_once(isa):
    syms = sorted(s for s in _descriptors(isa) if "db_pack_band_kernel" in s)
    want = sorted("_ZN6pirgpu19db_pack_band_kernelILi%dELb%dEEE" % (L, 1 if t else 0) for L, t in VARIANTS)
    assert [s.split("EEE")[0] + "EEE" for s in syms] == want, syms


@pytest.mark.parametrize("L,top4", VARIANTS)
def test_band_kernel_is_scratch_free_within_128_vgprs(isa, L, top4):
    name = "_ZN6pirgpu19db_pack_band_kernelILi%dELb%dEEE" % (L, 1 if top4 else 0)
    hits = [v for s, v in _descriptors(isa).items() if s.startswith(name)]
    assert len(hits) == 1, (name, hits)
    vgprs, scratch = hits[0]
    assert scratch == 0, "<%d, %s> uses %d bytes of scratch" % (L, top4, scratch)
    assert vgprs <= 128, "<%d, %s>: %d VGPRs" % (L, top4, vgprs)
