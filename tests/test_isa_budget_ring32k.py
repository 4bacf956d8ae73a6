"""Build-quality guard for the N = 32768 kernels (ntt_ring32k.hip; no GPU needed: hipcc cross-compiles gfx950 here).

Every kernel of the translation unit must run without scratch (a spill would put per-thread memory traffic into the
transforms, whose two passes are bound by HBM already) and within 128 VGPRs: at 128-thread (pass A) and 256-thread
(pass B, elementwise) workgroups that leaves room for four waves per SIMD, the latency hiding a transform that reads
and writes the whole polynomial through HBM twice depends on.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "pir_amd", "csrc", "ntt_ring32k.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# the kernels the file must define, with the workgroup size they are launched with
KERNELS = {
    "ntt32k_fwd_cols_kernel": 128, "ntt32k_inv_cols_kernel": 128,
    "ntt32k_fwd_rows_kernel": 256, "ntt32k_inv_rows_kernel": 256,
    "galois_digits_kernel": 256, "ks_mac_kernel": 256, "db_lift_kernel": 256, "upper_lift_kernel": 256,
    "upper_mac_int_kernel": 256,
}


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    assert os.path.exists(SRC), "the N = 32768 translation unit is missing"
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa32k") / "ntt_ring32k.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only", "-S", SRC,
                    "-o", str(out)], check=True, capture_output=True, timeout=600)
    return out.read_text()


def _descriptors(text):
    """kernel symbol -> (next_free_vgpr, private_segment_fixed_size, max flat workgroup size)"""
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        body = m.group(2)
        out[m.group(1)] = (int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)),
                           int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)))
    return out


def _flat_wg(text, sym):
    """.max_flat_workgroup_size of the kernel's metadata entry (the line right before its .name)"""
    m = re.search(r"\.max_flat_workgroup_size:\s+(\d+)\n\s+\.name:\s+" + re.escape(sym) + r"\n", text)
    return int(m.group(1)) if m else None


def test_every_kernel_is_spill_free_within_128_vgprs(isa):
    desc = _descriptors(isa)
    for name, wg in KERNELS.items():
        syms = [s for s in desc if name in s]
        assert len(syms) == 1, (name, syms)
        vgpr, scratch = desc[syms[0]]
        assert scratch == 0, "%s uses %d bytes of scratch" % (name, scratch)
        # launch bounds: wg threads = wg / 64 waves over 4 SIMDs; 128 VGPRs keep four waves per SIMD
        assert vgpr <= 128, "%s: %d VGPRs" % (name, vgpr)
    assert len(desc) == len(KERNELS), sorted(desc)


def test_launch_bounds_match_the_launch_shapes(isa):
    for name, wg in KERNELS.items():
        sym = next(s for s in _descriptors(isa) if name in s)
        got = _flat_wg(isa, sym)
        assert got == wg, (name, got)
