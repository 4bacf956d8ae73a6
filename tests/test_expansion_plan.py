"""The oblivious expansion's per-level plan (pir_amd/csrc/expansion_plan.h) without a GPU: the invariants that make
expand_core's internal errors unreachable over the whole domain, and walks pinned by hand -- under AddressSanitizer +
UBSan (tests/cpp/expansion_plan_test.cpp, a stand-alone program; its head states how the domain is cut)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "expansion_plan_test.cpp")


def test_expansion_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "expansion_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall",
                    "-Wextra", SOURCE, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)      # about 35 s; 2.3 * 10^7 walks
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "expansion_plan_test OK" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]


def test_the_library_is_built_from_the_header():
    """ctx.hip plans with the header (no second copy of the rules in the library), the kernels take their wide-level
    rule from it, and the build's staleness check knows it."""
    from pir_amd import build
    assert "expansion_plan.h" in build.HEADERS
    csrc = os.path.join(ROOT, "pir_amd", "csrc")
    with open(os.path.join(csrc, "ctx.hip")) as f:
        src = f.read()
    assert '#include "expansion_plan.h"' in src and "plan_expansion(" in src and "expansion_uses_head(" in src
    assert "level_fused" not in src and "next_reads40" not in src and "fuse_from" not in src
    with open(os.path.join(csrc, "kernels.h")) as f:
        assert "ks_digit_takes_c0(uint32_t" not in f.read()


def test_the_hook_is_declared_and_bound():
    from pir_amd import capi
    assert "pirgpu_expansion_forms" in capi.SIGNATURES
    with open(os.path.join(ROOT, "include", "pirgpu.h")) as f:
        assert "int pirgpu_expansion_forms(pirgpu_ctx* ctx, uint32_t B, uint32_t n, int head_split" in f.read()
