"""The batch pipeline's planning logic (pir_amd/csrc/batch_plan.h) without a GPU: how a call is cut into groups, pairs
and lanes, the order of a batch that names tables and what its groups report as complete -- under AddressSanitizer +
UBSan (tests/cpp/batch_plan_test.cpp, a stand-alone program)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "batch_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall",
                    "-Wextra", os.path.join(ROOT, "tests", "cpp", "batch_plan_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "batch_plan_test OK" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]


def test_the_library_is_built_from_the_header():
    """ctx.hip includes the header (no second copy of the plan in the library) and the build's staleness check knows it."""
    from pir_amd import build
    assert "batch_plan.h" in build.HEADERS
    with open(os.path.join(ROOT, "pir_amd", "csrc", "ctx.hip")) as f:
        src = f.read()
    assert '#include "batch_plan.h"' in src and "TablePlan plan_table_runs(" not in src
