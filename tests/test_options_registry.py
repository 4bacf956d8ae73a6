"""The option registry (pir_amd/csrc/options.h) without a GPU: its host logic -- the list of options, name lookup, the
PIRGPU_ALLOW_ENV gate, precedence, kinds, counters -- under AddressSanitizer + UBSan (tests/cpp/options_test.cpp, a
stand-alone program), and DESIGN.md's option table against the registry's rows."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIONS_H = os.path.join(ROOT, "pir_amd", "csrc", "options.h")


def test_option_registry_under_sanitizers(tmp_path):
    exe = str(tmp_path / "options_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall",
                    "-Wextra", os.path.join(ROOT, "tests", "cpp", "options_test.cpp"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("PIRGPU_")}    # the program sets what it tests
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "options_test OK" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]


def registry_rows():
    """{name: kind} as options.h declares them: X(NAME, Kind, "description ...")."""
    with open(OPTIONS_H) as f:
        rows = re.findall(r"^\s*X\(([A-Z0-9_]+), (Early|Live|Counter),", f.read(), re.M)
    return {name: kind.lower() for name, kind in rows}


def design_table_rows():
    """{name: kind} of DESIGN.md's option table: | `NAME` | kind | default | what it does |."""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        rows = re.findall(r"^\| `([A-Z0-9_]+)` \| (early|live|counter) \|[^|]+\|[^|]+\|$", f.read(), re.M)
    assert len(rows) == len(set(name for name, _ in rows)), "a name appears twice in DESIGN.md's option table"
    return dict(rows)


def test_design_table_lists_the_registry():
    reg, doc = registry_rows(), design_table_rows()
    assert len(reg) == 42
    assert sorted(set(reg) - set(doc)) == [], "options missing from DESIGN.md's table"
    assert sorted(set(doc) - set(reg)) == [], "DESIGN.md's table names options the registry lacks"
    assert {n: k for n, k in doc.items() if reg[n] != k} == {}, "kinds differ"
