"""The host side of compact queries without a GPU: rpk::check_poly and the query codec's splitting
loader under AddressSanitizer + UBSan (tests/cpp/query_compact_test.cpp, a stand-alone program that links the host codec
only) -- compact objects at odd alignments, objects truncated inside the array, the seed and the header, the packed
byte on a full-size array, a c0 coefficient equal to its modulus in the first and the last position."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_query_compact_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "query_compact_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall",
                    "-Wextra", os.path.join(ROOT, "tests", "cpp", "query_compact_test.cpp"),
                    os.path.join(ROOT, "pir_amd", "csrc", "wire_codec.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "query_compact_test OK" in r.stdout
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
