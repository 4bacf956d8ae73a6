"""CPU checks of the in-place database update surface (pirgpu_db_update_items / _plaintexts): the library exports the
symbols, the Python wrappers reject malformed arguments before they reach the C ABI, and the C++ facade's
PIRDatabase::update_items compiles and links against the library."""
import os
import subprocess

import numpy as np
import pytest

import oracle
from gpu_helpers import to_product_params
from pir_amd.server import PIRDatabase, PirGpuError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_update_symbols_are_exported_and_declared():
    import pir_amd.capi as capi
    lib = capi.load()
    for name in ("pirgpu_db_update_items", "pirgpu_db_update_plaintexts"):
        assert name in capi.SIGNATURES
        assert getattr(lib, name) is not None
    with open(os.path.join(ROOT, "include", "pirgpu.h")) as f:
        header = f.read()
    assert "int pirgpu_db_update_items(pirgpu_ctx* ctx, uint64_t n, const uint64_t* item_indices" in header
    assert "int pirgpu_db_update_plaintexts(pirgpu_ctx* ctx, uint64_t n, const uint64_t* pt_indices" in header


class _RecordingLib:
    """Stands in for libpirgpu: records every call, succeeds."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def _db():
    p = oracle.create_pir_parameters(300, 288, 2, N=4096, plain_bits=24)
    db = PIRDatabase.__new__(PIRDatabase)      # no device: only the argument checks run
    db.params = to_product_params(p)
    db.N, db.k = 4096, len(p.moduli) - 1
    db.lib = _RecordingLib()
    db._h = None
    return db


@pytest.mark.parametrize("indices,items", [
    ([0, 1], np.zeros((2, 287), dtype=np.uint8)),          # wrong width
    ([0, 1], np.zeros((3, 288), dtype=np.uint8)),          # more rows than indices
    ([0, 1], np.zeros((2, 288), dtype=np.int16)),          # not bytes
    ([0], [b"x" * 289]),                                   # wrong width, sequence of bytes
    ([0, 1], [b"x" * 288]),                                # fewer items than indices
    ([-1], [b"x" * 288]),                                  # negative index
    ([[0]], [b"x" * 288]),                                 # not 1-D
])
def test_update_items_rejects_bad_arguments_before_the_abi(indices, items):
    db = _db()
    with pytest.raises(PirGpuError) as e:
        db.update_items(indices, items)
    assert e.value.code == 3
    assert db.lib.calls == []


def test_update_items_passes_one_row_per_index():
    db = _db()
    db.update_items([4, 9], [b"a" * 288, b"b" * 288])
    db.update_items(np.array([1], dtype=np.int64), np.ones((1, 288), dtype=np.uint8))
    names = [c[0] for c in db.lib.calls]
    assert names == ["pirgpu_db_update_items"] * 2
    assert db.lib.calls[0][1][1] == 2 and db.lib.calls[0][1][4] == 288
    assert db.lib.calls[1][1][1] == 1


@pytest.mark.parametrize("indices,rows", [
    ([0, 1], [np.zeros(4096, dtype=np.uint64)]),           # fewer rows than indices
    ([0], [np.zeros(4097, dtype=np.uint64)]),              # longer than N
    ([0], [np.zeros((2, 8), dtype=np.uint64)]),            # not 1-D
    ([0], [np.array([-1, 2])]),                            # negative coefficient
    ([0], [np.array([0.5])]),                              # not integers
])
def test_update_plaintexts_rejects_bad_arguments_before_the_abi(indices, rows):
    db = _db()
    with pytest.raises(PirGpuError) as e:
        db.update_plaintexts(indices, rows)
    assert e.value.code == 3
    assert db.lib.calls == []


FACADE_SRC = r"""
#include "pir_facade.h"
#include <cstdio>

// never reached without arguments: the point is that update_items compiles and links against libpirgpu
int main(int argc, char** argv) {
  if (argc < 2) return 0;
  auto params = std::make_shared<pir::PIRParameters>();
  auto db = pir::PIRDatabase::Create(params);
  if (!db.ok()) return 1;
  pir::Status s = (*db)->update_items(std::vector<uint64_t>{0, 1}, std::vector<std::string>{"a", "b"});
  std::printf("%d %s\n", static_cast<int>(s.code()), s.message().c_str());
  return 0;
}
"""


def test_facade_update_items_compiles_and_links(tmp_path):
    import pir_amd.capi as capi
    capi.load()
    src = tmp_path / "update_facade.cpp"
    src.write_text(FACADE_SRC)
    exe = str(tmp_path / "update_facade")
    lib_dir = os.path.join(ROOT, "pir_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "pir_amd", "csrc"), str(src), "-o",
                    exe, "-L" + lib_dir, "-lpirgpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([exe], capture_output=True).returncode == 0
