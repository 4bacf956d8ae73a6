"""CPU checks of the streamed-database surface (pirgpu_create_ex with PIRGPU_CREATE_STREAMED_DB, pirgpu_db_memory,
pirgpu_db_read_operand): header, library and ctypes table agree, the argument errors that need no GPU are found before a
device is looked for, the Python mirrors pass the flag through, and the C++ facade compiles and links with it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
from gpu_helpers import to_product_params
from pir_amd import capi
from pir_amd.server import PIRDatabase

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "pirgpu_create_ex": "int pirgpu_create_ex(const pirgpu_params* params, uint32_t flags, pirgpu_ctx** out);",
    "pirgpu_db_memory": "int pirgpu_db_memory(const pirgpu_ctx* ctx, uint64_t out[4]);",
    "pirgpu_db_read_operand": "int pirgpu_db_read_operand(pirgpu_ctx* ctx, uint64_t offset, uint64_t n, uint8_t* out);",
}


def _params(d=2):
    return to_product_params(oracle.create_pir_parameters(300, 288, d, N=4096, plain_bits=24))


def _create_ex(cp, flags):
    lib = capi.load()
    h = C.c_void_p()
    rc = lib.pirgpu_create_ex(C.byref(cp), flags, C.byref(h))
    msg = lib.pirgpu_create_error().decode()
    if h:
        lib.pirgpu_destroy(h)
    return rc, msg


def test_header_library_and_signatures_agree():
    lib = capi.load()
    with open(os.path.join(ROOT, "include", "pirgpu.h")) as f:
        header = f.read()
    for name, decl in NEW.items():
        assert decl in header, name
        assert name in capi.SIGNATURES
        assert getattr(lib, name) is not None
    assert re.search(r"#define PIRGPU_CREATE_STREAMED_DB 1u\b", header)
    assert capi.CREATE_STREAMED_DB == 1
    assert capi.SIGNATURES["pirgpu_create_ex"][1][1] is C.c_uint32


def test_create_ex_without_flags_fails_or_succeeds_like_create():
    lib = capi.load()
    cp = capi.make_params(_params())
    h = C.c_void_p()
    rc = lib.pirgpu_create(C.byref(cp), C.byref(h))
    msg = lib.pirgpu_create_error().decode()
    if h:
        lib.pirgpu_destroy(h)
    for flags in (0, capi.CREATE_STREAMED_DB):
        rc_ex, msg_ex = _create_ex(cp, flags)
        assert rc_ex == rc, (flags, rc_ex, msg_ex)
        if rc:      # no GPU here: the same loud failure, there is no CPU fallback
            assert rc == capi.INTERNAL and "no HIP device" in msg and msg_ex == msg


@pytest.mark.parametrize("flags", [2, 3, 0x80000000, 0xFFFFFFFE])
def test_unknown_flag_bits_are_invalid_argument(flags):
    rc, msg = _create_ex(capi.make_params(_params()), flags)
    assert rc == capi.INVALID_ARGUMENT and "flags" in msg, (rc, msg)


def test_streamed_d1_is_invalid_argument_before_a_device_is_needed():
    cp = capi.make_params(_params(d=1))
    rc, msg = _create_ex(cp, capi.CREATE_STREAMED_DB)
    assert rc == capi.INVALID_ARGUMENT and "d >= 2" in msg, (rc, msg)


class _RecordingLib:
    """Stands in for libpirgpu: records every call, succeeds."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def test_python_mirrors_pass_the_flag_through(monkeypatch):
    lib = _RecordingLib()
    monkeypatch.setattr(capi, "load", lambda: lib)
    pp = _params()
    for kw, flag in [({}, 0), ({"streamed": False}, 0), ({"streamed": True}, 1)]:
        del lib.calls[:]
        db = PIRDatabase(pp, **kw)
        db._h = None        # nothing to destroy
        assert [(n, a[1]) for n, a in lib.calls] == [("pirgpu_create_ex", flag)]
    del lib.calls[:]
    db = PIRDatabase.Create(pp, streamed=True, slots=(0, 1024))
    db._h = None
    assert lib.calls[0][0] == "pirgpu_create_ex" and lib.calls[0][1][1] == 1


def test_memory_and_read_operand_wrappers():
    db = PIRDatabase.__new__(PIRDatabase)      # no device: only the marshalling runs

    class Lib(_RecordingLib):
        def pirgpu_db_memory(self, h, out):
            out[0], out[1], out[2], out[3] = 10, 20, 40, 5
            return 0

        def pirgpu_db_read_operand(self, h, offset, n, out):
            self.calls.append(("pirgpu_db_read_operand", (offset, n)))
            return 0

    db.lib, db._h = Lib(), None
    assert db.memory() == {"operand": 10, "staging": 20, "peak": 40, "band": 5}
    got = db.read_operand(16, 48)
    assert got.dtype == np.uint8 and got.shape == (48,)
    assert db.lib.calls == [("pirgpu_db_read_operand", (16, 48))]


FACADE_SRC = r"""
#include "pir_facade.h"

// never reached without arguments: the point is that the streamed overloads compile and link against libpirgpu
int main(int argc, char** argv) {
  if (argc < 2) return 0;
  auto params = std::make_shared<pir::PIRParameters>();
  auto db = pir::PIRDatabase::Create(params, 0, /*streamed=*/true);
  auto db2 = pir::PIRDatabase::Create(std::vector<std::string>{"a"}, params, 0, true);
  uint64_t mem[4];
  return db.ok() && db2.ok() ? pirgpu_db_memory(nullptr, mem) : 1;
}
"""


def test_facade_streamed_create_compiles_and_links(tmp_path):
    capi.load()
    src = tmp_path / "stream_facade.cpp"
    src.write_text(FACADE_SRC)
    exe = str(tmp_path / "stream_facade")
    lib_dir = os.path.join(ROOT, "pir_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "pir_amd", "csrc"), str(src), "-o",
                    exe, "-L" + lib_dir, "-lpirgpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([exe], capture_output=True).returncode == 0
