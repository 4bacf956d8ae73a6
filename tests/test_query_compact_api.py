"""Compact queries -- the host-side contract, no GPU: the exports of both libraries, their
declared signatures, null-safety, the Python mirrors against a recording library, and what stays as it was: no create
flag and no option for the feature."""
import ctypes as C
import os

import numpy as np
import pytest

import pir_amd
from pir_amd import capi
from pir_amd.server import PIRServer, PirGpuError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u64p, u32 = capi.u64p, C.c_uint32

SERVER = {
    "pirgpu_query_compact_words": (C.c_uint64, [C.c_void_p, C.c_int]),
    "pirgpu_query_stage_compact": (C.c_int, [C.c_void_p, u64p, u32, C.c_int]),
    "pirgpu_query_stage_compact_async": (C.c_int, [C.c_void_p, u64p, u32, C.c_int]),
    "pirgpu_batch_stage_compact": (C.c_int, [C.c_void_p, u64p, u32, u32, C.c_int]),
    "pirgpu_batch_stage_compact_async": (C.c_int, [C.c_void_p, u64p, u32, u32, C.c_int]),
    "pirgpu_query_expand": (C.c_int, [C.c_void_p, u64p, u32, C.c_int, u64p]),
    "pirgpu_query_expand_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
}
CLIENT = {
    "pirclient_set_compact_queries": (C.c_int, [C.c_void_p, C.c_int]),
    "pirclient_query_compact_words": (C.c_uint64, [C.c_void_p, C.c_int]),
    "pirclient_create_query_compact": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, u64p, C.c_size_t, C.POINTER(u32)]),
    "pirclient_save_request_compact": (C.c_int, [C.c_void_p, u64p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p),
                                                  C.POINTER(C.c_size_t)]),
}


def test_exports_and_signatures():
    header = open(os.path.join(ROOT, "include", "pirgpu.h")).read()
    lib = capi.load()
    for name, sig in SERVER.items():
        assert name + "(" in header and hasattr(lib, name) and capi.SIGNATURES[name] == sig, name
    cheader = open(os.path.join(ROOT, "include", "pirclient.h")).read()
    clib = capi.load_client()
    for name, sig in CLIENT.items():
        assert name + "(" in cheader and hasattr(clib, name) and capi.CLIENT_SIGNATURES[name] == sig, name
    # the three query forms are described where a caller looks
    for text in (header, cheader):
        assert "seed" in text and "0x80" in text and "section 6.9" in text


def test_null_safety():
    lib, clib = capi.load(), capi.load_client()
    assert lib.pirgpu_query_compact_words(None, 0) == 0 and lib.pirgpu_query_compact_words(None, 1) == 0
    assert lib.pirgpu_query_stage_compact(None, None, 1, 0) == capi.INVALID_ARGUMENT
    assert lib.pirgpu_query_stage_compact_async(None, None, 1, 1) == capi.INVALID_ARGUMENT
    assert lib.pirgpu_batch_stage_compact(None, None, 1, 1, 0) == capi.INVALID_ARGUMENT
    assert lib.pirgpu_batch_stage_compact_async(None, None, 1, 1, 1) == capi.INVALID_ARGUMENT
    assert lib.pirgpu_query_expand(None, None, 1, 0, None) == capi.INVALID_ARGUMENT
    assert lib.pirgpu_query_expand_stats(None, None) == capi.INVALID_ARGUMENT
    assert clib.pirclient_set_compact_queries(None, 1) == capi.INVALID_ARGUMENT
    assert clib.pirclient_query_compact_words(None, 1) == 0
    assert clib.pirclient_create_query_compact(None, 0, 0, None, 0, None) == capi.INVALID_ARGUMENT
    assert clib.pirclient_save_request_compact(None, None, 0, 0, None, None) == capi.INVALID_ARGUMENT


def test_no_create_flag_and_no_option_for_it():
    header = open(os.path.join(ROOT, "include", "pirgpu.h")).read()
    options = open(os.path.join(ROOT, "pir_amd", "csrc", "options.h")).read()
    assert "PIRGPU_CREATE_COMPACT" not in header and "PIRGPU_CREATE_QUERY" not in header
    assert "QUERY_EXPAND" not in options and "query_expand" not in options
    # the switch is environment-only, through the one gate
    wire = open(os.path.join(ROOT, "pir_amd", "csrc", "wire.cpp")).read()
    assert 'pirgpu_env("PIRGPU_WIRE_QUERY_EXPAND")' in wire and 'getenv("PIRGPU_WIRE_QUERY_EXPAND")' not in wire
    for name in ("pirgpu_query_stage_compact_async", "pirgpu_batch_stage_compact_async"):
        assert "#pragma weak " + name in wire


class _RecordingLib:
    """Stands in for libpirgpu: records every call, succeeds."""

    def __init__(self, words):
        self.calls, self.words = [], words

    def pirgpu_query_compact_words(self, h, packed):
        return self.words[packed]

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


class _Db:
    handle, N, k = 0x1234, 64, 2

    def __init__(self, lib):
        self.lib = lib

    def _check(self, rc):
        if rc:
            raise PirGpuError(rc, "recorded")


def test_python_mirrors_pass_shapes_and_forms_through():
    lib = _RecordingLib({0: 2 * 64 + 8, 1: 55})
    srv = PIRServer(_Db(lib), None)
    assert srv.query_compact_words(False) == 136 and srv.query_compact_words(True) == 55
    srv.stage_query_compact(np.zeros((3, 136), dtype=np.uint64))
    srv.stage_query_compact(np.zeros((3, 55), dtype=np.uint64), packed=True)
    srv.stage_batch_compact(np.zeros((5, 3, 55), dtype=np.uint64), packed=True, tables=[0, 1, 0, 1, 0])
    out = srv.query_expand(np.zeros((4, 136), dtype=np.uint64))
    assert out.shape == (4, 2, 2, 64)
    assert srv.query_expand_stats() == {"expanded": 0, "rejected": 0}
    names = [(n, a[2:4] if n.startswith("pirgpu_query_stage") else a[2:5]) for n, a in lib.calls
             if "compact" in n or n == "pirgpu_query_expand"]
    assert names[:3] == [("pirgpu_query_stage_compact", (3, 0)), ("pirgpu_query_stage_compact", (3, 1)),
                         ("pirgpu_batch_stage_compact", (3, 5, 1))]
    assert len(names) == 4 and names[3][0] == "pirgpu_query_expand" and names[3][1][:2] == (4, 0)
    assert any(n == "pirgpu_batch_set_tables" for n, _ in lib.calls)
    assert srv._batch_count == 5
    # wrong shapes never reach C
    before = len(lib.calls)
    for bad, packed in ((np.zeros((3, 136), dtype=np.uint64), True), (np.zeros((3, 2, 2, 64), dtype=np.uint64), False)):
        with pytest.raises(PirGpuError):
            srv.stage_query_compact(bad, packed=packed)
    with pytest.raises(PirGpuError):
        srv.stage_batch_compact(np.zeros((2, 3, 55), dtype=np.uint64), packed=True, tables=[0])
    assert len(lib.calls) == before
