"""Tables (pirgpu_params.tables) -- the host-side contract, no GPU: the parameters and their
mirrors, the struct layout against the compiled header, the new exports, and the order / runs the batch pipeline forms
for a batch that names tables (pirgpu_plan_table_runs: pure host code)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from pir_amd import capi
from pir_amd import parameters as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096


def test_create_pir_parameters_describes_one_table():
    enc = P.generate_encryption_params(N, 24)
    one = P.create_pir_parameters(3000, 288, 2, enc)
    for T in (0, 1, 3, 64):
        pp = P.create_pir_parameters(3000, 288, 2, enc, tables=T)
        assert pp.tables == T and capi.make_params(pp).tables == T
        # num_items, num_pt, dimensions and the item size are those of ONE table, whatever T is
        assert (pp.num_items, pp.num_pt, pp.dimensions, pp.bytes_per_item, pp.items_per_plaintext) == \
               (one.num_items, one.num_pt, one.dimensions, one.bytes_per_item, one.items_per_plaintext)
    assert one.tables == 0 and capi.make_params(one).tables == 0
    assert P.create_pir_parameters(3000, 288, 2, enc, result_primes=1, tables=3).result_primes == 1
    with pytest.raises(ValueError):
        P.create_pir_parameters(3000, 288, 2, enc, tables=-1)
    with pytest.raises(ValueError):                                   # a table and a plane both claim the outermost rows
        P.create_pir_parameters(100, 20000, 2, enc, max_plaintexts_per_item=4, tables=2)


def test_struct_layout_matches_the_header():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.c")
        open(src, "w").write('#include <stdio.h>\n#include "pirgpu.h"\nint main(){printf("%zu %zu %zu", '
                             'sizeof(pirgpu_params), __builtin_offsetof(pirgpu_params, tables), '
                             '__builtin_offsetof(pirgpu_params, result_primes));return 0;}')
        exe = os.path.join(d, "s")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        size, off_t, off_r = map(int, subprocess.run([exe], capture_output=True, text=True).stdout.split())
    assert C.sizeof(capi.ParamsLayout) == size == C.sizeof(capi.Params)
    assert capi.ParamsLayout.tables.offset == off_t == off_r + 4
    assert capi.ParamsLayout._fields_[-1][0] == "tables"                 # the trailing field
    assert off_t + 4 <= size < off_t + 4 + 8                             # nothing but padding behind it
    for name, _ in capi.Params._fields_:                                 # every other member where the header has it
        assert getattr(capi.Params, name).offset == getattr(capi.ParamsLayout, name).offset
    # the struct the entry points are given carries `tables` in exactly those four bytes
    p = capi.Params()
    assert p.tables == 0 and C.string_at(C.addressof(p), size) == bytes(size)
    p.tables = 0x01020304
    assert C.string_at(C.addressof(p) + off_t, 4) == (0x01020304).to_bytes(4, "little") and p.tables == 0x01020304
    assert p.result_primes == 0
    full = capi.ParamsLayout.from_buffer_copy(p)
    assert full.tables == 0x01020304


def test_new_exports_are_declared_bound_and_null_safe():
    header = open(os.path.join(ROOT, "include", "pirgpu.h")).read()
    lib = capi.load()
    for name in ("pirgpu_tables", "pirgpu_table_zero_plaintexts", "pirgpu_query_use_table", "pirgpu_batch_set_tables",
                 "pirgpu_db_load_table_items", "pirgpu_process_request_table", "pirgpu_process_requests_tables",
                 "pirgpu_plan_table_runs"):
        assert name in header and hasattr(lib, name) and name in capi.SIGNATURES, name
    assert lib.pirgpu_tables(None) == 0 and lib.pirgpu_table_zero_plaintexts(None, 0) == 0
    assert lib.pirgpu_query_use_table(None, 0) == capi.INVALID_ARGUMENT
    assert lib.pirgpu_batch_set_tables(None, None, 0) == capi.INVALID_ARGUMENT
    assert lib.pirgpu_db_load_table_items(None, 0, None, 0, 0) == capi.INVALID_ARGUMENT
    assert lib.pirgpu_process_request_table(None, 0, None, 0, None, None) == capi.INVALID_ARGUMENT
    assert lib.pirgpu_process_requests_tables(None, 0, None, None, None, None, None, None) == capi.INVALID_ARGUMENT
    assert lib.pirgpu_plan_table_runs(None, 1, 8, None, None, None) == capi.INVALID_ARGUMENT
    facade = open(os.path.join(ROOT, "pir_amd", "csrc", "pir_facade.h")).read()
    for word in ("p.tables = params->tables", "load_table", "use_table", "pirgpu_process_requests_tables",
                 "pirgpu_process_request_table"):
        assert word in facade, word


def plan(tables, group=8):
    lib = capi.load()
    n = len(tables)
    t = (C.c_uint32 * max(n, 1))(*tables)
    order = (C.c_uint32 * max(n, 1))()
    runs = (C.c_uint32 * (n + 1))()
    n_runs = C.c_uint32(0)
    assert lib.pirgpu_plan_table_runs(t, n, group, order, runs, C.byref(n_runs)) == 0
    return list(order[:n]), list(runs[:n_runs.value + 1])


ISSUE_BATCH = [2, 0, 1, 1, 0, 2, 2, 2, 2, 2, 2, 2, 2, 2, 0, 1, 2, 0, 1]


@pytest.mark.parametrize("tables,group", [(ISSUE_BATCH, 8), (list(range(12)) + [0, 1, 2, 3], 8), ([5], 8), ([], 8),
                                          ([3, 3, 3, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0], 4),
                                          (list(np.random.default_rng(7).integers(0, 9, size=200)), 8),
                                          (list(np.random.default_rng(8).integers(0, 64, size=64)), 8)])
def test_order_is_a_stable_sort_and_runs_stay_inside_groups(tables, group):
    tables = [int(t) for t in tables]
    order, runs = plan(tables, group)
    n = len(tables)
    # a permutation, inverted exactly: scattering position i's reply to order[i] fills every submission index once
    assert sorted(order) == list(range(n))
    inverse = [0] * n
    for pos, q in enumerate(order):
        inverse[q] = pos
    assert [order[inverse[q]] for q in range(n)] == list(range(n))
    # stable sort by table
    assert order == sorted(range(n), key=lambda q: tables[q])
    served = [tables[q] for q in order]
    assert served == sorted(tables)
    # runs: consecutive, cover everything, one table each, never across a group boundary, and maximal
    assert runs[0] == 0 and runs[-1] == n and all(a < b for a, b in zip(runs[:-1], runs[1:])) or n == 0
    for a, b in zip(runs[:-1], runs[1:]):
        assert len(set(served[a:b])) == 1, (a, b)
        assert a // group == (b - 1) // group, (a, b)
    for b in runs[1:-1]:
        assert b % group == 0 or served[b] != served[b - 1], b


def test_issue_batch_groups_and_runs():
    order, runs = plan(ISSUE_BATCH, 8)
    served = [ISSUE_BATCH[q] for q in order]
    assert served == [0] * 4 + [1] * 4 + [2] * 11
    assert runs == [0, 4, 8, 16, 19]                  # group 0: two runs, groups 1 and 2: one run each
    order, runs = plan(list(range(12)) + [0, 1, 2, 3], 8)
    assert runs == [0, 2, 4, 6, 8, 9, 10, 11, 12, 13, 14, 15, 16]      # the second group has 8 runs of one query


@pytest.mark.parametrize("n", [1, 7, 8, 19, 64])
def test_a_batch_of_one_table_keeps_todays_grouping(n):
    for t in (0, 4):
        order, runs = plan([t] * n, 8)
        assert order == list(range(n))                                   # served in submission order
        assert runs == list(range(0, n, 8)) + [n]                        # one run per group of 8: the groups of today
