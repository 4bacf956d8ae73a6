"""What tables (pirgpu_params.tables) cost and save: 64 queries spread evenly over T = 64 tables of
2^14 items of 288 bytes each (N = 4096, 24-bit t; a table is a 21 x 20 matrix), 16 workers.

  (1) the T = 64 context with the multi-run launch (one database pass per batch group: the default), the same context
      shape with TABLES_ONE_LAUNCH = 0 (one launch per run of equal tables), and ONE context holding a single such table
      answering 64 queries -- the floor: the same expansion, one shared scan per group;
  (2) the same 2^20 items as ONE database (the benchmark's cfg 3 shape) answering 64 queries: the price of not revealing
      the table;
  (3) pirgpu_db_memory and the device memory the process holds (hipMemGetInfo through torch, when it is there) for one
      T = 64 context against one single-table context.

    python tools/tables_timing.py [--out profiles/tables.json] [--reps 7] [--tables 64] [--items 16384] [--queries 64]

Timing: host clock at the ABI around pirgpu_batch_stage (+ _set_tables) + _run + pirgpu_sync + _fetch into a buffer that
was allocated and touched beforehand.  The variants alternate inside one process on fresh contexts, `reps` times after one
untimed round; the JSON keeps every sample, the medians and the spread (max - min) of each variant, and the database-pass
launches per batch (option SCAN_LAUNCHES).  Replies of the two table variants are compared with each other and, per
query, with the single-table context given that table, once, before anything is timed."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# torch first (when it is there): its own HIP runtime must be the one the process loads
try:
    import torch  # noqa: F401
except ImportError:
    torch = None

import pir_amd  # noqa: E402
from pir_amd import capi  # noqa: E402
from pir_amd import parameters as P  # noqa: E402


def head_commit() -> str:
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=9", "HEAD"], capture_output=True,
                              text=True).stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def device_used_bytes():
    if torch is None:       # the library's own count is all there is
        return None
    try:
        free, total = torch.cuda.mem_get_info()
        return int(total - free)
    except RuntimeError:
        return None


def serve(pp, raw, keys, one_launch=None):
    db = pir_amd.PIRDatabase.Create(pp, raw)
    if one_launch is not None:
        db.set_option("tables_one_launch", one_launch)
    db.finalize(release_staging=True)
    srv = pir_amd.PIRServer.Create(db, pp)
    srv.set_galois_keys(keys)
    srv.set_concurrency(16)
    return db, srv


def reply_buffer(srv, count):
    return np.zeros((count, srv.db.reply_ct_count(), 2, srv.k, srv.N), dtype=np.uint64)   # zeros: every page touched


def batch_ms(srv, queries, out, tables=None):
    """(device ms, total ms, database-pass launches) of one batch; replies land in `out`."""
    got = C.c_uint64(0)
    srv.db.set_option("scan_launches", 0)
    t0 = time.perf_counter()
    srv.stage_batch(queries, tables=tables)
    srv.run_batch()
    srv.sync()
    t1 = time.perf_counter()
    srv._check(srv.lib.pirgpu_batch_fetch(srv.db.handle, out.ctypes.data_as(capi.u64p), out.shape[0] * out.shape[1],
                                          C.byref(got)))
    t2 = time.perf_counter()
    assert got.value == out.shape[0] * out.shape[1]
    return (t1 - t0) * 1e3, (t2 - t0) * 1e3, srv.db.get_option("scan_launches")


def summary(samples):
    tot = [s[1] for s in samples]
    dev = [s[0] for s in samples]
    return {"total_ms_median": statistics.median(tot), "total_ms_spread": max(tot) - min(tot), "total_ms_samples": tot,
            "device_ms_median": statistics.median(dev), "device_ms_spread": max(dev) - min(dev), "device_ms_samples": dev,
            "scan_launches_per_batch": samples[-1][2]}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tables.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tables", type=int, default=64)
    ap.add_argument("--items", type=int, default=1 << 14)
    ap.add_argument("--bytes", type=int, default=288)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--skip-whole", action="store_true", help="leave out (2), the one whole database")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("medians of at least 5 runs")
    T = a.tables
    enc = P.generate_encryption_params(4096, 24)
    one = P.create_pir_parameters(a.items, a.bytes, 2, enc)
    many = P.create_pir_parameters(a.items, a.bytes, 2, enc, tables=T)
    whole = P.create_pir_parameters(a.items * T, a.bytes, 2, enc)
    rng = np.random.default_rng(2026)
    raw = rng.integers(0, 256, size=(T * a.items, a.bytes), dtype=np.uint8)
    client = pir_amd.PIRClient.Create(one, seed=b"tables-timing")
    keys = client.galois_keys()
    idx = rng.integers(0, a.items, size=a.queries)
    queries = np.stack([client.create_query_for(int(i)) for i in idx])
    tables = [int(t) for t in rng.permutation(np.arange(a.queries) % T)]       # spread evenly, submitted unsorted

    used0 = device_used_bytes()
    db_one, srv_one = serve(one, raw[:a.items], keys)
    out_one = reply_buffer(srv_one, a.queries)
    batch_ms(srv_one, queries, out_one)
    used_one = device_used_bytes()
    mem_one = db_one.memory()
    db_m, srv_m = serve(many, raw, keys, one_launch=1)
    out_m = reply_buffer(srv_m, a.queries)
    batch_ms(srv_m, queries, out_m, tables)
    used_many = device_used_bytes()
    mem_many = db_m.memory()
    db_r, srv_r = serve(many, raw, keys, one_launch=0)
    out_r = reply_buffer(srv_r, a.queries)
    batch_ms(srv_r, queries, out_r, tables)
    assert np.array_equal(out_m, out_r), "multi-run launch and per-run launches disagree"
    # every query against the single-table context holding ITS table (a sample of the tables: one reload each)
    for t in sorted(set(tables))[:4]:
        db_one.close()
        db_one, srv_one = serve(one, raw[t * a.items:(t + 1) * a.items], keys)
        batch_ms(srv_one, queries, out_one)
        for q in range(a.queries):
            if tables[q] == t:
                assert np.array_equal(out_m[q], out_one[q]), "query %d on table %d differs from that table alone" % (q, t)
    variants = {"tables_one_launch": (srv_m, out_m, tables), "tables_launch_per_run": (srv_r, out_r, tables),
                "single_table_floor": (srv_one, out_one, None)}
    db_w = None
    if not a.skip_whole:
        wclient = pir_amd.PIRClient.Create(whole, seed=b"tables-timing")
        wq = np.stack([wclient.create_query_for(int(tables[q]) * a.items + int(idx[q])) for q in range(a.queries)])
        db_w, srv_w = serve(whole, raw, wclient.galois_keys())
        out_w = reply_buffer(srv_w, a.queries)
        batch_ms(srv_w, wq, out_w)
        variants["whole_database"] = (srv_w, out_w, None)
    samples = {name: [] for name in variants}
    for _ in range(a.reps):
        for name, (srv, out, tb) in variants.items():
            samples[name].append(batch_ms(srv, wq if name == "whole_database" else queries, out, tb))
    res = {"what": "batch of %d queries spread evenly over %d tables of %d items of %d bytes: one context with tables "
                   "(multi-run launch / one launch per run), one context of a single table (the floor), and the same "
                   "items as one database; host clock around batch stage + run + sync + fetch, alternating in one "
                   "process" % (a.queries, T, a.items, a.bytes),
           "commit": os.environ.get("PIRGPU_PROFILED_COMMIT") or head_commit(), "N": 4096, "plain_bits": 24,
           "tables": T, "items_per_table": a.items, "bytes_per_item": a.bytes, "queries": a.queries, "reps": a.reps,
           "table_dimensions": list(one.dimensions), "whole_dimensions": list(whole.dimensions),
           "scan_tables": srv_m.scan_info(), "scan_bytes_tables": srv_m.scan_bytes(), "scan_bytes_single": srv_one.scan_bytes(),
           "db_memory_tables": mem_many, "db_memory_single": mem_one,
           "device_bytes_single_context": None if used0 is None else used_one - used0,
           "device_bytes_tables_context": None if used0 is None else used_many - used_one,
           "variants": {name: summary(s) for name, s in samples.items()}}
    if db_w is not None:
        res["scan_whole"] = variants["whole_database"][0].scan_info()
        res["scan_bytes_whole"] = variants["whole_database"][0].scan_bytes()
    for name, v in res["variants"].items():
        print("%-24s median %8.3f ms (spread %.3f), upload + kernels %8.3f ms, %d database-pass launches per batch"
              % (name, v["total_ms_median"], v["total_ms_spread"], v["device_ms_median"], v["scan_launches_per_batch"]))
    print("database bytes: %d tables %s, single table %s" % (T, mem_many, mem_one))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    for db in (db_one, db_m, db_r, db_w):
        if db is not None:
            db.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
