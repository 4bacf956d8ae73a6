"""What wide items (pirgpu_params.plaintexts_per_item) save: items of 30 000 bytes -- three plaintexts at N = 4096, 24-bit
t -- in a database of 162 x 162 items (the matrix shape of the benchmark's cfg 3), a batch of 64 queries.

  (a) ONE wide context (planes = 3): every query is expanded once and answered on all three planes;
  (b) the way without the feature: THREE contexts of one-plaintext items (chunk j of every item each), every one
      answering the same 64 queries -- three expansions per query.  A planes = 1 context behaves exactly as before the
      feature, so (b) is the earlier cost measured in the same run.  Its time is the SUM over the three contexts.

    python tools/wide_items_timing.py [--out profiles/wide_items.json] [--reps 7] [--items 26244] [--queries 64]

Timing: host clock at the ABI around pirgpu_batch_stage + _run + pirgpu_sync + _fetch (the fetch downloads every reply
into a buffer that was allocated and touched beforehand: a fresh 200 MB numpy array per call costs more in page faults
than the GPU work and varies from run to run), 16 workers, staging released on every context.  "device" is the part up
to the end of pirgpu_sync (upload + all kernels), "total" includes the download.  (a) and (b) alternate inside one
process, `reps` times after one untimed round; the JSON keeps every sample, the medians and the spread (max - min) of
each side.  The replies of (a) are compared with those of (b) once, before anything is timed.  The phase times of a
single query (pirgpu_last_timings, HIP events) on the wide context and on one of the others are recorded as well."""
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

import pir_amd  # noqa: E402
from pir_amd import capi  # noqa: E402
from pir_amd import parameters as P  # noqa: E402


def head_commit() -> str:
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=9", "HEAD"], capture_output=True,
                              text=True).stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def serve(pp, raw, keys):
    db = pir_amd.PIRDatabase.Create(pp, raw)
    db.finalize(release_staging=True)
    srv = pir_amd.PIRServer.Create(db, pp)
    srv.set_galois_keys(keys)
    srv.set_concurrency(16)
    return db, srv


def reply_buffer(srv, count):
    return np.zeros((count, srv.db.reply_ct_count(), 2, srv.k, srv.N), dtype=np.uint64)   # zeros: every page touched


def batch_ms(srv, queries, out):
    """(device ms, total ms) of one batch; replies land in `out`."""
    got = C.c_uint64(0)
    t0 = time.perf_counter()
    srv.stage_batch(queries)
    srv.run_batch()
    srv.sync()
    t1 = time.perf_counter()
    srv._check(srv.lib.pirgpu_batch_fetch(srv.db.handle, out.ctypes.data_as(capi.u64p), out.shape[0] * out.shape[1],
                                          C.byref(got)))
    t2 = time.perf_counter()
    assert got.value == out.shape[0] * out.shape[1]
    return (t1 - t0) * 1e3, (t2 - t0) * 1e3


def single_query_phases(srv, query, runs=20):
    srv.set_profiling(True)
    for _ in range(runs):
        srv.stage_query(query)
        srv.run_staged()
        srv.fetch_reply()
    t = srv.last_timings()
    srv.set_profiling(False)
    return t


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_items.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--items", type=int, default=162 * 162)
    ap.add_argument("--bytes", type=int, default=30000)
    ap.add_argument("--queries", type=int, default=64)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("medians of at least 5 runs")
    enc = P.generate_encryption_params(4096, 24)
    wide = P.create_pir_parameters(a.items, a.bytes, 2, enc, max_plaintexts_per_item=16)
    planes, B = wide.planes, wide.max_bytes_per_plaintext
    rng = np.random.default_rng(2026)
    raw = rng.integers(0, 256, size=(a.items, a.bytes), dtype=np.uint8)
    # the same data the way a user without wide items has to store it: one database per chunk
    chunks = [np.ascontiguousarray(raw[:, j * B:min((j + 1) * B, a.bytes)]) for j in range(planes)]
    narrow = [P.create_pir_parameters(a.items, c.shape[1], 2, enc) for c in chunks]
    for pp in narrow:
        assert pp.items_per_plaintext == 1 and pp.dimensions == wide.dimensions, (pp.items_per_plaintext, pp.dimensions)
    client = pir_amd.PIRClient.Create(wide, seed=b"wide-items-timing")
    keys = client.galois_keys()
    idx = rng.choice(a.items, size=a.queries, replace=False)
    queries = np.stack([client.create_query_for(int(i)) for i in idx])

    db_a, srv_a = serve(wide, raw, keys)
    ctx_b = [serve(pp, c, keys) for pp, c in zip(narrow, chunks)]
    # correctness first (and the untimed first round: module loading, workspace, lanes): plane j of (a) == context j of (b)
    out_a = reply_buffer(srv_a, a.queries)
    out_b = [reply_buffer(srv, a.queries) for _, srv in ctx_b]
    batch_ms(srv_a, queries, out_a)
    R = out_a.shape[1] // planes
    for j, (_, srv) in enumerate(ctx_b):
        batch_ms(srv, queries, out_b[j])
        assert np.array_equal(out_a[:, j * R:(j + 1) * R], out_b[j]), "plane %d differs from its own context" % j
    a_ms, b_ms, a_dev, b_dev, b_parts = [], [], [], [], []
    for _ in range(a.reps):
        dev, tot = batch_ms(srv_a, queries, out_a)
        a_dev.append(dev)
        a_ms.append(tot)
        parts = [batch_ms(srv, queries, o) for (_, srv), o in zip(ctx_b, out_b)]
        b_parts.append([p[1] for p in parts])
        b_dev.append(sum(p[0] for p in parts))
        b_ms.append(sum(p[1] for p in parts))
    single_a = single_query_phases(srv_a, queries[0])
    single_b = single_query_phases(ctx_b[0][1], queries[0])
    res = {"what": "batch of %d queries on items of %d bytes (%d plaintexts each): (a) one wide context against (b) %d "
                   "contexts of one-plaintext items answering the same queries, summed; host clock around "
                   "batch stage + run + fetch, alternating in one process" % (a.queries, a.bytes, planes, planes),
           "commit": os.environ.get("PIRGPU_PROFILED_COMMIT") or head_commit(),
           "N": 4096, "plain_bits": 24, "num_items": a.items, "bytes_per_item": a.bytes, "planes": planes,
           "bytes_per_plaintext": B, "dimensions": list(wide.dimensions), "queries": a.queries, "reps": a.reps,
           "reply_cts_per_query": int(out_a.shape[1]), "scan_a": srv_a.scan_info(), "scan_b": ctx_b[0][1].scan_info(),
           "a_wide_ms_median": statistics.median(a_ms), "b_separate_ms_median": statistics.median(b_ms),
           "a_over_b": statistics.median(a_ms) / statistics.median(b_ms),
           "a_spread_ms": max(a_ms) - min(a_ms), "b_spread_ms": max(b_ms) - min(b_ms),
           "a_wide_device_ms_median": statistics.median(a_dev), "b_separate_device_ms_median": statistics.median(b_dev),
           "a_wide_device_ms_samples": a_dev, "b_separate_device_ms_samples": b_dev,
           "single_query_phases_ms_a_wide": single_a, "single_query_phases_ms_b_one_context": single_b,
           "a_wide_ms_samples": a_ms, "b_separate_ms_samples": b_ms, "b_per_context_ms_samples": b_parts}
    print("(a) wide, planes = %d : median %8.3f ms  (min %.3f, max %.3f)" % (planes, res["a_wide_ms_median"], min(a_ms), max(a_ms)))
    print("(b) %d contexts, summed: median %8.3f ms  (min %.3f, max %.3f)" % (planes, res["b_separate_ms_median"], min(b_ms), max(b_ms)))
    print("(a) / (b) = %.3f   (upload + kernels alone: %.3f against %.3f ms)" %
          (res["a_over_b"], res["a_wide_device_ms_median"], res["b_separate_device_ms_median"]))
    print("single query: wide %.3f ms, one of the %d contexts %.3f ms" % (single_a["total_ms"], planes, single_b["total_ms"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    db_a.close()
    for db, _ in ctx_b:
        db.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
