"""What modulus-switched results (pirgpu_params.result_primes) cost and save, measured.

Shapes: the benchmark's cfg 3 (N = 4096, 2 data primes, 2^20 items of 288 bytes, d = 2) with result_primes r = 0 / 1 and,
with --cfg4, its cfg 4 (N = 8192, 3 data primes, 2^22 items of 1 KB, d = 2) with r = 0 / 1 / 2 -- skipped with a note if
it does not load.  The variants of one shape live in ONE process on fresh contexts of the same database and alternate,
`reps` times after one untimed round; the JSON keeps every sample, the medians and the spread (max - min).

  * single query: the phases of pirgpu_last_timings (HIP events: expansion, scan, upper level, final) over 10 runs per
    sample;
  * a batch of 64 queries at the ABI: host clock around pirgpu_batch_stage + _run + pirgpu_sync ("device") and + the
    download of every reply into a buffer touched beforehand ("total");
  * reply bytes per query (pirgpu_reply_ct_count x pirgpu_reply_ct_words x 8);
  * libpirclient's ProcessResponse on one wire-level response (host clock);
  * the switch kernel's own time does not show at the ABI: a second, short pass of this tool under the profiler,
        rocprofv3 --kernel-trace --stats -d DIR -- python tools/modswitch_timing.py --profile-pass
    runs 20 single queries on cfg 3 with r = 1, and --kernel-stats DIR/.../*_kernel_stats.csv folds the rows of
    mod_switch_kernel into the JSON next to the bytes one query's switches move (reads at k primes, writes at r) and
    the rate that is.  Nothing here is gated.

    python tools/modswitch_timing.py [--out profiles/modswitch.json] [--reps 7] [--cfg4] [--kernel-stats CSV]

At 24-bit t the 162 x 162 shape of cfg 3 leaves a single 36-bit prime no noise budget: the timings
do not depend on what the ciphertexts decrypt to, the item check of ProcessResponse is therefore reported, not asserted."""
from __future__ import annotations

import argparse
import csv
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


def shape(name):
    if name == "cfg3":
        return P.generate_encryption_params(4096, 24), 20, 288
    m = pir_amd.BFV_DEFAULT[8192]
    return P.generate_encryption_params(8192, 24, coeff_modulus=m[:3] + [m[4]]), 22, 1024


def med(v):
    return {"median": statistics.median(v), "spread": max(v) - min(v), "samples": list(v)}


class Variant:
    def __init__(self, enc, log_items, item_bytes, raw, r, n_queries, rng):
        self.r = r
        self.pp = P.create_pir_parameters(1 << log_items, item_bytes, 2, enc, result_primes=r)
        self.db = pir_amd.PIRDatabase.Create(self.pp, raw)
        self.db.finalize(release_staging=True)
        self.srv = pir_amd.PIRServer.Create(self.db, self.pp)
        self.client = pir_amd.PIRClient.Create(self.pp, seed=b"modswitch-timing")     # (the request does not depend on r)
        self.srv.set_galois_keys(self.client.galois_keys())
        self.srv.set_concurrency(16)
        self.idx = [int(i) for i in rng.choice(1 << log_items, size=n_queries, replace=False)]
        self.queries = np.stack([self.client.create_query_for(i) for i in self.idx])
        self.out = np.zeros((n_queries, self.db.reply_ct_count(), 2, self.srv.reply_k, self.srv.N), dtype=np.uint64)
        self.request = self.client.CreateRequest(self.idx[:1])
        self.samples = {"phases": [], "batch_device_ms": [], "batch_total_ms": [], "client_ms": []}
        self.item_ok = None

    def single(self, runs=10):
        self.srv.set_profiling(True)
        for _ in range(runs):
            self.srv.stage_query(self.queries[0])
            self.srv.run_staged()
            self.srv.fetch_reply()
        t = self.srv.last_timings()
        self.srv.set_profiling(False)
        return t

    def batch(self):
        got = C.c_uint64(0)
        t0 = time.perf_counter()
        self.srv.stage_batch(self.queries)
        self.srv.run_batch()
        self.srv.sync()
        t1 = time.perf_counter()
        self.srv._check(self.srv.lib.pirgpu_batch_fetch(self.db.handle, self.out.ctypes.data_as(capi.u64p),
                                                        self.out.shape[0] * self.out.shape[1], C.byref(got)))
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t0) * 1e3

    def client_pass(self, raw):
        response = self.srv.ProcessRequest(self.request)
        t0 = time.perf_counter()
        try:
            items = self.client.ProcessResponse(self.idx[:1], response)
            self.item_ok = items == [raw[self.idx[0]].tobytes()]
        except pir_amd.server.PirGpuError:
            self.item_ok = False
        return (time.perf_counter() - t0) * 1e3, len(response)

    def round(self, raw, record=True):
        ph = self.single()
        dev, tot = self.batch()
        cl, self.response_bytes = self.client_pass(raw)
        if record:
            self.samples["phases"].append(ph)
            self.samples["batch_device_ms"].append(dev)
            self.samples["batch_total_ms"].append(tot)
            self.samples["client_ms"].append(cl)

    def switch_bytes(self):
        """HBM bytes one query's switch launches move: the scan's row sums read at k primes and written at r in place,
        the reply read at k and written compact."""
        N, k, r = self.srv.N, self.srv.k, self.r
        rows, reply = self.pp.dimensions[0], self.db.reply_ct_count()
        return (rows + reply) * 2 * N * 8 * (k + r) if r else 0

    def report(self):
        ph = self.samples["phases"]
        res = {"result_primes": self.r, "expansion_ratio": self.db.expansion_ratio(),
               "reply_cts_per_query": self.db.reply_ct_count(), "reply_bytes_per_query": self.db.reply_ct_count() *
               self.db.reply_ct_words() * 8, "response_bytes_one_query": self.response_bytes,
               "single_query_ms": {p: med([s[p] for s in ph]) for p in ("expand_ms", "scan_ms", "upper_ms", "final_ms",
                                                                       "total_ms")},
               "batch_device_ms": med(self.samples["batch_device_ms"]), "batch_total_ms": med(self.samples["batch_total_ms"]),
               "client_process_response_ms": med(self.samples["client_ms"]), "client_recovered_item": self.item_ok,
               "switch_bytes_per_query": self.switch_bytes(), "scan": self.srv.scan_info()}
        return res


def kernel_stats(path):
    rows = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "mod_switch_kernel" in row.get("Name", ""):
                rows.append({"name": row["Name"].split("(")[0], "calls": int(row["Calls"]),
                             "average_ns": float(row["AverageNs"]), "min_ns": float(row["MinNs"]),
                             "max_ns": float(row["MaxNs"]), "total_ns": float(row["TotalDurationNs"])})
    return rows


def run_shape(name, rs, reps, n_queries, res):
    enc, log_items, item_bytes = shape(name)
    rng = np.random.default_rng(2026)
    raw = rng.integers(0, 256, size=(1 << log_items, item_bytes), dtype=np.uint8)
    variants = [Variant(enc, log_items, item_bytes, raw, r, n_queries, np.random.default_rng(7)) for r in rs]
    for v in variants:
        v.round(raw, record=False)
    for _ in range(reps):
        for v in variants:
            v.round(raw)
    out = {"N": enc.poly_modulus_degree, "data_prime_bits": [int(q).bit_length() for q in enc.coeff_modulus[:-1]],
           "log_items": log_items, "bytes_per_item": item_bytes, "dimensions": list(variants[0].pp.dimensions),
           "variants": {"r%d" % v.r: v.report() for v in variants}}
    base = out["variants"]["r0"]
    for v in variants[1:]:
        o = out["variants"]["r%d" % v.r]
        o["upper_ms_over_r0"] = o["single_query_ms"]["upper_ms"]["median"] / base["single_query_ms"]["upper_ms"]["median"]
        o["expected_E_ratio"] = o["expansion_ratio"] / base["expansion_ratio"]
        o["batch_total_ms_over_r0"] = o["batch_total_ms"]["median"] / base["batch_total_ms"]["median"]
    res["shapes"][name] = out
    for key, o in out["variants"].items():
        s = o["single_query_ms"]
        print("%s %s: single %.3f ms (expand %.3f scan %.3f upper %.3f final %.3f) | batch of %d: %.2f ms device, %.2f ms "
              "with download | reply %d B/query | client %.2f ms" %
              (name, key, s["total_ms"]["median"], s["expand_ms"]["median"], s["scan_ms"]["median"], s["upper_ms"]["median"],
               s["final_ms"]["median"], n_queries, o["batch_device_ms"]["median"], o["batch_total_ms"]["median"],
               o["reply_bytes_per_query"], o["client_process_response_ms"]["median"]))
    for v in variants:
        v.db.close()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modswitch.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--cfg4", action="store_true")
    ap.add_argument("--profile-pass", action="store_true", help="20 single queries on cfg 3, r = 1, nothing written")
    ap.add_argument("--kernel-stats", metavar="CSV", help="rocprofv3 kernel stats of a --profile-pass run")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("medians of at least 5 runs")
    if a.profile_pass:
        enc, log_items, item_bytes = shape("cfg3")
        raw = np.random.default_rng(2026).integers(0, 256, size=(1 << log_items, item_bytes), dtype=np.uint8)
        v = Variant(enc, log_items, item_bytes, raw, 1, 1, np.random.default_rng(7))
        v.single(20)
        v.db.close()
        return 0
    res = {"what": "modulus-switched results against the full modulus: variants alternate in one process on fresh "
                   "contexts; medians of `reps` samples with their spread (max - min)",
           "commit": os.environ.get("PIRGPU_PROFILED_COMMIT") or head_commit(), "reps": a.reps, "queries": a.queries,
           "achievable_hbm_TBps": 6.3, "shapes": {}}
    run_shape("cfg3", (0, 1), a.reps, a.queries, res)
    if a.cfg4:
        try:
            run_shape("cfg4", (0, 1, 2), a.reps, a.queries, res)
        except (pir_amd.server.PirGpuError, MemoryError) as e:
            res["shapes"]["cfg4"] = {"skipped": "did not load: %s" % e}
    if a.kernel_stats:
        rows = kernel_stats(a.kernel_stats)
        b = res["shapes"]["cfg3"]["variants"]["r1"]["switch_bytes_per_query"]
        res["switch_kernel_cfg3_r1"] = {"rows": rows, "bytes_per_query": b, "source": os.path.basename(a.kernel_stats)}
        if rows:
            per_query_ns = sum(x["total_ns"] for x in rows) / max(1, min(x["calls"] for x in rows))
            res["switch_kernel_cfg3_r1"].update({"ns_per_query": per_query_ns, "TBps": b / per_query_ns / 1e3})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
