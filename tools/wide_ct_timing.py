"""Wide items in ciphertext-multiplication mode, and what the shared-selector path (option CT_SHARED_SEL, DESIGN.md section
6.6) is worth, measured.

Wide shapes: `--items` items (default 26 244 = 162 x 162) of 30 000 bytes, d = 2, three planes each -- N = 4096 with a 24-bit
plain modulus (23 bits per coefficient) and N = 8192 / k = 4 with a 42-bit one at 14 bits per coefficient.  Per shape three
contexts live in ONE process and alternate, `reps` times after one untimed round:

  * "ct_shared"    deferred ciphertext-multiplication context, CT_SHARED_SEL = 1;
  * "ct_baseline"  the same with CT_SHARED_SEL = 0: the four-polynomial kernels, unchanged;
  * "decomposition" a wide decomposition-mode context.

Per context: a batch of `--queries` queries at the ABI -- host clock around pirgpu_batch_stage + _run + pirgpu_sync
("device") and + the download of every reply ("total") --, one single query's phases (the one upper level of d = 2 is the
phase `final`), reply bytes per query and the counters CT_LIFTS / CT_BLOCKS / CT_RELINS of one single query.  The JSON keeps
every sample, the medians and the spread (max - min).  A shape whose chain the mode's plan refuses is recorded with the
refusal.

"narrow": CT_SHARED_SEL = 1 against 0 on deferred contexts WITHOUT wide items, d = 2 and d = 3, 4 096 one-plaintext items
at N = 4096 / 16-bit t (the option's default there is 0; recorded for a later decision).

Nothing here is gated: no ratio is fixed in advance.

    python tools/wide_ct_timing.py [--out profiles/wide_ct.json] [--reps 5] [--queries 64] [--items 26244]"""
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

ITEM_BYTES = 30000
WIDE_SHAPES = {"n4096_t24": (4096, 24, 0), "n8192_k4_t42": (8192, 42, 14)}      # N, plain bits, bits per coefficient
COUNTERS = ("ct_lifts", "ct_blocks", "ct_relins")
PHASES = ("expand_ms", "scan_ms", "upper_ms", "final_ms", "total_ms")


def head_commit() -> str:
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=9", "HEAD"], capture_output=True,
                              text=True).stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def med(v):
    return {"median": statistics.median(v), "spread": max(v) - min(v), "samples": list(v)}


class Variant:
    def __init__(self, name, pp, raw, n_queries, ct, shared=None):
        self.name, self.ct, self.pp = name, ct, pp
        self.db = pir_amd.PIRDatabase.Create(pp, ct_multiplication=ct, ct_deferred=ct)
        if shared is not None:
            self.db.set_option("ct_shared_sel", shared)
        self.db.populate(raw)
        self.srv = pir_amd.PIRServer.Create(self.db, pp)
        self.client = pir_amd.PIRClient.Create(pp, seed=b"wide-ct-timing")
        self.srv.set_galois_keys(self.client.galois_keys())
        if ct:
            self.srv.set_relin_key(self.client.relin_key())
        self.srv.set_concurrency(16)
        idx = [int(i) for i in np.random.default_rng(7).choice(pp.num_items, size=n_queries, replace=False)]
        self.queries = np.stack([self.client.create_query_for(i) for i in idx])
        self.out = np.zeros((n_queries, self.db.reply_ct_count(), 2, self.srv.reply_k, self.srv.N), dtype=np.uint64)
        self.samples = {"phases": [], "batch_device_ms": [], "batch_total_ms": []}
        self.counters = None

    def single(self, runs=5):
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

    def count(self):
        if not self.ct:
            return
        for name in COUNTERS:
            self.db.set_option(name, 0)
        self.srv.stage_query(self.queries[0])
        self.srv.run_staged()
        self.srv.fetch_reply()
        self.counters = {name: self.db.get_option(name) for name in COUNTERS}

    def round(self, record=True):
        ph = self.single()
        dev, tot = self.batch()
        if record:
            self.samples["phases"].append(ph)
            self.samples["batch_device_ms"].append(dev)
            self.samples["batch_total_ms"].append(tot)

    def report(self):
        ph = self.samples["phases"]
        return {"ct_multiplication": self.ct, "ct_deferred": self.ct,
                "ct_shared_sel": self.db.get_option("ct_shared_sel") if self.ct else None,
                "single_query_counters": self.counters, "reply_cts_per_query": self.db.reply_ct_count(),
                "reply_bytes_per_query": self.db.reply_ct_count() * self.db.reply_ct_words() * 8,
                "single_query_ms": {p: med([s[p] for s in ph]) for p in PHASES},
                "batch_device_ms": med(self.samples["batch_device_ms"]), "batch_total_ms": med(self.samples["batch_total_ms"]),
                "scan": self.srv.scan_info()}


def alternate(variants, reps):
    for v in variants:
        v.round(record=False)
        v.count()
    for _ in range(reps):
        for v in variants:
            v.round()
    out = {v.name: v.report() for v in variants}
    for v in variants:
        v.db.close()
    return out


def verdict(out):
    """shared against baseline: the difference of the batch medians against the baseline's own spread."""
    a, b = out["ct_shared"], out["ct_baseline"]
    r = {}
    for key in ("batch_device_ms", "batch_total_ms"):
        r[key] = {"shared_minus_baseline_ms": a[key]["median"] - b[key]["median"], "baseline_spread_ms": b[key]["spread"],
                  "shared_over_baseline": a[key]["median"] / b[key]["median"]}
    r["single_final_ms"] = {"shared_over_baseline": a["single_query_ms"]["final_ms"]["median"] /
                                                    b["single_query_ms"]["final_ms"]["median"]}
    r["shared_not_slower_than_baseline_spread"] = (r["batch_device_ms"]["shared_minus_baseline_ms"] <=
                                                   r["batch_device_ms"]["baseline_spread_ms"])
    return r


def show(shape, out, n_queries):
    for key, o in out.items():
        s = o["single_query_ms"]
        print("%s %s: batch of %d: %.2f ms device (spread %.2f), %.2f ms with download | single %.3f ms, final %.3f ms | "
              "reply %d B/query | %s" % (shape, key, n_queries, o["batch_device_ms"]["median"], o["batch_device_ms"]["spread"],
                                         o["batch_total_ms"]["median"], s["total_ms"]["median"], s["final_ms"]["median"],
                                         o["reply_bytes_per_query"], o["single_query_counters"]))


def run_wide(name, items, reps, n_queries, res):
    N, t_bits, bpc = WIDE_SHAPES[name]
    enc = P.generate_encryption_params(N, t_bits)
    raw = np.random.default_rng(2026).integers(0, 256, size=(items, ITEM_BYTES), dtype=np.uint8)
    pp_ct = P.create_pir_parameters(items, ITEM_BYTES, 2, enc, True, bpc, max_plaintexts_per_item=8)
    pp_de = P.create_pir_parameters(items, ITEM_BYTES, 2, enc, False, bpc, max_plaintexts_per_item=8)
    rec = {"N": N, "plain_bits": t_bits, "bits_per_coeff": pp_ct.max_bytes_per_plaintext * 8 // N,
           "data_prime_bits": [int(q).bit_length() for q in enc.coeff_modulus[:-1]], "items": items,
           "bytes_per_item": ITEM_BYTES, "planes": pp_ct.planes, "dimensions": list(pp_ct.dimensions)}
    res["wide"][name] = rec
    try:
        variants = [Variant("ct_shared", pp_ct, raw, n_queries, True, 1), Variant("ct_baseline", pp_ct, raw, n_queries, True, 0),
                    Variant("decomposition", pp_de, raw, n_queries, False)]
    except pir_amd.server.PirGpuError as e:
        rec["refused"] = e.message
        print("%s: refused: %s" % (name, e.message))
        return
    rec["variants"] = alternate(variants, reps)
    rec["shared_against_baseline"] = verdict(rec["variants"])
    show(name, rec["variants"], n_queries)
    print("%s shared against baseline: %s" % (name, rec["shared_against_baseline"]))


def run_narrow(d, reps, n_queries, res):
    items = 4096
    enc = P.generate_encryption_params(4096, 16)
    pp = P.create_pir_parameters(items, 0, d, enc, True)
    raw = np.random.default_rng(2026).integers(0, 256, size=(items, pp.bytes_per_item), dtype=np.uint8)
    variants = [Variant("ct_shared", pp, raw, n_queries, True, 1), Variant("ct_baseline", pp, raw, n_queries, True, 0)]
    rec = {"N": 4096, "plain_bits": 16, "items": items, "dimensions": list(pp.dimensions), "variants": alternate(variants, reps)}
    rec["shared_against_baseline"] = verdict(rec["variants"])
    res["narrow"]["d%d" % d] = rec
    show("narrow d = %d" % d, rec["variants"], n_queries)
    print("narrow d = %d shared against baseline: %s" % (d, rec["shared_against_baseline"]))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_ct.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--items", type=int, default=26244)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("medians of at least 5 runs")
    res = {"what": "wide items (30 000 bytes, 3 planes) on a deferred ciphertext-multiplication context with CT_SHARED_SEL = 1 "
                   "and = 0 (the four-polynomial kernels) and on a decomposition-mode context; CT_SHARED_SEL = 1 against 0 on "
                   "contexts without wide items; contexts alternate in one process, medians of `reps` samples with their "
                   "spread (max - min)",
           "commit": os.environ.get("PIRGPU_PROFILED_COMMIT") or head_commit(), "reps": a.reps, "queries": a.queries,
           "wide": {}, "narrow": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

    for name in WIDE_SHAPES:
        run_wide(name, a.items, a.reps, a.queries, res)
        save()
    for d in (2, 3):
        run_narrow(d, a.reps, a.queries, res)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
