"""What the ciphertext-multiplication mode (PIRGPU_CREATE_CT_MULTIPLY) costs and saves, measured.

Shapes: N = 8192 with a 42-bit plain modulus and N = 4096 with a 16-bit one, d = 2, `--items` items of one plaintext each
(the plain moduli of the reference's own tuples, correctness_test.cpp:99-101: they leave the product a noise budget).
Variants: a ciphertext-multiplication context ("ct": one rounding and one relinearisation per child), one with deferred
rounding ("ct_deferred", PIRGPU_CREATE_CT_DEFERRED: one per row) and a decomposition-mode context of the same shape; all
three live in ONE process on fresh contexts and alternate, `reps` times after one untimed round; the JSON keeps every sample, the medians and the
spread (max - min).

  * single query: the phases of pirgpu_last_timings (HIP events: expansion, scan, upper level, final) over 10 runs per
    sample;
  * a batch of 64 queries at the ABI: host clock around pirgpu_batch_stage + _run + pirgpu_sync ("device") and + the
    download of every reply ("total");
  * reply bytes per query; the counters CT_RELINS and CT_BLOCKS of one single query (ciphertexts key-switched and product
    blocks queued by the upper level);
  * libpirclient's ProcessResponse on one wire-level response (host clock), and whether it recovered the item.

Nothing here is gated: no ratio is fixed in advance.

    python tools/ctmult_timing.py [--out profiles/ctmult.json] [--reps 5] [--items 4096]"""
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

SHAPES = {"n8192_t42": (8192, 42), "n4096_t16": (4096, 16)}


def head_commit() -> str:
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=9", "HEAD"], capture_output=True,
                              text=True).stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def med(v):
    return {"median": statistics.median(v), "spread": max(v) - min(v), "samples": list(v)}


class Variant:
    def __init__(self, enc, items, raw, ct, n_queries, rng, deferred=False):
        self.ct = ct
        self.deferred = deferred
        self.name = "ct_deferred" if deferred else "ct" if ct else "decomposition"
        self.counters = None
        self.pp = P.create_pir_parameters(items, 0, 2, enc, ct)
        self.db = pir_amd.PIRDatabase.Create(self.pp, raw, ct_multiplication=ct, ct_deferred=deferred)
        self.srv = pir_amd.PIRServer.Create(self.db, self.pp)
        self.client = pir_amd.PIRClient.Create(self.pp, seed=b"ctmult-timing")
        self.srv.set_galois_keys(self.client.galois_keys())
        if ct:
            self.srv.set_relin_key(self.client.relin_key())
        self.srv.set_concurrency(16)
        self.idx = [int(i) for i in rng.choice(items, size=n_queries, replace=False)]
        self.queries = np.stack([self.client.create_query_for(i) for i in self.idx])
        self.out = np.zeros((n_queries, self.db.reply_ct_count(), 2, self.srv.reply_k, self.srv.N), dtype=np.uint64)
        self.request = self.client.CreateRequest(self.idx[:1])
        self.samples = {"phases": [], "batch_device_ms": [], "batch_total_ms": [], "client_ms": []}
        self.item_ok = None
        self.response_bytes = 0

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

    def count(self):
        """CT_RELINS and CT_BLOCKS of one single query."""
        if not self.ct:
            return
        for name in ("ct_relins", "ct_blocks"):
            self.db.set_option(name, 0)
        self.srv.stage_query(self.queries[0])
        self.srv.run_staged()
        self.srv.fetch_reply()
        self.counters = {name: self.db.get_option(name) for name in ("ct_relins", "ct_blocks")}

    def client_pass(self, raw):
        response = self.srv.ProcessRequest(self.request)
        t0 = time.perf_counter()
        try:
            self.item_ok = self.client.ProcessResponse(self.idx[:1], response) == [raw[self.idx[0]].tobytes()]
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

    def report(self):
        ph = self.samples["phases"]
        return {"ct_multiplication": self.ct, "ct_deferred": self.deferred, "single_query_counters": self.counters,
                "reply_cts_per_query": self.db.reply_ct_count(),
                "reply_bytes_per_query": self.db.reply_ct_count() * self.db.reply_ct_words() * 8,
                "response_bytes_one_query": self.response_bytes,
                "single_query_ms": {p: med([s[p] for s in ph]) for p in ("expand_ms", "scan_ms", "upper_ms", "final_ms",
                                                                        "total_ms")},
                "batch_device_ms": med(self.samples["batch_device_ms"]), "batch_total_ms": med(self.samples["batch_total_ms"]),
                "client_process_response_ms": med(self.samples["client_ms"]), "client_recovered_item": self.item_ok,
                "scan": self.srv.scan_info()}


def run_shape(name, items, reps, n_queries, res):
    N, t_bits = SHAPES[name]
    enc = P.generate_encryption_params(N, t_bits)
    width = P.create_pir_parameters(items, 0, 2, enc).bytes_per_item
    raw = np.random.default_rng(2026).integers(0, 256, size=(items, width), dtype=np.uint8)
    variants = [Variant(enc, items, raw, ct, n_queries, np.random.default_rng(7), deferred)
                for ct, deferred in ((True, False), (True, True), (False, False))]
    for v in variants:
        v.round(raw, record=False)
        v.count()
    for _ in range(reps):
        for v in variants:
            v.round(raw)
    out = {"N": N, "plain_bits": t_bits, "data_prime_bits": [int(q).bit_length() for q in enc.coeff_modulus[:-1]],
           "items": items, "bytes_per_item": width, "dimensions": list(variants[0].pp.dimensions),
           "variants": {v.name: v.report() for v in variants}}
    ct, de = out["variants"]["ct"]["single_query_ms"], out["variants"]["ct_deferred"]["single_query_ms"]
    # the one upper level of d = 2 is recorded as the phase `final`
    out["deferred_over_per_child"] = {p: de[p]["median"] / ct[p]["median"] for p in ("final_ms", "total_ms")}
    out["deferred_over_per_child"]["batch_device_ms"] = (out["variants"]["ct_deferred"]["batch_device_ms"]["median"] /
                                                         out["variants"]["ct"]["batch_device_ms"]["median"])
    res["shapes"][name] = out
    for key, o in out["variants"].items():
        s = o["single_query_ms"]
        print("%s %s: single %.3f ms (expand %.3f scan %.3f upper %.3f final %.3f) | batch of %d: %.2f ms device, %.2f ms "
              "with download | reply %d B/query | client %.2f ms (item %s)" %
              (name, key, s["total_ms"]["median"], s["expand_ms"]["median"], s["scan_ms"]["median"], s["upper_ms"]["median"],
               s["final_ms"]["median"], n_queries, o["batch_device_ms"]["median"], o["batch_total_ms"]["median"],
               o["reply_bytes_per_query"], o["client_process_response_ms"]["median"], o["client_recovered_item"]))
        if o["single_query_counters"]:
            print("%s %s: %s" % (name, key, o["single_query_counters"]))
    print("%s deferred / per-child: %s" % (name, out["deferred_over_per_child"]))
    for v in variants:
        v.db.close()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctmult.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--items", type=int, default=4096)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("medians of at least 5 runs")
    res = {"what": "ciphertext-multiplication mode, per child and with deferred rounding, against decomposition mode on the "
                   "same shape: the three alternate in one process on fresh contexts; medians of `reps` samples with their spread (max - min)",
           "commit": os.environ.get("PIRGPU_PROFILED_COMMIT") or head_commit(), "reps": a.reps, "queries": a.queries,
           "shapes": {}}
    for name in SHAPES:
        run_shape(name, a.items, a.reps, a.queries, res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
