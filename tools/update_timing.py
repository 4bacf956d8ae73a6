"""Cost of in-place database updates (pirgpu_db_update_items) against a full reload, at the benchmark's cfg 3 shape
(N = 4096, 2^20 items of 288 bytes, d = 2, 162 x 162) with the staging copy released (pirgpu_db_finalize(ctx, 1)), the
way bench.py and the multi-GPU step serve.

    python tools/update_timing.py [--out profiles/update_timing.json] [--reps 5]
    python tools/update_timing.py --trace-only 1024      # one update only: run it under rocprofv3 --kernel-trace --stats

Timing: host clock around the ABI call, which is synchronous (it waits for queued work first and for its own kernels
before it returns); populate + finalize are timed the same way on the same context in the same run.  Each update size
is timed `reps` times on fresh random item indices; the JSON keeps every sample and the median."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle  # noqa: E402
import pir_amd  # noqa: E402
from pir_amd.parameters import EncryptionParams, PIRParameters  # noqa: E402

SIZES = [1, 64, 1024, 16384]


def cfg3():
    p = oracle.create_pir_parameters(1 << 20, 288, 2, N=4096, plain_bits=24)
    enc = EncryptionParams(p.N, list(p.moduli), p.t)
    return p, PIRParameters(num_items=p.num_items, num_pt=p.num_pt, dimensions=list(p.dimensions),
                            encryption_parameters=enc, bytes_per_item=p.bytes_per_item,
                            items_per_plaintext=p.items_per_plaintext, bits_per_coeff=p.bits_per_coeff,
                            use_ciphertext_multiplication=p.use_ciphertext_multiplication)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace-only", type=int, default=0, help="populate, finalize, then ONE update of this many items")
    a = ap.parse_args()
    p, pp = cfg3()
    rng = np.random.default_rng(2026)
    raw = rng.integers(0, 256, size=(p.num_items, p.bytes_per_item), dtype=np.uint8)
    if not a.trace_only:        # a throwaway context first: module loading and first-touch costs stay out of the timing
        warm = pir_amd.PIRDatabase(pp)
        warm.populate(raw)
        warm.finalize(release_staging=True)
        warm.close()
    db = pir_amd.PIRDatabase(pp)
    t0 = time.perf_counter()
    db.populate(raw)
    t1 = time.perf_counter()
    db.finalize(release_staging=True)
    t2 = time.perf_counter()
    if a.trace_only:
        idx = rng.choice(p.num_items, size=a.trace_only, replace=False)
        db.update_items(idx, rng.integers(0, 256, size=(a.trace_only, p.bytes_per_item), dtype=np.uint8))
        print("traced update of %d items" % a.trace_only)
        return 0
    db.update_items([0], raw[:1])          # first call: lazy HIP module loading of the update kernels
    res = {"what": "pirgpu_db_update_items at cfg 3, staging released; host clock around the synchronous ABI call",
           "N": p.N, "num_items": p.num_items, "bytes_per_item": p.bytes_per_item, "num_pt": p.num_pt,
           "dimensions": list(p.dimensions), "items_per_plaintext": p.items_per_plaintext,
           "populate_ms": (t1 - t0) * 1e3, "finalize_release_ms": (t2 - t1) * 1e3,
           "populate_finalize_ms": (t2 - t0) * 1e3, "reps": a.reps, "updates": []}
    for n in SIZES:
        samples, touched = [], []
        for _ in range(a.reps):
            idx = rng.choice(p.num_items, size=n, replace=False)
            items = rng.integers(0, 256, size=(n, p.bytes_per_item), dtype=np.uint8)
            t = time.perf_counter()
            db.update_items(idx, items)
            samples.append((time.perf_counter() - t) * 1e3)
            touched.append(len(set((idx // p.items_per_plaintext).tolist())))
        res["updates"].append({"items": n, "touched_plaintexts_mean": statistics.mean(touched),
                               "ms_median": statistics.median(samples), "ms_min": min(samples), "ms_samples": samples})
        print("update %6d items (%8.1f plaintexts): median %9.3f ms   min %9.3f ms" %
              (n, statistics.mean(touched), statistics.median(samples), min(samples)), flush=True)
    print("populate %.1f ms + finalize(release) %.1f ms = %.1f ms" %
          (res["populate_ms"], res["finalize_release_ms"], res["populate_finalize_ms"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    db.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
