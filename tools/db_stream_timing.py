"""Load time and device memory of a streamed database context (pirgpu_create_ex, PIRGPU_CREATE_STREAMED_DB) against the
plain load, at the benchmark's cfg 3 shape (N = 4096, 2^20 items of 288 bytes, d = 2, 162 x 162):

    (a) plain     pirgpu_db_load_items + pirgpu_db_finalize(ctx, 1)      (u64 staging copy, packed, then released)
    (b) streamed  pirgpu_db_load_items at the default DB_STREAM_MB (256)
    (c) streamed  pirgpu_db_load_items at DB_STREAM_MB = 1                (one row band per chunk)

    python tools/db_stream_timing.py [--out profiles/db_stream.json] [--reps 5]
    python tools/db_stream_timing.py --trace-only streamed     # one load only: run it under rocprofv3 --kernel-trace --stats

Timing: host clock around the ABI calls, which are synchronous; the three variants alternate in one process, each on a
fresh context (the first use of a context -- workspace, and on a streamed one the zero-filled operand layout -- is
inside the timed calls of all three; pirgpu_create, where the plain context allocates its staging copy, is recorded
separately).  The JSON keeps every sample, the medians, pirgpu_db_memory of each variant and the ratio b / a."""
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

VARIANTS = [("a_plain_populate_finalize_release", False, None), ("b_streamed_default", True, None),
            ("c_streamed_1mb", True, 1)]


def cfg3():
    p = oracle.create_pir_parameters(1 << 20, 288, 2, N=4096, plain_bits=24)
    enc = EncryptionParams(p.N, list(p.moduli), p.t)
    return p, PIRParameters(num_items=p.num_items, num_pt=p.num_pt, dimensions=list(p.dimensions),
                            encryption_parameters=enc, bytes_per_item=p.bytes_per_item,
                            items_per_plaintext=p.items_per_plaintext, bits_per_coeff=p.bits_per_coeff,
                            use_ciphertext_multiplication=p.use_ciphertext_multiplication)


def load_once(pp, raw, streamed, stream_mb):
    """(create ms, load ms, pirgpu_db_memory) of one fresh context."""
    t0 = time.perf_counter()
    db = pir_amd.PIRDatabase(pp, streamed=streamed)
    if stream_mb is not None:
        db.set_option("DB_STREAM_MB", stream_mb)
    t1 = time.perf_counter()
    db.populate(raw)
    if not streamed:
        db.finalize(release_staging=True)
    t2 = time.perf_counter()
    mem = db.memory()
    db.close()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, mem


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "db_stream.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace-only", choices=["plain", "streamed"], default=None, help="ONE load of this kind, nothing else")
    a = ap.parse_args()
    p, pp = cfg3()
    raw = np.random.default_rng(2026).integers(0, 256, size=(p.num_items, p.bytes_per_item), dtype=np.uint8)
    if a.trace_only:
        _, ms, mem = load_once(pp, raw, a.trace_only == "streamed", None)
        print("traced %s load: %.1f ms, %s" % (a.trace_only, ms, mem))
        return 0
    for _, streamed, mb in VARIANTS:       # throwaway contexts first: module loading and first-touch costs stay out
        load_once(pp, raw, streamed, mb)
    samples = {name: {"create_ms": [], "load_ms": []} for name, _, _ in VARIANTS}
    memory = {}
    for _ in range(a.reps):
        for name, streamed, mb in VARIANTS:
            create_ms, load_ms, mem = load_once(pp, raw, streamed, mb)
            samples[name]["create_ms"].append(create_ms)
            samples[name]["load_ms"].append(load_ms)
            memory[name] = mem
    res = {"what": "database load at cfg 3: plain populate + finalize(release) against streamed populate; host clock "
                   "around the synchronous ABI calls, variants alternating in one process, fresh context each",
           "N": p.N, "num_items": p.num_items, "bytes_per_item": p.bytes_per_item, "num_pt": p.num_pt,
           "dimensions": list(p.dimensions), "reps": a.reps, "variants": {}}
    for name, _, mb in VARIANTS:
        s = samples[name]
        res["variants"][name] = {"db_stream_mb": mb, "load_ms_median": statistics.median(s["load_ms"]),
                                 "load_ms_min": min(s["load_ms"]), "load_ms_samples": s["load_ms"],
                                 "create_ms_median": statistics.median(s["create_ms"]), "memory": memory[name]}
        print("%-36s load median %8.1f ms  min %8.1f ms  create %6.1f ms  %s" %
              (name, statistics.median(s["load_ms"]), min(s["load_ms"]), statistics.median(s["create_ms"]), memory[name]),
              flush=True)
    med = lambda n: res["variants"][n]["load_ms_median"]
    res["ratio_b_over_a"] = med(VARIANTS[1][0]) / med(VARIANTS[0][0])
    res["ratio_c_over_a"] = med(VARIANTS[2][0]) / med(VARIANTS[0][0])
    print("b / a = %.3f   c / a = %.3f" % (res["ratio_b_over_a"], res["ratio_c_over_a"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
