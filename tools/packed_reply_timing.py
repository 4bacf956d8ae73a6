"""What packed replies (PIRGPU_CREATE_PACKED_REPLIES) cost and save: a batch of 64 queries with the
flag off and on, at two shapes --

  4096   N = 4096, k = 2 (36-bit primes), 2^20 items of 288 bytes, d = 2: the benchmark's headline shape;
  8192   N = 8192, k = 3 (43 / 43 / 44 bits), 2^16 items of 288 bytes, d = 2.

Per shape and per form: the device time of the batch (pirgpu_batch_run to pirgpu_sync, queries staged before the clock),
the time with the replies downloaded into a preallocated pinned buffer (pirgpu_batch_set_host_replies: every group's
replies leave as soon as they exist, then pirgpu_batch_fetch waits), and the reply bytes.  The byte ratio must equal
sum_j w_j / (64 r) exactly; the tool fails otherwise.  Before anything is timed the packed replies are unpacked and
compared with the unpacked context's, word for word.

    python tools/packed_reply_timing.py [--out profiles/packed_replies.json] [--reps 7] [--shapes 4096,8192]
                                        [--kernel-stats 4096=stats.csv,8192=stats.csv]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python tools/packed_reply_timing.py --trace-only 4096

Method: one process.  Every round builds a FRESH context per form, the two forms in alternating order; on it one untimed
batch, then the timed batch without and the timed batch with the download.  One untimed round first.  The JSON keeps
every sample, the medians and the spread (max - min).  The pack kernel's own time is not visible from the host: it comes
from a kernel trace of --trace-only (one packed context, three batches of 64: 24 launches of reply_pack_kernel, one per
group of 8) whose kernel_stats CSV is handed to --kernel-stats."""
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

# torch first (when it is there): its own HIP runtime must be the one the process loads
try:
    import torch  # noqa: F401
except ImportError:
    torch = None

import pir_amd  # noqa: E402
from pir_amd import parameters as P  # noqa: E402

BATCH = 64


def head_commit() -> str:
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=9", "HEAD"], capture_output=True,
                              text=True).stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def shape_params(N: int):
    if N == 8192:       # three data primes and the special prime of SEAL's default chain
        m = P.BFV_DEFAULT[8192]
        enc = P.generate_encryption_params(8192, 24, coeff_modulus=m[:3] + [m[4]])
        return P.create_pir_parameters(1 << 16, 288, 2, enc)
    return P.create_pir_parameters(1 << 20, 288, 2, P.generate_encryption_params(N, 24))


def fresh(pp, raw, keys, packed: bool):
    db = pir_amd.PIRDatabase.Create(pp, raw, packed_replies=packed)
    srv = pir_amd.PIRServer.Create(db, pp)
    srv.set_galois_keys(keys)
    srv.set_concurrency(16)
    return db, srv


def run_batch_ms(srv, queries) -> float:
    srv.stage_batch(queries)
    srv.sync()
    t0 = time.perf_counter()
    srv.run_batch()
    srv.sync()
    return (time.perf_counter() - t0) * 1e3


def run_batch_download_ms(db, srv, queries, host) -> float:
    lib, h = srv.lib, db.handle
    n = db.reply_ct_count()
    srv.stage_batch(queries)
    srv.sync()
    cnt = C.c_uint64(0)
    t0 = time.perf_counter()
    srv.run_batch()
    rc = lib.pirgpu_batch_fetch(h, C.cast(host, C.POINTER(C.c_uint64)), BATCH * n, C.byref(cnt))
    dt = (time.perf_counter() - t0) * 1e3
    if rc or cnt.value != BATCH * n:
        raise RuntimeError("pirgpu_batch_fetch: %d %s" % (rc, lib.pirgpu_last_error(h).decode()))
    return dt


def host_ring(db, srv):
    lib, h = srv.lib, db.handle
    host = lib.pirgpu_host_reply_buffer(h, BATCH)
    if not host or lib.pirgpu_batch_set_host_replies(h, C.c_void_p(host), BATCH * db.reply_ct_count()):
        raise RuntimeError("no host reply buffer")
    return host


def summary(samples):
    return {"median": round(statistics.median(samples), 4), "min": round(min(samples), 4),
            "spread": round(max(samples) - min(samples), 4), "samples": [round(x, 4) for x in samples]}


def world(N: int):
    pp = shape_params(N)
    raw = np.random.default_rng(N).integers(0, 256, size=(pp.num_items, 288), dtype=np.uint8)
    client = pir_amd.PIRClient.Create(pp, seed=b"packed-reply-timing")
    keys = client.galois_keys()
    queries = np.stack([client.create_query_for((7919 * (i + 1)) % pp.num_items) for i in range(BATCH)])
    return pp, raw, keys, queries


def trace_only(N: int) -> None:
    pp, raw, keys, queries = world(N)
    db, srv = fresh(pp, raw, keys, True)
    for _ in range(3):
        run_batch_ms(srv, queries)
    db.close()


def pack_kernel_stats(path: str):
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "reply_pack_kernel" in row.get("Name", ""):
                return {"launches": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 3),
                        "min_us": round(float(row["MinNs"]) / 1e3, 3), "max_us": round(float(row["MaxNs"]) / 1e3, 3),
                        "source": "rocprofv3 --kernel-trace --stats of --trace-only %s" % os.path.basename(path)}
    raise RuntimeError("%s has no reply_pack_kernel row" % path)


def measure_shape(N: int, reps: int):
    pp, raw, keys, queries = world(N)
    q = [int(v) for v in pp.encryption_parameters.coeff_modulus[:-1]]
    widths = [(v - 1).bit_length() for v in q]
    samples = {f: {"batch_ms": [], "batch_with_download_ms": []} for f in ("unpacked", "packed")}
    info = {}
    for rnd in range(reps + 1):                       # round 0 is not kept
        order = ("unpacked", "packed") if rnd % 2 == 0 else ("packed", "unpacked")
        replies = {}
        for form in order:
            db, srv = fresh(pp, raw, keys, form == "packed")
            run_batch_ms(srv, queries)                # untimed: workspace, lanes, first kernel loads
            dev = run_batch_ms(srv, queries)
            host = host_ring(db, srv)
            run_batch_download_ms(db, srv, queries, host)     # untimed: the copy stream and its events
            dl = run_batch_download_ms(db, srv, queries, host)
            if rnd == 0:
                view = np.ctypeslib.as_array(C.cast(host, C.POINTER(C.c_uint64)),
                                             shape=(BATCH, db.reply_ct_count(), db.reply_ct_words()))
                replies[form] = srv.unpack_replies(view.copy()) if form == "packed" else view.copy().reshape(
                    BATCH, db.reply_ct_count(), 2, len(q), pp.encryption_parameters.poly_modulus_degree)
                info[form] = {"reply_ct_words": db.reply_ct_words(), "reply_cts": db.reply_ct_count(),
                              "reply_bytes": db.reply_ct_count() * db.reply_ct_words() * 8}
            else:
                samples[form]["batch_ms"].append(dev)
                samples[form]["batch_with_download_ms"].append(dl)
            db.close()
        if rnd == 0 and not np.array_equal(replies["packed"], replies["unpacked"]):
            raise RuntimeError("N = %d: unpack(packed replies) differs from the unpacked context's replies" % N)
    num, den = info["packed"]["reply_bytes"], info["unpacked"]["reply_bytes"]
    if num * 64 * len(q) != den * sum(widths):
        raise RuntimeError("N = %d: byte ratio %d / %d is not sum w_j / (64 r) = %d / %d" % (N, num, den, sum(widths), 64 * len(q)))
    out = {"N": N, "k": len(q), "widths": widths, "items": pp.num_items, "dimensions": list(pp.dimensions), "batch": BATCH,
           "byte_ratio": "%d / %d" % (sum(widths), 64 * len(q)), "replies_equal_after_unpack": True}
    for form in samples:
        out[form] = dict(info[form], **{k: summary(v) for k, v in samples[form].items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_replies.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="4096,8192")
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--trace-only", type=int, default=0)
    args = ap.parse_args()
    if args.trace_only:
        trace_only(args.trace_only)
        return
    if args.reps < 5:
        raise SystemExit("--reps must be at least 5")
    stats = dict(kv.split("=", 1) for kv in args.kernel_stats.split(",") if kv)
    result = {"tool": "tools/packed_reply_timing.py", "commit": head_commit(), "reps": args.reps, "shapes": {}}
    for N in (int(x) for x in args.shapes.split(",")):
        t0 = time.perf_counter()
        shape = measure_shape(N, args.reps)
        shape["pack_kernel"] = pack_kernel_stats(stats[str(N)]) if str(N) in stats else None
        result["shapes"][str(N)] = shape
        print("N = %d: %.1f s; batch %.3f -> %.3f ms, with download %.3f -> %.3f ms, reply %d -> %d B" % (
            N, time.perf_counter() - t0, shape["unpacked"]["batch_ms"]["median"], shape["packed"]["batch_ms"]["median"],
            shape["unpacked"]["batch_with_download_ms"]["median"], shape["packed"]["batch_with_download_ms"]["median"],
            shape["unpacked"]["reply_bytes"], shape["packed"]["reply_bytes"]), file=sys.stderr, flush=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
