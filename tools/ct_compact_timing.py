"""What PIRGPU_CREATE_CT_COMPACT_REPLY costs and saves in time and bytes, measured.

Shapes: the two of profiles/ctmult.json -- d = 2, 64 x 64 plaintexts of one item each; N = 4096 / k = 2 with a 16-bit
plain modulus and N = 8192 / k = 4 with a 42-bit one -- each per child and with deferred rounding.  Variants: a
ciphertext-multiplication context without the flag ("plain"), one with the flag and result_primes = 1 ("compact_r1") and
one with the flag and result_primes = 0 ("compact_r0": packed only).

Per variant: the device time of a batch of 64 (pirgpu_batch_run to pirgpu_sync, queries staged before the clock), the
same batch with the replies downloaded into a pinned buffer (pirgpu_batch_set_host_replies: every group's replies leave
as soon as they exist, then pirgpu_batch_fetch waits), a lone query (pirgpu_query_run_staged + the fetch of its reply,
query staged before the clock), and the reply bytes per query.  The tool FAILS unless the reply bytes equal
8 * ct_words(N, q, r) exactly (plain: 8 * 2 k N), and unless the unpacked replies of compact_r0 equal plain's word for
word.

Method: one process.  Every round builds a FRESH context per variant, the variants in an order that rotates from round to
round; on it one untimed pass of everything, then the timed one.  One untimed round first.  The JSON keeps every sample,
the medians and the spread (max - min).  Nothing is gated on time: no figure is fixed in advance.

    python tools/ct_compact_timing.py [--out profiles/ct_compact_reply.json] [--reps 5] [--items 4096]"""
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
from pir_amd import parameters as P  # noqa: E402

BATCH = 64
SHAPES = {"n4096_t16": (4096, 16), "n8192_t42": (8192, 42)}
VARIANTS = [("plain", False, 0), ("compact_r1", True, 1), ("compact_r0", True, 0)]


def head_commit() -> str:
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=9", "HEAD"], capture_output=True,
                              text=True).stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def ct_words(N, q, r):
    return 2 * sum(N * (int(v) - 1).bit_length() // 64 for v in q[:r])


def summary(samples):
    return {"median": round(statistics.median(samples), 4), "min": round(min(samples), 4),
            "spread": round(max(samples) - min(samples), 4), "samples": [round(x, 4) for x in samples]}


class World:
    def __init__(self, N, t_bits, items):
        self.enc = P.generate_encryption_params(N, t_bits)
        self.items = items
        self.pp = {r: P.create_pir_parameters(items, 0, 2, self.enc, True, result_primes=r) for r in (0, 1)}
        self.raw = np.random.default_rng(2026).integers(0, 256, size=(items, self.pp[0].bytes_per_item), dtype=np.uint8)
        self.client = pir_amd.PIRClient.Create(self.pp[0], seed=b"ct-compact-timing")
        self.keys, self.rk = self.client.galois_keys(), self.client.relin_key()
        idx = np.random.default_rng(7).choice(items, size=BATCH, replace=False)
        self.queries = np.stack([self.client.create_query_for(int(i)) for i in idx])

    def fresh(self, compact, r, deferred):
        pp = self.pp[r]
        db = pir_amd.PIRDatabase.Create(pp, self.raw, ct_multiplication=True, ct_deferred=deferred, ct_compact_reply=compact)
        srv = pir_amd.PIRServer.Create(db, pp)
        srv.set_galois_keys(self.keys)
        srv.set_relin_key(self.rk)
        srv.set_concurrency(16)
        return db, srv


def batch_ms(srv, queries):
    srv.stage_batch(queries)
    srv.sync()
    t0 = time.perf_counter()
    srv.run_batch()
    srv.sync()
    return (time.perf_counter() - t0) * 1e3


def batch_download_ms(db, srv, queries, host):
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


def lone_ms(srv, query):
    srv.stage_query(query)
    srv.sync()
    t0 = time.perf_counter()
    srv.run_staged()
    srv.fetch_reply()
    return (time.perf_counter() - t0) * 1e3


def host_ring(db, srv):
    lib, h = srv.lib, db.handle
    host = lib.pirgpu_host_reply_buffer(h, BATCH)
    if not host or lib.pirgpu_batch_set_host_replies(h, C.c_void_p(host), BATCH * db.reply_ct_count()):
        raise RuntimeError("no host reply buffer")
    return host


def measure(name, items, reps, deferred):
    N, t_bits = SHAPES[name]
    w = World(N, t_bits, items)
    q = [int(v) for v in w.enc.coeff_modulus[:-1]]
    k = len(q)
    samples = {v[0]: {"batch_ms": [], "batch_with_download_ms": [], "lone_query_ms": []} for v in VARIANTS}
    info, replies = {}, {}
    for rnd in range(reps + 1):                       # round 0 is not kept
        order = VARIANTS[rnd % 3:] + VARIANTS[:rnd % 3]
        for vname, compact, r in order:
            db, srv = w.fresh(compact, r, deferred)
            batch_ms(srv, w.queries)                  # untimed: workspace, lanes, first kernel loads
            dev = batch_ms(srv, w.queries)
            host = host_ring(db, srv)
            batch_download_ms(db, srv, w.queries, host)       # untimed: the copy stream and its events
            dl = batch_download_ms(db, srv, w.queries, host)
            if rnd == 0:
                words = db.reply_ct_words()
                view = np.ctypeslib.as_array(C.cast(host, C.POINTER(C.c_uint64)), shape=(BATCH, db.reply_ct_count(), words)).copy()
                want = 8 * (ct_words(N, q, r or k) if compact else 2 * k * N)
                got = 8 * db.reply_ct_count() * words
                if got != want:
                    raise RuntimeError("%s %s: reply bytes %d, expected %d" % (name, vname, got, want))
                replies[vname] = srv.unpack_replies(view) if compact else view.reshape(BATCH, 1, 2, k, N)
                info[vname] = {"result_primes": r, "reply_ct_words": words, "reply_bytes_per_query": got,
                               "reply_packing": int(db.reply_packing())}
            srv.lib.pirgpu_batch_set_host_replies(db.handle, None, 0)
            lone_ms(srv, w.queries[0])
            lone = lone_ms(srv, w.queries[0])
            if rnd:
                samples[vname]["batch_ms"].append(dev)
                samples[vname]["batch_with_download_ms"].append(dl)
                samples[vname]["lone_query_ms"].append(lone)
            db.close()
        if rnd == 0 and not np.array_equal(replies["compact_r0"], replies["plain"]):
            raise RuntimeError("%s: unpack(compact r = 0 replies) differs from the plain context's replies" % name)
    out = {"N": N, "k": k, "plain_bits": t_bits, "data_prime_bits": [int(v).bit_length() for v in q], "items": items,
           "dimensions": list(w.pp[0].dimensions), "batch": BATCH, "deferred": deferred,
           "compact_r0_unpacked_equals_plain": True, "variants": {}}
    for vname, _, _ in VARIANTS:
        out["variants"][vname] = dict(info[vname], **{key: summary(v) for key, v in samples[vname].items()})
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ct_compact_reply.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--items", type=int, default=4096)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("medians of at least 5 runs")
    res = {"tool": "tools/ct_compact_timing.py",
           "what": "a ciphertext-multiplication context without PIRGPU_CREATE_CT_COMPACT_REPLY against one with it at "
                   "result_primes = 1 and at 0: fresh contexts in rotating order in one process; medians of `reps` samples "
                   "with their spread (max - min), milliseconds",
           "commit": os.environ.get("PIRGPU_PROFILED_COMMIT") or head_commit(), "reps": a.reps, "shapes": {}}
    for name in a.shapes.split(","):
        for deferred in (False, True):
            t0 = time.perf_counter()
            o = measure(name, a.items, a.reps, deferred)
            res["shapes"]["%s/%s" % (name, "deferred" if deferred else "per_child")] = o
            for vname, v in o["variants"].items():
                print("%s %s %s: batch %.3f ms (spread %.3f), with download %.3f (%.3f), lone query %.3f (%.3f), reply %d B" % (
                    name, "deferred" if deferred else "per-child", vname, v["batch_ms"]["median"], v["batch_ms"]["spread"],
                    v["batch_with_download_ms"]["median"], v["batch_with_download_ms"]["spread"],
                    v["lone_query_ms"]["median"], v["lone_query_ms"]["spread"], v["reply_bytes_per_query"]), flush=True)
            print("  (%.1f s)" % (time.perf_counter() - t0), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
