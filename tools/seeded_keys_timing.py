"""What a NEW client's first request costs with seed-compressed keys, in three forms:

  (a) device   the request as the reference client sends it (Serializable<GaloisKeys>: c0 halves + seeds), the c1
               halves re-sampled by the kernel on the device (the default);
  (b) host     the same bytes with PIRGPU_WIRE_SEED_EXPAND=0: BLAKE2Xb + rejection sampling on the wire pool's threads,
               the whole key set uploaded -- the code path before the device expansion existed;
  (c) expanded the same keys as fully expanded objects (twice the bytes, nothing to sample).

Per shape (N = 4096 / k = 2 and N = 8192 / k = 3, 2^12 items of 288 bytes, d = 2 -- the database size does not enter)
and per form: the first request of one new client at the C ABI (pirgpu_process_request, response freed outside the
clock), and 64 new clients in ONE pirgpu_process_requests call as new clients per second.

    python tools/seeded_keys_timing.py [--out profiles/seeded_keys.json] [--reps 9] [--clients 64] [--shapes 4096,8192]

Method: one process.  The clients (reps + clients + 1 of them per shape, each with its own keys) and their requests in
both encodings are made before anything is timed.  Every round builds a FRESH context per form, the forms in rotating
order; on it, one untimed request of a warm-up client (workspace, staging and the first kernel loads are the
context's, not the client's), then the timed first request of a client this context has not seen -- a different client
every round --, then the timed call with 64 more clients it has not seen.  One untimed round first.  The JSON keeps
every sample, the medians and the spread (max - min).  Before anything is timed the three forms' responses to one
request are compared byte for byte."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

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

FORMS = ("device", "host", "expanded")


def head_commit() -> str:
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=9", "HEAD"], capture_output=True,
                              text=True).stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def shape_params(N: int):
    if N == 8192:       # BASELINE config 4's chain: three data primes and the special prime of SEAL's default
        m = P.BFV_DEFAULT[8192]
        enc = P.generate_encryption_params(8192, 24, coeff_modulus=m[:3] + [m[4]])
    else:
        enc = P.generate_encryption_params(N, 24)
    return P.create_pir_parameters(1 << 12, 288, 2, enc)


def make_client(pp, tag: int):
    cl = pir_amd.PIRClient.Create(pp, seed=b"seeded-keys-timing-%d" % tag)
    q = cl.create_query_for((7919 * (tag + 1)) % pp.num_items)
    cl.set_seeded_keys(True)
    seeded = cl.SaveRequest([q])
    cl.set_seeded_keys(False)
    expanded = cl.SaveRequest([q])
    cl.close()
    return seeded, expanded


def set_form(form: str) -> None:
    os.environ["PIRGPU_ALLOW_ENV"] = "1"
    if form == "host":
        os.environ["PIRGPU_WIRE_SEED_EXPAND"] = "0"
    else:
        os.environ.pop("PIRGPU_WIRE_SEED_EXPAND", None)


def fresh(pp, raw, slots: int):
    db = pir_amd.PIRDatabase.Create(pp, raw)
    srv = pir_amd.PIRServer.Create(db, pp)
    srv.set_keyset_capacity(slots)
    return db, srv


def one_request_ms(srv, request: bytes):
    buf = np.frombuffer(request, dtype=np.uint8)
    resp, rlen = C.c_void_p(), C.c_size_t(0)
    t0 = time.perf_counter()
    rc = srv.lib.pirgpu_process_request(srv.db.handle, buf.ctypes.data_as(capi.u8p), len(request), C.byref(resp), C.byref(rlen))
    dt = (time.perf_counter() - t0) * 1e3
    if rc:
        raise RuntimeError("pirgpu_process_request: %d %s" % (rc, srv.lib.pirgpu_last_error(srv.db.handle).decode()))
    srv.lib.pirgpu_free(resp)
    return dt


def many_requests_ms(srv, requests):
    n = len(requests)
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in requests]
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (C.c_size_t * n)(*[len(r) for r in requests])
    resp, rlen, status = (C.c_void_p * n)(), (C.c_size_t * n)(), (C.c_int * n)()
    t0 = time.perf_counter()
    srv.lib.pirgpu_process_requests_tables(srv.db.handle, n, ptrs, lens, None, resp, rlen, status)
    dt = (time.perf_counter() - t0) * 1e3
    for i in range(n):
        if status[i]:
            raise RuntimeError("request %d: status %d %s" % (i, status[i], srv.lib.pirgpu_request_error(i).decode()))
        srv.lib.pirgpu_free(resp[i])
    return dt


def summary(samples):
    return {"median": round(statistics.median(samples), 4), "min": round(min(samples), 4),
            "spread": round(max(samples) - min(samples), 4), "samples": [round(x, 4) for x in samples]}


def measure_shape(N: int, reps: int, n_clients: int):
    pp = shape_params(N)
    raw = np.random.default_rng(N).integers(0, 256, size=(pp.num_items, 288), dtype=np.uint8)
    total = 1 + (reps + 1) + n_clients
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:     # keygen releases the GIL
        made = list(ex.map(lambda i: make_client(pp, i), range(total)))
    print("N = %d: %d clients in %.1f s" % (N, total, time.perf_counter() - t0), file=sys.stderr, flush=True)
    req = {"device": [m[0] for m in made], "host": [m[0] for m in made], "expanded": [m[1] for m in made]}
    warm, singles, crowd = 0, list(range(1, reps + 2)), list(range(reps + 2, total))
    slots = n_clients + 8

    # the three forms answer one request with the same bytes
    answers, stats = {}, {}
    for form in FORMS:
        set_form(form)
        db, srv = fresh(pp, raw, slots)
        answers[form] = srv.ProcessRequest(req[form][warm])
        # (a library from before the device expansion, given through PIRGPU_LIB for comparison, has no such counters:
        # its "device" form is the host path too)
        stats[form] = srv.keyset_seed_stats() if hasattr(srv, "keyset_seed_stats") else None
        db.close()
    same = answers["device"] == answers["host"] == answers["expanded"]
    if not same:
        raise RuntimeError("the three forms answer one request differently")
    if stats["device"] is not None and (stats["device"]["objects"] == 0 or stats["host"]["objects"] or stats["expanded"]["objects"]):
        raise RuntimeError("a form took the wrong path: %s" % stats)

    first = {f: [] for f in FORMS}
    batch = {f: [] for f in FORMS}
    for r in range(reps + 1):              # round 0 is not kept
        for s in range(len(FORMS)):
            form = FORMS[(r + s) % len(FORMS)]
            set_form(form)
            db, srv = fresh(pp, raw, slots)
            one_request_ms(srv, req[form][warm])
            a = one_request_ms(srv, req[form][singles[r]])
            b = many_requests_ms(srv, [req[form][i] for i in crowd])
            db.close()
            if r:
                first[form].append(a)
                batch[form].append(b)
    out = {"N": N, "k": len(pp.encryption_parameters.coeff_modulus) - 1, "items": pp.num_items,
           "request_bytes": {"seeded": len(req["device"][warm]), "expanded": len(req["expanded"][warm])},
           "objects_expanded_per_client": stats["device"]["objects"] if stats["device"] else None,
           "responses_identical": same,
           "first_request_ms": {f: summary(first[f]) for f in FORMS},
           "new_clients_call_ms": {f: summary(batch[f]) for f in FORMS},
           "new_clients_per_s": {f: round(n_clients / statistics.median(batch[f]) * 1e3, 1) for f in FORMS}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seeded_keys.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--clients", type=int, default=64)
    ap.add_argument("--shapes", default="4096,8192")
    args = ap.parse_args()
    result = {"tool": "tools/seeded_keys_timing.py", "commit": head_commit(), "library_override": bool(os.environ.get("PIRGPU_LIB")),
              "reps": args.reps, "clients_per_call": args.clients,
              "forms": {"device": "seed-compressed keys, c1 halves sampled on the device (default)",
                        "host": "seed-compressed keys, PIRGPU_WIRE_SEED_EXPAND=0: sampled on the host's pool threads",
                        "expanded": "fully expanded key objects"},
              "shapes": []}
    for N in [int(x) for x in args.shapes.split(",")]:
        result["shapes"].append(measure_shape(N, args.reps, args.clients))
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps({s["N"]: {"first_request_ms": {f: s["first_request_ms"][f]["median"] for f in FORMS},
                               "new_clients_per_s": s["new_clients_per_s"]} for s in result["shapes"]}))


if __name__ == "__main__":
    main()
