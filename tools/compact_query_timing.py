"""What compact queries cost and save on the wire path: one pirgpu_process_requests call of 64
single-query requests of one client whose keys are resident, at two shapes --

  4096   N = 4096, k = 2 (36-bit primes), 2^20 items of 288 bytes, d = 2: the benchmark's headline shape;
  8192   N = 8192, k = 3 (43 / 43 / 44 bits), 2^16 items of 288 bytes, d = 2

-- under four conditions:

  a  full      public-key queries as Ciphertext::save writes them (mode 0);
  b  host      seeded queries (mode 1) with PIRGPU_WIRE_QUERY_EXPAND=0: expanded on the host's parse pool, what a server
               without this path does with such requests;
  c  seeded    the same requests, expanded on the device;
  d  packed    seeded and packed queries (mode 2), unpacked and expanded on the device.

Per condition: the bytes of one request and of its query field, the wall time of the call at the C ABI (the responses are
complete when it returns), and a lone request's latency (pirgpu_process_request).  Per form (c, d): the HIP-event
time of one piece of 8 queries on the context's stream -- its upload, query_unpack_kernel and seed_expand_kernel alone,
queued behind a plug of device work so that no host time lies between the two events (piece_ms).  Conditions b and c send the same bytes: their responses must be equal, and the tool fails otherwise; so it does
when a condition's queries were not expanded where the condition says (pirgpu_query_expand_stats).  Whether the first
response of a condition decodes to its item is recorded, not required: the shapes are the benchmark's, which compares
ciphertexts; the items are recovered in tests/test_gpu_query_compact.py.

    python tools/compact_query_timing.py [--out profiles/compact_queries.json] [--reps 5] [--shapes 4096,8192]

Method: one process, one context per shape, one untimed round, then `reps` rounds with the four conditions in rotating
order.  The JSON keeps every sample, the medians and the spread (max - min), and the ratios of c and d to b and to a."""
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

import torch  # noqa: E402  (first: its HIP runtime is the one the process loads; the events below are torch's)

import pir_amd  # noqa: E402
from pir_amd import parameters as P  # noqa: E402

BATCH = 64
PIECE = 8
CONDITIONS = {"full": (0, None), "host": (1, "0"), "seeded": (1, None), "packed": (2, None)}


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


def summary(samples):
    return {"median": round(statistics.median(samples), 4), "min": round(min(samples), 4),
            "spread": round(max(samples) - min(samples), 4), "samples": [round(x, 4) for x in samples]}


def set_gate(value):
    os.environ["PIRGPU_ALLOW_ENV"] = "1"
    if value is None:
        os.environ.pop("PIRGPU_WIRE_QUERY_EXPAND", None)
    else:
        os.environ["PIRGPU_WIRE_QUERY_EXPAND"] = value


class Call:
    """The arguments of one pirgpu_process_requests call, built once."""

    def __init__(self, srv, requests):
        self.srv, self.n = srv, len(requests)
        self.bufs = [np.frombuffer(r, dtype=np.uint8) for r in requests]
        self.ptrs = (C.c_void_p * self.n)(*[b.ctypes.data for b in self.bufs])
        self.lens = (C.c_size_t * self.n)(*[len(r) for r in requests])
        self.resp = (C.c_void_p * self.n)()
        self.rlen = (C.c_size_t * self.n)()
        self.status = (C.c_int * self.n)()

    def run(self):
        lib, h = self.srv.lib, self.srv.db.handle
        t0 = time.perf_counter()
        lib.pirgpu_process_requests(h, self.n, self.ptrs, self.lens, self.resp, self.rlen, self.status)
        dt = (time.perf_counter() - t0) * 1e3
        if any(self.status[i] for i in range(self.n)):
            raise RuntimeError("request failed: %s" % [lib.pirgpu_request_error(i).decode() for i in range(self.n)])
        out = [C.string_at(self.resp[i], self.rlen[i]) for i in range(self.n)]
        for i in range(self.n):
            lib.pirgpu_free(self.resp[i])
        return dt, out


def lone_ms(srv, request) -> float:
    t0 = time.perf_counter()
    srv.ProcessRequest(request)
    return (time.perf_counter() - t0) * 1e3


def piece_ms(srv, client, indexes, packed: bool, reps: int):
    """HIP-event time of one piece of 8 on the context's stream: its upload, query_unpack_kernel and seed_expand_kernel,
    nothing else.  The piece is staged with the asynchronous entry from the context's pinned buffer while the stream is
    still busy with a plug of device fills queued in front: the host's range check and the three enqueues happen under
    the plug, the first event fires when the plug ends and the second behind the expansion.  A sample whose first event
    had already fired when the call returned (the plug was too short) is dropped and the plug doubled."""
    lib, h = srv.lib, srv.db.handle
    objs = np.stack([client.create_query_compact(i, packed) for i in indexes[:PIECE]])
    host = lib.pirgpu_host_query_buffer(h, PIECE)
    if not host:
        raise RuntimeError("no pinned query buffer")
    np.ctypeslib.as_array(C.cast(host, C.POINTER(C.c_uint64)), shape=(objs.size,))[:] = objs.reshape(-1)
    stream = torch.cuda.ExternalStream(srv.stream_handle())
    plug = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
    out, fills, r = [], 40, 0
    while len(out) < reps:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            for _ in range(fills):
                plug.fill_(r & 1)
        e0.record(stream)
        rc = lib.pirgpu_batch_stage_compact_async(h, C.cast(host, C.POINTER(C.c_uint64)), objs.shape[1], PIECE,
                                                  1 if packed else 0)
        under_plug = not e0.query()
        e1.record(stream)
        e1.synchronize()
        if rc:
            raise RuntimeError("pirgpu_batch_stage_compact_async: %d %s" % (rc, lib.pirgpu_last_error(h).decode()))
        if not under_plug:                                # the events would time the host: a longer plug, sample dropped
            fills *= 2
            if fills > 2560:
                raise RuntimeError("the plug ends before the piece is queued")
            continue
        if r:                                             # the first good sample warms the path
            out.append(e0.elapsed_time(e1))
        r += 1
    srv.unstage_batch()
    srv.sync()
    return out


def measure_shape(N: int, reps: int):
    pp = shape_params(N)
    raw = np.random.default_rng(N).integers(0, 256, size=(pp.num_items, 288), dtype=np.uint8)
    client = pir_amd.PIRClient.Create(pp, seed=b"compact-query-timing")
    db = pir_amd.PIRDatabase.Create(pp, raw)
    srv = pir_amd.PIRServer.Create(db, pp)
    indexes = [(7919 * (i + 1)) % pp.num_items for i in range(BATCH)]
    calls, info = {}, {}
    for name, (mode, _) in CONDITIONS.items():
        if name == "seeded":                              # the same bytes as "host": only the gate differs
            calls[name], info[name] = calls["host"], info["host"]
            continue
        client.set_compact_queries(mode)
        reqs = [client.CreateRequest([i]) for i in indexes]
        calls[name] = Call(srv, reqs)
        fields = [len(p) for n, p in _fields(reqs[0]) if n == 1]
        info[name] = {"request_bytes": len(reqs[0]), "query_field_bytes": sum(fields), "lone_request": reqs[0]}
    client.set_compact_queries(0)
    samples = {c: {"call_ms": [], "lone_ms": []} for c in CONDITIONS}
    responses, decodes = {}, {}
    names = list(CONDITIONS)
    for rnd in range(reps + 1):                           # round 0 is not kept: keys become resident, buffers grow
        order = names[rnd % 4:] + names[:rnd % 4]
        for name in order:
            set_gate(CONDITIONS[name][1])
            before = srv.query_expand_stats()["expanded"]
            dt, out = calls[name].run()
            took_device = srv.query_expand_stats()["expanded"] - before
            if took_device != (BATCH * client.query_ct_count if name in ("seeded", "packed") else 0):
                raise RuntimeError("%s: %d ciphertexts expanded on the device" % (name, took_device))
            lone = lone_ms(srv, info[name]["lone_request"])
            if rnd == 0:
                responses[name] = out
                try:                                      # recorded, not required (see the head of the file)
                    decodes[name] = client.ProcessResponse([indexes[0]], out[0]) == [raw[indexes[0]].tobytes()]
                except pir_amd.PirGpuError:
                    decodes[name] = False
            else:
                samples[name]["call_ms"].append(dt)
                samples[name]["lone_ms"].append(lone)
    set_gate(None)
    if responses["host"] != responses["seeded"]:
        raise RuntimeError("N = %d: host and device expansion give different responses" % N)
    pieces = {"seeded": summary(piece_ms(srv, client, indexes, False, reps)),
              "packed": summary(piece_ms(srv, client, indexes, True, reps))}
    q = [int(v) for v in pp.encryption_parameters.coeff_modulus[:-1]]
    out = {"N": N, "k": len(q), "widths": [(v - 1).bit_length() for v in q], "items": pp.num_items,
           "dimensions": list(pp.dimensions), "batch": BATCH, "query_cts": client.query_ct_count,
           "responses_equal_host_vs_device": True, "first_response_decodes_to_its_item": decodes}
    for name in CONDITIONS:
        out[name] = {"request_bytes": info[name]["request_bytes"], "query_field_bytes": info[name]["query_field_bytes"],
                     "call_ms": summary(samples[name]["call_ms"]), "lone_request_ms": summary(samples[name]["lone_ms"])}
    for name in pieces:
        out[name]["piece_of_8_upload_unpack_expand_event_ms"] = pieces[name]
    med = lambda n: out[n]["call_ms"]["median"]
    out["ratios_of_call_ms"] = {"%s/%s" % (a, b): round(med(a) / med(b), 4) for a in ("seeded", "packed")
                                for b in ("host", "full")}
    db.close()
    return out


def _fields(buf):
    """(field number, payload) of a serialized proto3 message with length-delimited fields only."""
    i, out = 0, []
    while i < len(buf):
        tag = shift = 0
        while True:
            b = buf[i]
            i += 1
            tag |= (b & 0x7F) << shift
            shift += 7
            if not b & 0x80:
                break
        ln = shift = 0
        while True:
            b = buf[i]
            i += 1
            ln |= (b & 0x7F) << shift
            shift += 7
            if not b & 0x80:
                break
        out.append((tag >> 3, buf[i:i + ln]))
        i += ln
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact_queries.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="4096,8192")
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("--reps must be at least 5")
    result = {"tool": "tools/compact_query_timing.py", "commit": head_commit(), "reps": args.reps, "shapes": {}}
    for N in (int(x) for x in args.shapes.split(",")):
        t0 = time.perf_counter()
        shape = measure_shape(N, args.reps)
        result["shapes"][str(N)] = shape
        print("N = %d: %.1f s; call ms full %.3f host %.3f seeded %.3f packed %.3f; request bytes %d -> %d -> %d" % (
            N, time.perf_counter() - t0, shape["full"]["call_ms"]["median"], shape["host"]["call_ms"]["median"],
            shape["seeded"]["call_ms"]["median"], shape["packed"]["call_ms"]["median"],
            shape["full"]["query_field_bytes"], shape["seeded"]["query_field_bytes"],
            shape["packed"]["query_field_bytes"]), file=sys.stderr, flush=True)
        with open(args.out, "w") as f:                    # after every shape: a later shape's failure keeps the earlier one
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
