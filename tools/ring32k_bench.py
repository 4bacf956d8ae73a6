#!/usr/bin/env python3
"""Recorded figures at ring degree N = 32768 (profiles/ring32k.txt): not a bench.py configuration.

Config: database 2^log_items x 288 B, d = 2, four 49-bit data primes + a 50-bit special prime (SEAL
CoeffModulus::Create(32768, {49, 49, 49, 49, 50})), 24-bit batching plain modulus -- a chain below 2^55, so the scan
is the int8-MFMA one with 7 digits.  Prints one JSON line:

  * latency_ms_single_query   median wall time of process_query (one query, keys resident)
  * batch_qps                 queries/s of stage_batch + run_batch over --batch queries (median of --reps)
  * transform                 the two-pass transform alone on --ntt-polys polynomials (ntt_batch through the
                              pirgpu_ntt_forward / _inverse test entry points): bytes each pass moves (read + write of
                              every polynomial) -- divide by the per-kernel times of a `rocprofv3 --kernel-trace
                              --stats` run of this script for GB/s against the 8 TB/s HBM peak.

Run from the repository root:  python3 tools/ring32k_bench.py [--log-items 20] [--batch 64]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pir_amd  # noqa: E402
from pir_amd import parameters as P  # noqa: E402

N = 32768


def chain():
    # SEAL CoeffModulus::Create(N, {49 x 4, 50}): per bit size the largest primes = 1 mod 2N below 2^bits
    out = []
    for bits, cnt in ((49, 4), (50, 1)):
        v, found = (1 << bits) - 2 * N + 1, []
        while len(found) < cnt:
            if P._is_prime(v):
                found.append(v)
            v -= 2 * N
        out += sorted(found)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-items", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--latency-runs", type=int, default=10)
    ap.add_argument("--ntt-polys", type=int, default=512)
    ap.add_argument("--ntt-reps", type=int, default=10)
    a = ap.parse_args()
    enc = P.generate_encryption_params(N, 24, coeff_modulus=chain())
    n_items = 1 << a.log_items
    pp = P.create_pir_parameters(n_items, 288, 2, enc)
    raw = np.random.default_rng(1).integers(0, 256, size=(n_items, 288), dtype=np.uint8)
    t0 = time.time()
    db = pir_amd.PIRDatabase.Create(pp, raw)
    srv = pir_amd.PIRServer.Create(db, pp)
    t_db = time.time() - t0
    client = pir_amd.PIRClient.Create(pp, seed=b"ring32k-bench")
    srv.set_galois_keys(client.galois_keys())
    info = srv.scan_info()

    idx = [(7919 * i + 11) % n_items for i in range(max(a.batch, a.latency_runs))]
    queries = [client.create_query_for(i) for i in idx]
    reply = srv.process_query(queries[0])                       # warm-up + correctness
    pt = client.process_reply(reply)
    off = (idx[0] % pp.items_per_plaintext) * 288
    assert client.string_decode(pt, 288, off) == raw[idx[0]].tobytes()
    lat = []
    for q in queries[:a.latency_runs]:
        t0 = time.perf_counter()
        srv.process_query(q)
        lat.append(time.perf_counter() - t0)

    batch = np.stack(queries[:a.batch])
    srv.set_concurrency(16)
    qps = []
    for _ in range(a.reps + 1):
        t0 = time.perf_counter()
        srv.stage_batch(batch)
        srv.run_batch()
        srv.sync()
        qps.append(a.batch / (time.perf_counter() - t0))
    got = srv.fetch_batch()
    assert np.array_equal(got[0], reply)

    k = len(enc.coeff_modulus) - 1
    cts = np.zeros((a.ntt_polys // (2 * k), 2, k, N), dtype=np.uint64)
    for j in range(k):
        cts[:, :, j, :] = np.random.default_rng(j).integers(0, enc.coeff_modulus[j], size=cts[:, :, j, :].shape,
                                                            dtype=np.uint64)
    for _ in range(a.ntt_reps):
        fwd = srv.ntt_forward(cts)
        assert np.array_equal(srv.ntt_inverse(fwd), cts)
    polys = cts.shape[0] * 2 * k
    print(json.dumps({
        "config": {"N": N, "items": n_items, "item_bytes": 288, "d": 2, "dims": pp.dimensions, "k": k,
                   "data_prime_bits": [q.bit_length() for q in enc.coeff_modulus[:-1]],
                   "special_prime_bits": enc.coeff_modulus[-1].bit_length(), "plain_bits": 24, "scan": info},
        "db_create_populate_s": round(t_db, 2),
        "latency_ms_single_query": round(1e3 * float(np.median(lat)), 2),
        "batch": a.batch, "batch_qps": round(float(np.median(qps[1:])), 2),
        "transform": {"polys_per_launch": polys, "bytes_per_pass_launch": polys * 2 * N * 8,
                      "launches_per_pass": 2 * a.ntt_reps},
    }))
    db.close()


if __name__ == "__main__":
    main()
