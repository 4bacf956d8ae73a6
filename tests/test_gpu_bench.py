"""`bench.py --gpus 1` end to end on the GPU at a small size: --steps K times exactly K steps, --dump-outputs DIR
writes the replies of the last timed step -- bit for bit what the CPU oracle computes from the same seeded inputs --, a
plain run reports the headline alone and --full adds the figures that take runs of their own."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_dumps_the_replies_of_the_last_timed_step(tmp_path, oracle_mod):
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update(PIRGPU_BENCH_SKIP_WIRE="1", PIRGPU_BENCH_SKIP_SWEEP="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--log-items", "12", "--batch", "16",
                        "--steps", "3", "--warmup", "1", "--latency-runs", "2", "--no-cpu-baseline",
                        "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["steps"] == 3 and j["timed_blocks"] == 1 and j["ms_per_step"] > 0
    assert abs(j["ms_per_step"] - j["timed_block_seconds"][0] / 3 * 1e3) < 1e-3
    # a plain run: the headline only, none of what --full adds
    assert j["full"] is False and j["unit"] == "queries/s" and j["higher_is_better"] is True and j["dtype"] == "u64"
    assert not set(j) & {"roofline", "roofline_compute", "latency_ms_single_query", "phases_ms_single_query",
                         "cpu_baseline", "batch_reply0_equals_single_query_reply"}, sorted(j)
    assert sorted(os.listdir(out)) == ["replies.npy"]
    got = np.load(out / "replies.npy")

    # the same inputs, made the way bench.py makes them, through the CPU oracle
    sys.path.insert(0, ROOT)
    import bench
    import pir_amd
    enc, pp, _ = bench.build_workload(argparse.Namespace(config=3, log_items=12, dims=2), pir_amd)
    raw, keys, queries = bench.synthetic_inputs(pp, n_queries=16)
    k, N = len(enc.coeff_modulus) - 1, enc.poly_modulus_degree
    assert got.dtype == np.float64 and got.shape[0] == 16 and got.shape[2:] == (2, k, N)
    orc = oracle_mod.Oracle(N, enc.coeff_modulus, enc.plain_modulus)
    bits = pp.bits_per_coeff or oracle_mod.bits_per_coeff(enc.plain_modulus)
    rc, db_ntt = orc.db_encode(raw.tobytes(), pp.num_items, pp.bytes_per_item, pp.items_per_plaintext, bits, pp.num_pt)
    assert rc == 0
    for i in (0, 7, 15):
        rc, want = orc.process_query(db_ntt, pp.dimensions, queries[i], keys)
        assert rc == 0
        assert np.array_equal(got[i].astype(np.uint64), want), i


def test_bench_full_adds_latency_roofline_and_cpu_baseline():
    """--full at a small size: the single-query latency and the scan kernel's roofline from runs of their own, and the
    CPU baseline, whose reply is bit for bit the GPU's (the wire legs and the reference sweep are left out here: they
    run at the reference's own sizes whatever --log-items says)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update(PIRGPU_BENCH_SKIP_WIRE="1", PIRGPU_BENCH_SKIP_SWEEP="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--log-items", "12", "--batch", "16",
                        "--steps", "3", "--warmup", "1", "--latency-runs", "2", "--full"], env=env, capture_output=True,
                       text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["full"] is True and j["steps"] == 3 and j["timed_blocks"] == 1
    assert abs(j["ms_per_step"] - j["timed_block_seconds"][0] / 3 * 1e3) < 1e-3
    assert j["latency_ms_single_query"] > 0 and j["phases_ms_single_query"]["scan_ms"] > 0
    assert j["roofline"]["kernel_ms"] > 0 and j["roofline"]["launches_averaged"] > 0
    assert j["batch_reply0_equals_single_query_reply"] is True
    assert j["cpu_baseline"]["bit_exact_vs_gpu"] is True and j["cpu_baseline"]["value"] > 0
