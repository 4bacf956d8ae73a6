"""Compact queries on the GPU: c0 unpacked by query_unpack_kernel and c1 re-sampled by
seed_expand_kernel where a query is staged, against the Python model (tests/query_compact_model.py), the oracle's
process_query on the model-expanded query, and the ordinary staging of the expanded words.  Everything downstream of the
staged-query buffer must be byte for byte what it was, on every context kind; the wire takes the device path for a
window exactly when every query in it is compact and of one form.

Run as a program (python tests/test_gpu_query_compact.py SCENARIO) this file is the child process of the tests that need
an environment of their own: it prints one JSON line of digests."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import numpy as np
import pytest

import oracle
import pir_amd
import query_compact_model as M
import seal_wire as W
from gpu_helpers import chain, chain_low, to_product_params
from pir_amd import parameters as P
from pir_fixtures import PirSetup, generate_test_db

pytestmark = pytest.mark.gpu

N = 4096
_c1 = {}


def model_c1(seed, q, n):
    key = (seed, tuple(q), n)
    if key not in _c1:
        _c1[key] = W.sample_poly_uniform(seed, list(q), n)
    return _c1[key]


def model_expand(objs, n, q, packed):
    """M.expand_all with the sampled halves cached across the two forms of one ciphertext."""
    objs = np.asarray(objs, dtype=np.uint64)
    flat = objs.reshape(-1, objs.shape[-1])
    out = np.empty((flat.shape[0], 2, len(q), n), dtype=np.uint64)
    for i, o in enumerate(flat):
        assert M.check(o, n, q, packed)
        c0, seed = M.split(o, n, q, packed)
        out[i, 0], out[i, 1] = c0, model_c1(seed, q, n)
    return out.reshape(objs.shape[:-1] + out.shape[1:])


def seed_of(i):
    return hashlib.blake2b(b"compact-query-%d" % i, digest_size=64).digest()


def symmetric_twin(s, query, first_seed):
    """A public-key query of the oracle's client [nq, 2, k, N] -> (c0 [nq, k, N], seeds): the same plaintext at the same
    noise with c1 re-sampled from a seed, c0' = c0 + (c1 - c1') s."""
    orc, cl = s.orc, s.client
    q = [int(v) for v in orc.moduli[:orc.k]]
    c0s, seeds = [], []
    for c in range(query.shape[0]):
        seed = seed_of(first_seed + c)
        c1n = model_c1(seed, q, orc.N)
        c0 = np.empty((orc.k, orc.N), dtype=np.uint64)
        for j in range(orc.k):
            d = (query[c, 1, j] + np.uint64(q[j]) - c1n[j]) % np.uint64(q[j])
            ds = orc.ntt_inv(j, orc.dyadic_mul(j, orc.ntt_fwd(j, d), cl.s_ntt[j]))
            c0[j] = orc.poly_add(j, query[c, 0, j], ds)
        c0s.append(c0)
        seeds.append(seed)
    return np.stack(c0s), seeds


_twins = {}


def compact_query(s, index, first_seed, packed):
    """-> (compact [nq, words], expanded [nq, 2, k, N]) of a valid symmetric query for `index`."""
    q = [int(v) for v in s.orc.moduli[:s.orc.k]]
    key = (id(s), index, first_seed)
    if key not in _twins:                                # one encryption per query: its two forms hold the same c0
        _twins[key] = symmetric_twin(s, s.client.create_query_for(s.params, index), first_seed)
    c0, seeds = _twins[key]
    obj = np.stack([M.compact(c0[c], seeds[c], q, packed) for c in range(c0.shape[0])])
    return obj, model_expand(obj, s.orc.N, q, packed)


def server_of(s, **kw):
    pp = to_product_params(s.params)
    db = pir_amd.PIRDatabase.Create(pp, s.raw, **kw)
    srv = pir_amd.PIRServer.Create(db, pp)
    srv.set_galois_keys(s.galois_keys)
    return db, srv


# ---------------------------------------------------------------- 1. the hook against the model

def bare_server(n, moduli, plain_bits):
    p = oracle.create_pir_parameters(4, 0, 1, N=n, plain_bits=plain_bits, moduli=[int(m) for m in moduli])
    pp = to_product_params(p)
    db = pir_amd.PIRDatabase.Create(pp)
    return db, pir_amd.PIRServer(db, pp)


HOOK_CHAINS = {
    "2048-k1": (2048, oracle.coeff_modulus_create(2048, [27, 27]), 14, False),
    "2048-k2": (2048, chain(2048, [27, 27]), 14, False),
    "2048-k3": (2048, chain(2048, [27, 27, 27]), 14, False),
    "4096-k1": (4096, chain(4096, [36]), 20, False),
    "4096-default": (4096, oracle.BFV_DEFAULT[4096], 20, False),
    "4096-k3": (4096, chain(4096, [36, 36, 37]), 20, False),
    "4096-rejecting": (4096, chain_low(4096, 61), 20, True),       # one draw in eight rejected on both data residues
    "4096-60bit": (4096, chain(4096, [60, 36]), 20, False),
}


def hook_case(n, moduli, plain_bits, rejecting, counts):
    q = [int(m) for m in moduli[:-1]]
    db, srv = bare_server(n, moduli, plain_bits)
    rng = np.random.default_rng(n + len(q))
    total = max(counts)
    c0 = np.stack([np.stack([rng.integers(0, v, n, dtype=np.uint64) for v in q]) for _ in range(total)])
    c0[0, :, 0] = [v - 1 for v in q]                     # the largest residue in the first and the last position
    c0[0, :, -1] = [v - 1 for v in q]
    c0[-1, :, :] = np.array([v - 1 for v in q], dtype=np.uint64)[:, None]
    for packed in (False, True):
        assert srv.query_compact_words(packed) == M.words(n, q, packed)
        objs = np.stack([M.compact(c0[i], seed_of(i), q, packed) for i in range(total)])
        want = model_expand(objs, n, q, packed)
        for cnt in counts:
            before = srv.query_expand_stats()
            got = srv.query_expand(objs[:cnt], packed)
            assert np.array_equal(got, want[:cnt]), (packed, cnt)
            after = srv.query_expand_stats()
            assert after["expanded"] == before["expanded"] + cnt
            assert (after["rejected"] > before["rejected"]) == rejecting, (before, after)
        # a coefficient equal to its modulus: InvalidArgument, nothing expanded
        bad = c0[:2].copy()
        bad[1, -1, -1] = q[-1]
        bad_objs = objs[:2].copy()
        w = M.widths(q, packed)
        tail = M.rpm.poly_words(n, w[-1])
        bad_objs[1, -8 - tail:-8] = M.rpm.pack_poly(bad[1, -1], w[-1])
        before = srv.query_expand_stats()
        with pytest.raises(pir_amd.PirGpuError) as e:
            srv.query_expand(bad_objs, packed)
        assert e.value.code == pir_amd.StatusCode.INVALID_ARGUMENT
        assert "ciphertext data is invalid (coefficient out of range)" in e.value.message
        assert srv.query_expand_stats() == before
    db.close()


@pytest.mark.parametrize("name", sorted(HOOK_CHAINS))
def test_hook_equals_the_model(name):
    n, moduli, plain_bits, rejecting = HOOK_CHAINS[name]
    hook_case(n, moduli, plain_bits, rejecting, (1, 3, 9))     # 9: two pieces of the staging path


def test_hook_at_ring_degree_32768():
    moduli = oracle.coeff_modulus_create(32768, [49, 49, 49, 49, 50])   # the chain of tests/test_gpu_ring32k.py
    hook_case(32768, moduli, 24, False, (2,))


# ---------------------------------------------------------------- 2. a query, end to end

_setups = {}


def setup(items, d, **kw):
    key = (items, d, tuple(sorted(kw.items())))
    if key not in _setups:
        _setups[key] = PirSetup(items, 288, d, N=N, plain_bits=24, **kw)
    return _setups[key]


@pytest.mark.parametrize("d,items", [(2, 1024), (1, 100), (3, 1024)], ids=["d2", "d1", "d3"])
def test_compact_query_equals_the_oracle_and_the_expanded_query(d, items):
    s = setup(items, d)
    if d == 2:
        assert list(s.params.dimensions) == [6, 5]          # the reference's 2^10-item shape
    db, srv = server_of(s)
    index = items - 3
    for packed in (False, True):
        obj, expanded = compact_query(s, index, 100 * d, packed)
        rc, want = s.orc.process_query(s.db_ntt, s.params.dimensions, expanded, s.galois_keys)
        assert rc == 0
        before = srv.query_expand_stats()["expanded"]
        srv.stage_query_compact(obj, packed)
        srv.run_staged()
        got = srv.fetch_reply()
        assert srv.query_expand_stats()["expanded"] == before + obj.shape[0]
        assert np.array_equal(got, want), packed
        srv.stage_query(expanded)
        srv.run_staged()
        assert np.array_equal(srv.fetch_reply(), got), packed
        assert s.client.process_response(s.params, index, got) == s.item(index)
    # a coefficient equal to its modulus: nothing is staged, and the context serves the next query
    bad = obj.copy()
    q0 = int(s.orc.moduli[0])
    w0 = M.rpm.width(q0)
    bad[0, :N * w0 // 64] = M.rpm.pack_poly(np.where(np.arange(N) == 0, q0, 0).astype(np.uint64), w0)
    with pytest.raises(pir_amd.PirGpuError) as e:
        srv.stage_query_compact(bad, True)
    assert e.value.code == pir_amd.StatusCode.INVALID_ARGUMENT and "coefficient out of range" in e.value.message
    srv.stage_query_compact(obj, True)
    srv.run_staged()
    assert np.array_equal(srv.fetch_reply(), got)
    db.close()


def product_world(pp, client_seed, **kw):
    raw = generate_test_db(pp.num_items, pp.bytes_per_item)
    client = pir_amd.PIRClient.Create(pp, seed=client_seed)
    db = pir_amd.PIRDatabase.Create(pp, raw, **kw)
    srv = pir_amd.PIRServer.Create(db, pp)
    if kw.get("ct_multiplication"):
        srv.set_galois_keys(client.galois_keys())
        srv.set_relin_key(client.relin_key())
    else:
        srv.set_galois_keys(client.galois_keys())
    return raw, client, db, srv


def kinds():
    enc = P.generate_encryption_params(N, 24)
    enc16 = P.generate_encryption_params(N, 16)
    return {
        "packed-replies": (P.create_pir_parameters(256, 288, 2, enc), dict(packed_replies=True)),
        "result-primes": (P.create_pir_parameters(256, 288, 2, enc, result_primes=1), {}),
        "wide-items": (P.create_pir_parameters(64, 30000, 2, enc, max_plaintexts_per_item=4), {}),
        "ct-multiplication": (P.create_pir_parameters(256, 0, 2, enc16, True, 6), dict(ct_multiplication=True)),
    }


@pytest.mark.parametrize("kind", ["packed-replies", "result-primes", "wide-items", "ct-multiplication"])
def test_nothing_downstream_changes_on_other_context_kinds(kind):
    """The product client's own compact query (symmetric, seeded and packed) on a context of each kind: the reply is the
    one the expanded words give, and it decodes to the item."""
    pp, kw = kinds()[kind]
    raw, client, db, srv = product_world(pp, b"compact-" + kind.encode(), **kw)
    q = [int(v) for v in pp.encryption_parameters.coeff_modulus[:-1]]
    index = pp.num_items - 2
    for packed in (True, False):
        obj = client.create_query_compact(index, packed)
        expanded = model_expand(obj, N, q, packed)
        srv.stage_query_compact(obj, packed)
        srv.run_staged()
        got = srv.fetch_reply()
        srv.stage_query(expanded)
        srv.run_staged()
        assert np.array_equal(srv.fetch_reply(), got), packed
    # through the wire, the same client in mode 2
    client.set_compact_queries(2)
    before = srv.query_expand_stats()["expanded"]
    response = srv.ProcessRequest(client.CreateRequest([index]))
    assert srv.query_expand_stats()["expanded"] == before + client.query_ct_count
    assert client.ProcessResponse([index], response) == [raw[index].tobytes()]
    db.close()


# ---------------------------------------------------------------- 3. batches

BATCH = 19      # two groups and a partial one


def batch_inputs(s):
    idx = [(s.params.num_items - 1 - 131 * i) % s.params.num_items for i in range(BATCH)]
    sets = {}
    for packed in (False, True):
        pairs = [compact_query(s, idx[i], 1000 + 4 * i, packed) for i in range(BATCH)]
        sets[packed] = (np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]))
    return idx, sets


def batch_scenario():
    """19 queries staged compact (both forms, twice back to back with different queries in between) against the same
    queries staged expanded; returns digests of the replies and the counters."""
    s = setup(3000, 2)
    idx, sets = batch_inputs(s)
    db, srv = server_of(s)
    srv.set_concurrency(16)
    out = {}
    srv.stage_batch(sets[False][1])
    srv.run_batch()
    plain = srv.fetch_batch()
    out["plain"] = hashlib.sha256(plain.tobytes()).hexdigest()
    rc, want = s.orc.process_query(s.db_ntt, s.params.dimensions, sets[False][1][BATCH - 1], s.galois_keys)
    assert rc == 0 and np.array_equal(plain[BATCH - 1], want)
    order = np.arange(BATCH)[::-1].copy()
    for packed in (False, True):
        objs = sets[packed][0]
        # two compact batches back to back: the second may not read the first's staging
        srv.stage_batch_compact(objs[order], packed)
        srv.run_batch()
        launches = db.get_option("SCAN_LAUNCHES")
        srv.stage_batch_compact(objs, packed)
        srv.run_batch()
        got = srv.fetch_batch()
        out["launches"] = db.get_option("SCAN_LAUNCHES") - launches      # database passes of one batch: a pair counts one
        assert np.array_equal(got, plain), packed
        srv.stage_batch_compact(objs[order], packed)
        srv.run_batch()
        assert np.array_equal(srv.fetch_batch(), plain[order]), packed
        out["compact-%d" % packed] = hashlib.sha256(got.tobytes()).hexdigest()
    out["expanded"] = srv.query_expand_stats()["expanded"]
    db.close()
    return out


def child(scenario, env):
    e = dict(os.environ)
    e.update(env)
    e["PIRGPU_ALLOW_ENV"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), scenario], env=e, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().split("\n")[-1])


_batch_out = {}


def child_free_launches():
    """Database passes of the 19-query batch in this process (pairing as the context defaults it)."""
    if not _batch_out:
        _batch_out.update(batch_scenario())
    return _batch_out["launches"]


def test_compact_batch_equals_the_expanded_batch():
    child_free_launches()
    out = _batch_out
    assert out["compact-0"] == out["plain"] and out["compact-1"] == out["plain"]
    assert out["expanded"] == 2 * 3 * BATCH * (sum(setup(3000, 2).params.dimensions) // N + 1)


def test_compact_batch_under_the_paired_pass():
    """PIRGPU_SCAN_MFMA_PAIR=2 in a child process: the paired pass reads pieces the compact path filled."""
    out = child("batch", {"PIRGPU_SCAN_MFMA_PAIR": "2"})
    alone = child_free_launches()
    assert out["launches"] < alone, (out, alone)               # 8 + 8 + 3 queries: a pair and a single, not three passes
    assert out["compact-0"] == out["plain"] and out["compact-1"] == out["plain"]


def test_sharded_contexts_refuse_compact_staging():
    s = setup(3000, 2)
    pp = to_product_params(s.params)
    q = [int(v) for v in s.orc.moduli[:s.orc.k]]
    objs = np.zeros((2, sum(s.params.dimensions) // N + 1, M.words(N, q, True)), dtype=np.uint64)
    for kw in (dict(slots=(0, 1024)), dict(shard=(0, 4))):
        db = pir_amd.PIRDatabase.Create(pp, s.raw, **kw)
        srv = pir_amd.PIRServer(db, pp)
        with pytest.raises(pir_amd.PirGpuError) as e:
            srv.stage_batch_compact(objs, True)
        assert e.value.code == pir_amd.StatusCode.FAILED_PRECONDITION, kw
        with pytest.raises(pir_amd.PirGpuError) as e:
            srv.stage_query_compact(objs[0], True)
        assert e.value.code == pir_amd.StatusCode.FAILED_PRECONDITION, kw
        db.close()


# ---------------------------------------------------------------- 4. the wire

def wire_world(items, seed=b"compact-wire"):
    enc = P.generate_encryption_params(N, 24)
    pp = P.create_pir_parameters(items, 288, 2, enc)
    raw = generate_test_db(items, pp.bytes_per_item)
    client = pir_amd.PIRClient.Create(pp, seed=seed)
    db = pir_amd.PIRDatabase.Create(pp, raw)
    return pp, raw, client, db, pir_amd.PIRServer.Create(db, pp)


@pytest.mark.parametrize("items", [2 ** 8, 2 ** 12])
def test_wire_round_trip_of_a_mode_2_client(items):
    pp, raw, client, db, srv = wire_world(items)
    client.set_compact_queries(2)
    idx = [0, items - 1, items // 2 + 1]
    response = srv.ProcessRequest(client.CreateRequest(idx))
    assert client.ProcessResponse(idx, response) == [raw[i].tobytes() for i in idx]
    assert srv.query_expand_stats()["expanded"] == len(idx) * client.query_ct_count
    client.set_compact_queries(1)
    response = srv.ProcessRequest(client.CreateRequest(idx[:1]))
    assert client.ProcessResponse(idx[:1], response) == [raw[idx[0]].tobytes()]
    assert srv.query_expand_stats()["expanded"] == (len(idx) + 1) * client.query_ct_count
    db.close()


def window_requests(client, n, modes):
    """n single-query requests of one client, request i in compact mode modes[i % len(modes)]."""
    reqs = []
    for i in range(n):
        client.set_compact_queries(modes[i % len(modes)])
        reqs.append(client.CreateRequest([(37 * i + 5) % 256]))
    client.set_compact_queries(0)
    return reqs


def wire_scenario():
    """64 compact requests in one call, and a window of 5 compact and 3 full requests: digests and counters."""
    pp, raw, client, db, srv = wire_world(256)
    out = {}
    reqs = window_requests(client, 64, [2])
    res = srv.ProcessRequests(reqs)
    assert all(rc == 0 for rc, _ in res), srv.request_errors
    out["all-compact"] = hashlib.sha256(b"".join(r for _, r in res)).hexdigest()
    out["all-compact-expanded"] = srv.query_expand_stats()["expanded"]
    for i in (0, 63):
        assert client.ProcessResponse([(37 * i + 5) % 256], res[i][1]) == [raw[(37 * i + 5) % 256].tobytes()]
    before = srv.query_expand_stats()["expanded"]
    mixed = window_requests(client, 8, [2, 2, 0, 2, 0, 2, 0, 2])
    res = srv.ProcessRequests(mixed)
    assert all(rc == 0 for rc, _ in res), srv.request_errors
    out["mixed"] = hashlib.sha256(b"".join(r for _, r in res)).hexdigest()
    out["mixed-expanded"] = srv.query_expand_stats()["expanded"] - before
    assert client.ProcessResponse([(37 * 1 + 5) % 256], res[1][1]) == [raw[(37 * 1 + 5) % 256].tobytes()]
    db.close()
    return out


def test_wire_windows_take_the_device_path_only_when_every_query_is_compact():
    out = wire_scenario()
    host = child("wire", {"PIRGPU_WIRE_QUERY_EXPAND": "0"})
    nq = 1                                                  # 256 items, d = 2: one query ciphertext
    assert out["all-compact-expanded"] == 64 * nq and host["all-compact-expanded"] == 0
    assert out["all-compact"] == host["all-compact"]        # the same response bytes either way
    assert out["mixed-expanded"] == 0 and host["mixed-expanded"] == 0
    assert out["mixed"] == host["mixed"]


def test_wire_request_with_a_coefficient_equal_to_its_modulus():
    pp, raw, client, db, srv = wire_world(256, seed=b"compact-wire-bad")
    q0 = int(pp.encryption_parameters.coeff_modulus[0])
    for mode in (1, 2):
        client.set_compact_queries(mode)
        good = client.CreateRequest([9])
        obj = client.create_query_compact(9, mode == 2)
        w = M.rpm.width(q0) if mode == 2 else 64
        first = M.rpm.unpack_poly(obj[0, :N * w // 64], N, w)
        first[N - 1] = q0
        obj[0, :N * w // 64] = M.rpm.pack_poly(first, w)
        bad = client.SaveRequestCompact([obj], mode == 2)
        before = srv.query_expand_stats()["expanded"]
        with pytest.raises(pir_amd.PirGpuError) as e:
            srv.ProcessRequest(bad)
        assert e.value.code == pir_amd.StatusCode.INVALID_ARGUMENT
        assert "ciphertext data is invalid (coefficient out of range)" in e.value.message
        res = srv.ProcessRequests([good, bad, good])
        assert [rc for rc, _ in res] == [0, pir_amd.StatusCode.INVALID_ARGUMENT, 0]
        assert "coefficient out of range" in srv.request_errors[1]
        assert srv.query_expand_stats()["expanded"] == before + 2
        assert client.ProcessResponse([9], srv.ProcessRequest(good)) == [raw[9].tobytes()]
    db.close()


if __name__ == "__main__":
    print(json.dumps({"batch": batch_scenario, "wire": wire_scenario}[sys.argv[1]]()))
