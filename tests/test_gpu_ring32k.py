"""Ring degree N = 32768 on the GPU (ntt_ring32k.hip: two-pass integer transforms), bit for bit against the oracle.

Two coefficient-modulus sets, each an explicit chain (SEAL's default for this degree has 16 primes, more than the 8 data
primes the server holds), built with SEAL's CoeffModulus::Create:

  * SET_A: four 49-bit data primes + a 50-bit special prime.  Below 2^55: d >= 2 takes the int8-MFMA scan with
    7 base-256 digits;
  * SET_B: three 60-bit data primes + a 60-bit special prime.  Above 2^55: the 64-bit multiply-accumulate scan.

The plain modulus is PlainModulus::Batching(32768, 24) throughout.  Both sets keep well over 100 bits of noise budget
in every reply checked here (printed by the full-reply tests)."""
import numpy as np
import pytest

import oracle
import pir_amd
from gpu_helpers import random_ct, random_key, to_product_params
from oracle.client import Client
from pir_amd import parameters as P
from pir_fixtures import PirSetup, generate_test_db

pytestmark = pytest.mark.gpu

N = 32768
SET_A = oracle.coeff_modulus_create(N, [49, 49, 49, 49, 50])
SET_B = oracle.coeff_modulus_create(N, [60, 60, 60, 60])
SETS = {"A49": SET_A, "B60": SET_B}
ITEMS = {1: 700, 2: 21824, 3: 1364}   # 288-byte items, 341 per plaintext: 3 plaintexts; 64 (9 x 8); 4 (d = 3)


def _server(s, populate=True):
    pp = to_product_params(s.params)
    db = pir_amd.PIRDatabase.Create(pp)
    if populate:
        db.populate(s.raw)
    srv = pir_amd.PIRServer(db, pp)
    srv.set_galois_keys(s.galois_keys)
    return db, srv


_setups = {}


def _setup(name, d):
    key = (name, d)
    if key not in _setups:
        _setups[key] = PirSetup(ITEMS[d], 288, d, N=N, plain_bits=24, moduli=SETS[name])
    return _setups[key]


@pytest.fixture(scope="module", params=sorted(SETS))
def ring(request):
    """d = 1 setup of one modulus set, with its server."""
    s = _setup(request.param, 1)
    db, srv = _server(s)
    yield request.param, s, db, srv
    db.close()


# ---------------------------------------------------------------- NTT

def test_ntt_matches_oracle_and_round_trips(ring):
    name, s, db, srv = ring
    rng = np.random.default_rng(7)
    cts = random_ct(s.orc, rng, 2)
    fwd = srv.ntt_forward(cts)
    assert np.array_equal(fwd, np.stack([s.orc.ct_ntt_fwd(c) for c in cts]))
    assert np.array_equal(srv.ntt_inverse(fwd), cts)
    # key level: every modulus, the special prime included
    kl = np.empty((2, s.orc.k + 1, N), dtype=np.uint64)
    for i in range(s.orc.k + 1):
        kl[:, i, :] = rng.integers(0, s.orc.moduli[i], size=(2, N), dtype=np.uint64)
    fk = srv.ntt_forward(kl, key_level=True)
    for b in range(2):
        for i in range(s.orc.k + 1):
            assert np.array_equal(fk[b, i], s.orc.ntt_fwd(i, kl[b, i])), (b, i)
            assert np.array_equal(s.orc.ntt_inv(i, fk[b, i]), kl[b, i])
    assert np.array_equal(srv.ntt_inverse(fk, key_level=True), kl)
    # the extreme residues: 0 and q - 1 everywhere
    edge = np.zeros_like(cts[:1])
    for j in range(s.orc.k):
        edge[0, 1, j, :] = s.orc.moduli[j] - 1
    assert np.array_equal(srv.ntt_forward(edge)[0], s.orc.ct_ntt_fwd(edge[0]))


# ---------------------------------------------------------------- database encode

def test_db_encode_matches_oracle(ring):
    name, s, db, srv = ring
    assert db.size() == s.params.num_pt == 3
    for i in range(s.params.num_pt):
        assert np.array_equal(db.read_plaintext(i), s.db_ntt[i]), i


# ---------------------------------------------------------------- key switch and expansion

@pytest.mark.parametrize("g", [3, 5, N + 1, 2 * N - 1, N // 2 + 1, 4097])
def test_substitute_matches_oracle(ring, g):
    name, s, db, srv = ring
    rng = np.random.default_rng(g)
    ct = random_ct(s.orc, rng)[0]
    key = random_key(s.orc, rng)
    srv.set_galois_keys({g: key})
    try:
        rc, exp = s.orc.apply_galois_ct(ct, g, key)
        assert rc == 0
        assert np.array_equal(srv.substitute_power_x_inplace(ct.copy(), g), exp)
    finally:
        srv.set_galois_keys(s.galois_keys)


@pytest.fixture(scope="module")
def expander(ring):
    """A context whose expansion workspace holds 4096 selectors (next_power_two(dim_sum)): the d = 1 database of
    `ring` described as one dimension of 4096 (only 3 plaintexts exist; nothing here scans them)."""
    import dataclasses
    name, s, _, _ = ring
    pp = dataclasses.replace(to_product_params(s.params), dimensions=[4096])
    db = pir_amd.PIRDatabase.Create(pp)
    srv = pir_amd.PIRServer(db, pp)
    srv.set_galois_keys(s.galois_keys)
    yield name, s, db, srv
    db.close()


@pytest.mark.parametrize("n", [1, 3, 64])
def test_expansion_matches_oracle(expander, n):
    name, s, db, srv = expander
    ct = s.client.encrypt(np.random.default_rng(n).integers(0, s.params.t, size=N, dtype=np.uint64))
    rc, exp = s.orc.oblivious_expansion(ct, n, s.galois_keys)
    assert rc == 0
    assert np.array_equal(srv.oblivious_expansion(ct, n), exp)


def test_expansion_4096_items_known_answers(expander):
    """4096 outputs (12 levels): too many for the CPU oracle here, so the plaintext-level answer of the reference's
    expansion is checked on a sample: output i encrypts 4096 m_i (mod t) as a constant."""
    name, s, db, srv = expander
    n, t = 4096, s.params.t
    m = np.zeros(N, dtype=np.uint64)                # a query's plaintext: nothing beyond the n selected positions
    m[:n] = np.random.default_rng(4096).integers(0, t, size=n, dtype=np.uint64)
    res = srv.oblivious_expansion(s.client.encrypt(m), n)
    assert res.shape[0] == n
    for i in [0, 1, 2, 1000, 2047, 2048, 4094, 4095] + list(np.random.default_rng(1).integers(0, n, 8)):
        pt = s.client.decrypt(res[i])
        assert pt[0] == (n * int(m[i])) % t and not pt[1:].any(), i
    assert s.client.noise_budget(res[n - 1]) > 0


# ---------------------------------------------------------------- full replies

@pytest.mark.parametrize("name", sorted(SETS))
@pytest.mark.parametrize("d", [1, 2, 3])
def test_full_reply_matches_oracle(name, d):
    s = _setup(name, d)
    p = s.params
    db, srv = _server(s)
    try:
        info = srv.scan_info()
        if d == 2 and name == "A49":   # (d = 3 here: 4 plaintexts, too few rows for the MFMA scan)
            assert info["mfma"] and info["digits"] == 7, info
        if name == "B60":
            assert not info["mfma"], info
        # (the CPU oracle takes seconds per reply at this degree -- up to ~20 at d = 3: fewer indexes at larger d)
        for index in [0, p.num_items - 1, (p.num_items * 5) // 7][:4 - d]:
            q = s.client.create_query_for(p, index)
            rc, exp = s.orc.process_query(s.db_ntt, p.dimensions, q, s.galois_keys)
            assert rc == 0
            got = srv.process_query(q)
            assert got.shape == exp.shape and np.array_equal(got, exp), index
            assert s.client.process_response(p, index, got) == s.item(index)
        budget = s.client.noise_budget(got[0])
        print("N=32768 set %s d=%d: reply noise budget %.1f bits" % (name, d, budget))
        assert budget > 0
    finally:
        db.close()


def test_batch_of_eight_clients():
    """8 queries with 8 different key sets through one staged batch."""
    s = _setup("A49", 2)
    p = s.params
    db, srv = _server(s)
    try:
        # the expansion of one query ciphertext to dim_sum selectors needs the Galois keys of its ceil(log2(dim_sum)) levels
        logm = int(np.ceil(np.log2(sum(p.dimensions))))
        elts = [(N >> j) + 1 for j in range(logm)]
        clients = [Client(s.orc, seed=500 + i) for i in range(8)]
        keys = [c.galois_keys(elts) for c in clients]
        slots = [srv.install_keyset(b"c32k-%d" % i, keys[i]) for i in range(8)]
        idx = [(p.num_items - 1 - 2711 * i) % p.num_items for i in range(8)]
        queries = np.stack([clients[i].create_query_for(p, idx[i]) for i in range(8)])
        srv.set_concurrency(8)
        srv.stage_batch(queries)
        srv.set_batch_keysets(slots)
        srv.run_batch()
        got = srv.fetch_batch()
        for i in range(8):
            if i in (0, 5):   # against the oracle (seconds per reply on the CPU here) ...
                rc, exp = s.orc.process_query(s.db_ntt, p.dimensions, queries[i], keys[i])
                assert rc == 0
                assert np.array_equal(got[i], exp), i
            srv.use_keyset(slots[i])   # ... and every one against the single-query path with that client's key set
            assert np.array_equal(got[i], srv.process_query(queries[i])), i
            assert clients[i].process_response(p, idx[i], got[i]) == s.item(idx[i])
        srv.use_keyset(0)
    finally:
        db.close()


def test_two_slot_shards_in_one_process():
    """The slot-sharded multi-GPU step with G = 2 contexts on one GPU (test_gpu_slots.py's pattern)."""
    import torch
    from gpu_helpers import all_to_all_in_process
    from pir_amd import distributed as D
    s = _setup("A49", 2)
    p = s.params
    pp = to_product_params(p)
    G, per = 2, 1
    cuts = D.slot_cuts(s.orc.k * N, G)
    srvs = []
    for g in range(G):
        db = pir_amd.PIRDatabase.Create(pp, s.raw, slots=(cuts[g], cuts[g + 1]))
        db.finalize(release_staging=True)
        v = pir_amd.PIRServer(db, pp)
        v.set_galois_keys(s.galois_keys)
        v.set_concurrency(16)
        srvs.append(v)
    try:
        assert all(D.slots_exchange_supported(v) for v in srvs)
        indexes = [(p.num_items - 1 - 977 * i) % p.num_items for i in range(G * per)]
        queries = np.stack([s.client.create_query_for(p, i) for i in indexes])
        bufs = [D.SlotsBuffers(srvs[g], G * per, g, G, torch, "cuda:0") for g in range(G)]
        for g in range(G):
            srvs[g].stage_batch(queries)
            srvs[g].slots_expand_async(g * per, per, bufs[g].packed_send.data_ptr(), bufs[g].sv.data_ptr(), cuts)
            srvs[g].sync()
        all_to_all_in_process([b.packed_recv for b in bufs], [b.packed_send for b in bufs], [b.x1_recv for b in bufs],
                              [b.x1_send for b in bufs])
        for g in range(G):
            srvs[g].slots_scan_async(bufs[g].packed_recv.data_ptr(), G, per, bufs[g].rows_send.data_ptr())
            srvs[g].sync()
        all_to_all_in_process([b.rows_recv for b in bufs], [b.rows_send for b in bufs], [b.x2_recv for b in bufs],
                              [b.x2_send for b in bufs])
        for g in range(G):
            srvs[g].slots_finish_async(bufs[g].rows_recv.data_ptr(), per, bufs[g].sv.data_ptr(), cuts,
                                       bufs[g].replies.data_ptr())
            srvs[g].sync()
        for g in range(G):
            mine = bufs[g].replies.cpu().numpy().view(np.uint64)
            for i in range(per):
                rc, want = s.orc.process_query(s.db_ntt, p.dimensions, queries[g * per + i], s.galois_keys)
                assert rc == 0
                assert np.array_equal(mine[i], want), (g, i)
        assert s.client.process_response(p, indexes[0], bufs[0].replies.cpu().numpy().view(np.uint64)[0]) == \
            s.item(indexes[0])
    finally:
        for v in srvs:
            v.db.close()


# ---------------------------------------------------------------- wire path

def test_wire_round_trip_with_seeded_keys():
    """PIRClient (CPU, seed-compressed keys) -> serialized request -> PIRServer.ProcessRequest -> PIRClient, d = 2."""
    enc = P.generate_encryption_params(N, 24, coeff_modulus=SET_A)
    pp = P.create_pir_parameters(3000, 288, 2, enc)
    raw = generate_test_db(3000, 288)
    db = pir_amd.PIRDatabase.Create(pp, raw)
    try:
        server = pir_amd.PIRServer.Create(db, pp)
        client = pir_amd.PIRClient.Create(pp, seed=b"ring32k")
        client.set_seeded_keys(True)
        indexes = [0, 1777, 2999]
        response = server.ProcessRequest(client.CreateRequest(indexes))
        assert client.ProcessResponse(indexes, response) == [raw[i].tobytes() for i in indexes]
        replies = client.LoadResponse(response)
        budget = client.noise_budget(replies[0])
        print("N=32768 wire path d=2: reply noise budget %d bits" % budget)
        assert budget > 0
    finally:
        db.close()


# ---------------------------------------------------------------- limits

def test_generate_encryption_params_needs_an_explicit_modulus():
    with pytest.raises(ValueError, match="8 data primes"):
        P.generate_encryption_params(N, 24)
    assert P.generate_encryption_params(N, 24, coeff_modulus=SET_A).poly_modulus_degree == N


def _create_rc(params_struct):
    import ctypes
    lib = pir_amd.capi.load()
    h = ctypes.c_void_p()
    rc = lib.pirgpu_create(ctypes.byref(params_struct), ctypes.byref(h))
    if rc == 0:
        lib.pirgpu_destroy(h)
    return rc, lib.pirgpu_create_error().decode()


def test_limits_still_refused():
    t = oracle.plain_modulus_batching(N, 24)
    pp = P.create_pir_parameters(100, 64, 1, P.EncryptionParams(N, SET_A, t))
    cp = pir_amd.capi.make_params(pp)
    cp.num_data_primes = 9                                          # k = 9 > PIRGPU_MAX_PRIMES
    rc, msg = _create_rc(cp)
    assert rc == 3 and "primes" in msg, msg
    big = 65536
    enc = P.EncryptionParams(big, oracle.coeff_modulus_create(big, [49, 49, 50]), oracle.plain_modulus_batching(big, 24))
    with pytest.raises(pir_amd.PirGpuError) as e:
        pir_amd.PIRDatabase.Create(P.create_pir_parameters(100, 64, 1, enc))
    assert e.value.code == 3 and "32768" in e.value.message
