"""The ciphertext-multiplication mode on the GPU (PIRGPU_CREATE_CT_MULTIPLY), bit for bit against
the CPU model of tests/ctmult_model.py:

  * pirgpu_ct_multiply on one batch of pairs -- random, zero, q_j - 1, the centring boundary, the magnitude bound, the
    three remainders around the rounding step -- in the default flavour, the integer flavour and at N = 8192 / k = 4;
    pirgpu_relinearize on its outputs with a random key;
  * whole replies against process_query_ct: d = 2 on the 64-bit and the int8-MFMA scan, d = 3, d = 1, a batch of 9 under
    two clients' keys, a database that ends mid-row, a level multiplied in two blocks (the block split at large:
    tests/test_gpu_ctmult_blocks.py; every k, flavour and width of the hooks: tests/test_gpu_ctmult_ladder.py);
  * the wire round trip with the product client on the reference's three d = 2 tuples, seeded and expanded keys;
  * the refusals, and the untouched default.

Every test fails without the feature: the flag and the exports do not exist there."""
import math

import numpy as np
import pytest

import ctmult_model as M
import oracle
import pir_amd
from gpu_helpers import random_key, to_product_params
from oracle.client import Client
from pir_amd import capi
from pir_amd import parameters as P
from pir_amd.server import PirGpuError
from pir_fixtures import PirSetup, generate_test_db

pytestmark = pytest.mark.gpu

CHAIN_8192 = oracle.coeff_modulus_create(8192, [43, 43, 44, 44, 44])


def ct_params(p):
    pp = to_product_params(p)
    pp.use_ciphertext_multiplication = True
    return pp


def ct_server(s, keys=True, ct_scratch_mb=None, **kw):
    pp = ct_params(s.params)
    db = pir_amd.PIRDatabase.Create(pp, ct_multiplication=True, **kw)
    if ct_scratch_mb is not None:
        db.set_option("ct_scratch_mb", ct_scratch_mb)       # (shapes the workspace: before the first use)
    db.populate(s.raw)
    srv = pir_amd.PIRServer(db, pp)
    if keys:
        srv.set_galois_keys(s.galois_keys)
        srv.set_relin_key(s.rk)
    return db, srv


def setup(dbsize, d, N=4096, plain_bits=16, dims=None, moduli=None, bpc=0):
    s = PirSetup(dbsize, 0, d, N=N, plain_bits=plain_bits, moduli=moduli, bits_per_coeff=bpc)
    if dims is not None:
        assert math.prod(dims) >= s.params.num_pt
        s.params.dimensions = list(dims)
    s.rk = M.relin_key(s.client)
    return s


def check_item(client, s, index, got):
    """The reply decrypts to the item: asserted on the reference's own tuples (same setup, same index as
    tests/test_ctmult_model.py, where the model keeps 1.9 and 1.6 bits of budget).  The other shapes here -- full-width
    plaintext coefficients, two nested products -- leave this chain no budget in the model either:
    on them the bits alone are compared."""
    assert client.noise_budget(got[0]) > 0
    assert M.process_response_ct(client, s.params, index, got) == s.item(index)


def expected(s, q, keys=None, rk=None):
    rc, out = M.process_query_ct(s.orc, s.db_ntt, s.params.dimensions, q, keys or s.galois_keys, s.rk if rk is None else rk)
    assert rc == 0
    return out


# ------------------------------------------------------------------------------------------------ the hooks

_HOOK = {}


def hook_case(N, moduli, t_bits):
    """inputs, exact products and relinearised products of one chain, computed once."""
    key = (N, tuple(moduli))
    if key not in _HOOK:
        t = oracle.plain_modulus_batching(N, t_bits)
        orc = oracle.Oracle(N, moduli, t)
        q = [int(x) for x in moduli[:-1]]
        rng = np.random.default_rng(N)
        names, A, B = M.hook_inputs(q, t, N, rng)
        xs = [M.tensor(A[i], B[i], q) for i in range(len(names))]
        M.check_hook_inputs(names, xs, q, t)       # the remainders and the magnitude bound are really reached
        want = np.stack([M.scaled_residues(x, q, t) for x in xs])
        rk = random_key(orc, rng)
        relin = np.stack([M.relinearize(orc, want[i], rk) for i in range(len(names))])
        _HOOK[key] = (t, names, A, B, want, rk, relin)
    return _HOOK[key]


@pytest.mark.parametrize("N,moduli,t_bits,mode", [(4096, oracle.BFV_DEFAULT[4096], 16, None),
                                                  (4096, oracle.BFV_DEFAULT[4096], 16, 0),
                                                  (8192, CHAIN_8192, 42, None)],
                         ids=["4096-default", "4096-integer", "8192-k4"])
def test_multiply_and_relinearize_hooks_match_the_model(monkeypatch, N, moduli, t_bits, mode):
    t, names, A, B, want, rk, relin = hook_case(N, [int(x) for x in moduli], t_bits)
    if mode is not None:
        monkeypatch.setenv("PIRGPU_ALLOW_ENV", "1")
        monkeypatch.setenv("PIRGPU_NTT_MODE", str(mode))
    enc = P.EncryptionParams(N, [int(x) for x in moduli], t)
    pp = P.create_pir_parameters(4, 0, 1, enc, True)
    db = pir_amd.PIRDatabase.Create(pp, ct_multiplication=True)
    if mode is not None:
        assert db.lib.pirgpu_ntt_mode(db.handle) == mode
    got = db.ct_multiply(A, B)
    for i, name in enumerate(names):
        bad = np.argwhere(got[i] != want[i])
        assert bad.size == 0, "%s: first mismatch at [component, residue, coefficient] = %s" % (name, bad[:1].tolist())
    srv = pir_amd.PIRServer(db, pp)
    with pytest.raises(PirGpuError) as e:       # no relinearisation key yet
        db.relinearize(got)
    assert e.value.code == capi.INVALID_ARGUMENT and "RelinKeys" in e.value.message
    srv.set_relin_key(rk)
    out = db.relinearize(got)
    for i, name in enumerate(names):
        assert np.array_equal(out[i], relin[i]), name
    db.close()


# ------------------------------------------------------------------------------------------------ whole replies

_SINGLE = {}


def single_case(dbsize, d):
    """setup, index, query and the model's reply of one single-query shape, computed once (the block tests run the
    d = 2, 100-item case again under a small scratch)."""
    if (dbsize, d) not in _SINGLE:
        # (9 items: the reference's tuple, correctness_test.cpp:99 -- 16-bit t, 10 bits per coefficient, index 5)
        s = setup(dbsize, d, bpc=10 if dbsize == 9 else 0)
        index = 5 if dbsize == 9 else dbsize - 2
        q = s.client.create_query_for(s.params, index)
        _SINGLE[dbsize, d] = (s, index, q, expected(s, q))
    return _SINGLE[dbsize, d]


@pytest.mark.parametrize("dbsize,d,mfma", [(9, 2, 0), (100, 2, 1), (27, 3, 1), (10, 1, 0)])
def test_single_queries_match_the_model(dbsize, d, mfma):
    s, index, q, want = single_case(dbsize, d)
    assert s.params.dimensions == {9: [3, 3], 100: [10, 10], 27: [3, 3, 3], 10: [10]}[dbsize]
    db, srv = ct_server(s, keys=d > 1)
    if d == 1:
        srv.set_galois_keys(s.galois_keys)      # d = 1 needs no relinearisation key
    assert db.reply_ct_count() == 1 and db.reply_ct_words() == 2 * s.orc.k * s.orc.N
    assert srv.scan_info()["mfma"] == mfma
    db.set_option("ct_blocks", 0)
    got = srv.process_query(q)
    assert db.get_option("ct_blocks") == d - 1          # the default scratch holds every level in one block
    assert got.shape == want.shape == (1, 2, s.orc.k, s.orc.N)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first mismatch at [ct, poly, residue, coefficient] = %s" % bad[:1].tolist()
    if d == 1:
        rc, ref = s.orc.process_query(s.db_ntt, s.params.dimensions, q, s.galois_keys)
        assert rc == 0 and np.array_equal(got, ref)
    if dbsize == 9:
        check_item(s.client, s, index, got)
    db.close()


def test_database_ending_mid_row():
    """500 plaintexts in 23 x 22: the last row has 16 columns, the level sums 23 products (database.cpp:196-212 stops at
    the end of the database)."""
    s = setup(500, 2, bpc=6)
    assert s.params.dimensions == [23, 22]
    db, srv = ct_server(s)
    q = s.client.create_query_for(s.params, 125)     # (correctness_test.cpp:100; row 5 of 23, every row is multiplied)
    got = srv.process_query(q)
    assert np.array_equal(got, expected(s, q))
    check_item(s.client, s, 125, got)
    db.close()


_NINE = []


def nine_case():
    """8 x 2 plaintexts, 9 queries alternating two clients' key sets, and the model's reply to each with its own keys:
    (setup, [(client, galois keys, relinearisation key)] * 2, queries [9], replies [9]), computed once."""
    if not _NINE:
        s = setup(16, 2, dims=[8, 2])
        other = Client(s.orc, seed=7)
        clients = [(s.client, s.galois_keys, s.rk), (other, other.galois_keys(), M.relin_key(other))]
        idx = [(5 * i + 3) % 16 for i in range(9)]
        qs = np.stack([clients[i % 2][0].create_query_for(s.params, x) for i, x in enumerate(idx)])
        want = [expected(s, qs[i], clients[i % 2][1], clients[i % 2][2]) for i in range(9)]
        _NINE.append((s, clients, qs, want))
    return _NINE[0]


def run_nine(srv, clients, qs):
    """The batch of nine_case on one server: key sets installed, groups of 8 + 1 on the lanes -> replies [9]."""
    slots = [srv.install_keyset(b"client-%d" % i, keys, relin_key=rk) for i, (_, keys, rk) in enumerate(clients)]
    srv.set_concurrency(8)
    srv.stage_batch(qs)
    srv.set_batch_keysets([slots[i % 2] for i in range(9)])
    srv.run_batch()
    return srv.fetch_batch()


def test_batch_of_nine_under_two_clients_keys():
    """8 x 2 plaintexts (the int8-MFMA scan, groups of 8 + 1 on the lanes): every product of a group is relinearised with
    its own query's key."""
    s, clients, qs, want = nine_case()
    db, srv = ct_server(s)
    assert srv.scan_info()["mfma"] == 1
    out = run_nine(srv, clients, qs)
    assert out.shape == (9, 1, 2, s.orc.k, s.orc.N)
    for i in range(9):
        assert np.array_equal(out[i], want[i]), "query %d of the batch" % i
    assert db.get_option("ct_blocks") == 2              # one block per group: 8 x 8 and 1 x 8 pairs
    db.close()


def test_small_scratch_blocks_give_the_same_bits():
    """ct_scratch_mb = 1 on 10 x 10 plaintexts: the scratch is floored at 8 pairs, so the 10 children of the one upper
    level are multiplied in the blocks {0 .. 7} and {8, 9}, the row's sum carried from the first to the second.  The
    query selects row 9: its product is in the second block, and the reply is right only if the first block's sum
    (the noise of eight products with encryptions of zero) is carried."""
    s, index, q, want = single_case(100, 2)
    assert index // 10 == 9
    db, srv = ct_server(s, ct_scratch_mb=1)
    got = srv.process_query(q)
    assert db.get_option("ct_blocks") == 2
    assert np.array_equal(got, want)
    db.close()


# ------------------------------------------------------------------------------------------------ the wire

@pytest.mark.parametrize("seeded", [True, False], ids=["seeded", "expanded"])
@pytest.mark.parametrize("N,t_bits,dbsize,bpc,indexes", [(4096, 16, 9, 10, [1, 5]), (4096, 16, 500, 6, [9, 125]),
                                                         (8192, 42, 87, 0, [5, 33, 86])])
def test_wire_round_trip_on_the_reference_tuples(N, t_bits, dbsize, bpc, indexes, seeded):
    """correctness_test.cpp:99-101 with product code on both sides: the request carries the RelinKeys, the response one
    ciphertext per query."""
    enc = P.generate_encryption_params(N, t_bits)
    pp = P.create_pir_parameters(dbsize, 0, 2, enc, True, bpc)
    raw = generate_test_db(dbsize, pp.bytes_per_item)
    db = pir_amd.PIRDatabase.Create(pp, raw, ct_multiplication=True)
    server = pir_amd.PIRServer.Create(db, pp)
    client = pir_amd.PIRClient.Create(pp, seed=b"ct-wire")
    client.set_seeded_keys(seeded)
    response = server.ProcessRequest(client.CreateRequest(indexes))
    replies = client.LoadResponse(response)
    assert replies.shape[:2] == (len(indexes), 1)
    assert client.ProcessResponse(indexes, response) == [raw[i].tobytes() for i in indexes]
    # the same client again finds its keys (RelinKeys included) resident; another client gets its own
    before = server.keyset_stats()["key_uploads"]
    assert client.ProcessResponse(indexes[:1], server.ProcessRequest(client.CreateRequest(indexes[:1]))) == [raw[indexes[0]].tobytes()]
    assert server.keyset_stats()["key_uploads"] == before
    db.close()


def strip_field(message, number):
    """A serialized protobuf message without its top-level length-delimited fields `number`."""
    out, i = b"", 0
    while i < len(message):
        start, tag, shift = i, 0, 0
        while True:
            tag |= (message[i] & 0x7F) << shift
            shift += 7
            i += 1
            if not message[i - 1] & 0x80:
                break
        assert tag & 7 == 2
        size, shift = 0, 0
        while True:
            size |= (message[i] & 0x7F) << shift
            shift += 7
            i += 1
            if not message[i - 1] & 0x80:
                break
        i += size
        if tag >> 3 != number:
            out += message[start:i]
    return out


def test_wire_request_without_relin_keys_is_refused():
    enc = P.generate_encryption_params(4096, 16)
    pp = P.create_pir_parameters(9, 0, 2, enc, True, 10)
    plain = P.create_pir_parameters(9, 0, 2, enc, False, 10)
    raw = generate_test_db(9, pp.bytes_per_item)
    db = pir_amd.PIRDatabase.Create(pp, raw, ct_multiplication=True)
    server = pir_amd.PIRServer.Create(db, pp)
    request = strip_field(pir_amd.PIRClient.Create(plain, seed=b"no-relin").CreateRequest([1]), 3)   # Request.relin_keys
    with pytest.raises(PirGpuError) as e:
        server.ProcessRequest(request)
    assert e.value.code == capi.INVALID_ARGUMENT and "RelinKeys" in e.value.message
    db.close()


# ------------------------------------------------------------------------------------------------ statuses

def create_error(pp, **kw):
    with pytest.raises(PirGpuError) as e:
        pir_amd.PIRDatabase.Create(pp, **kw)
    return e.value.code, e.value.message


def test_refusals_at_create():
    enc = P.generate_encryption_params(4096, 16)
    pp = P.create_pir_parameters(100, 0, 2, enc, True)
    code, msg = create_error(pp)                                             # the field without the flag: as before
    assert code == capi.UNIMPLEMENTED and "PIRGPU_CREATE_CT_MULTIPLY" in msg
    code, msg = create_error(P.create_pir_parameters(100, 0, 2, enc, False), ct_multiplication=True)
    assert code == capi.INVALID_ARGUMENT and "use_ciphertext_multiplication" in msg
    for kw, word in [(dict(shard=(0, 5)), "row shard"), (dict(slots=(0, 4096)), "slot shard"), (dict(streamed=True), "STREAMED")]:
        code, msg = create_error(pp, ct_multiplication=True, **kw)
        assert code == capi.INVALID_ARGUMENT and word in msg, (kw, msg)
    for field, value in [("plaintexts_per_item", 2), ("result_primes", 1), ("tables", 2)]:
        bad = P.create_pir_parameters(100, 0, 2, enc, True)
        setattr(bad, field, value)
        code, msg = create_error(bad, ct_multiplication=True)
        assert code == capi.INVALID_ARGUMENT and field in msg, (field, msg)
    big = P.EncryptionParams(32768, oracle.coeff_modulus_create(32768, [49, 49, 50]), oracle.plain_modulus_batching(32768, 20))
    code, msg = create_error(P.create_pir_parameters(100, 0, 2, big, True), ct_multiplication=True)
    assert code == capi.INVALID_ARGUMENT and "32768" in msg
    seven = P.EncryptionParams(4096, oracle.coeff_modulus_create(4096, [40] * 8), 65537)
    code, msg = create_error(P.create_pir_parameters(100, 0, 2, seven, True), ct_multiplication=True)
    assert code == capi.INVALID_ARGUMENT and "6 data primes" in msg
    small = P.EncryptionParams(4096, oracle.coeff_modulus_create(4096, [30, 30, 30]), oracle.plain_modulus_batching(4096, 59))
    code, msg = create_error(P.create_pir_parameters(100, 0, 2, small, True), ct_multiplication=True)
    assert code == capi.INVALID_ARGUMENT and "auxiliary base" in msg


def test_missing_relin_key_and_multi_gpu_entry_points():
    s = setup(9, 2)
    db, srv = ct_server(s, keys=False)
    srv.set_galois_keys(s.galois_keys)
    q = s.client.create_query_for(s.params, 1)
    with pytest.raises(PirGpuError) as e:
        srv.process_query(q)
    assert e.value.code == capi.INVALID_ARGUMENT and "RelinKeys" in e.value.message
    srv.stage_batch(np.stack([q, q]))
    with pytest.raises(PirGpuError) as e:
        srv.run_batch()
    assert e.value.code == capi.INVALID_ARGUMENT and "RelinKeys" in e.value.message
    assert db.lib.pirgpu_reply_copy_to_device(db.handle, None, 1) == capi.FAILED_PRECONDITION
    assert db.lib.pirgpu_reduce_fixup_device(db.handle, None, 1) == capi.FAILED_PRECONDITION
    assert db.lib.pirgpu_batch_reply_copy_to_device(db.handle, None, 1) == capi.FAILED_PRECONDITION
    srv.set_relin_key(s.rk)
    assert np.array_equal(srv.process_query(q), expected(s, q))             # ... and the context still serves
    db.close()
    # the hooks on a context without the flag
    plain = pir_amd.PIRDatabase.Create(to_product_params(s.params))
    with pytest.raises(PirGpuError) as e:
        plain.ct_multiply(q[:1], q[:1])
    assert e.value.code == capi.FAILED_PRECONDITION
    plain.close()


# ------------------------------------------------------------------------------------------------ the untouched default

def test_default_mode_is_untouched_on_the_same_shape():
    """Flag off, 8 x 2 plaintexts: the reply is the oracle's decomposition-mode reply, the batch queues the database
    passes it queued before (two groups: two launches) and the library counts the same database bytes as on the
    ciphertext-multiplication context (the mode adds no database buffer; its scratch exists on its own contexts only)."""
    s = setup(16, 2, dims=[8, 2])
    db = pir_amd.PIRDatabase.Create(to_product_params(s.params))
    db.populate(s.raw)
    srv = pir_amd.PIRServer(db, to_product_params(s.params))
    srv.set_galois_keys(s.galois_keys)
    q = s.client.create_query_for(s.params, 5)
    rc, want = s.orc.process_query(s.db_ntt, s.params.dimensions, q, s.galois_keys)
    assert rc == 0 and np.array_equal(srv.process_query(q), want)
    assert db.reply_ct_count() == 2 * s.orc.expansion_ratio()
    with pytest.raises(PirGpuError) as e:
        db.set_option("no_such_option", 1)
    assert e.value.code == capi.INVALID_ARGUMENT
    srv.set_concurrency(8)
    db.set_option("scan_launches", 0)
    srv.stage_batch(np.stack([q] * 9))
    srv.run_batch()
    out = srv.fetch_batch()
    assert all(np.array_equal(out[i], want) for i in range(9))
    assert db.get_option("scan_launches") == 2
    mem = db.memory()
    ctdb, ctsrv = ct_server(s)
    ctdb.finalize()                     # (the operand layout is packed by the first query, or here)
    got = ctdb.memory()
    assert (got["operand"], got["staging"], got["band"]) == (mem["operand"], mem["staging"], mem["band"])
    db.close()
    ctdb.close()
