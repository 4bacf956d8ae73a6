"""Modulus-switched results on the GPU (pirgpu_params.result_primes), bit for bit against the CPU
model of tests/modswitch_model.py:

  * pirgpu_mod_switch (the launcher of the query path) on random and boundary residues, every ring degree and chain
    shape the kernel meets: 36-bit, 60-bit (width of the integer products), k = 3 and k = 4 (several drop steps),
    N = 32768;
  * whole replies against process_query_switched: int8-MFMA and 64-bit scans, fused / split / integer upper levels,
    d = 1 (reply switch only), d = 3 (the intermediate switch runs twice), batches under two key sets, wide items, a
    streamed database;
  * the wire round trip with the product client; result_primes = 0 as the control; the refusals.

Every test but the control fails without the feature: the field and the exports do not exist there."""
import math

import numpy as np
import pytest

import modswitch_model as M
import oracle
import pir_amd
from gpu_helpers import to_product_params
from oracle.client import Client
from pir_amd import capi
from pir_amd import parameters as P
from pir_amd.server import PirGpuError
from pir_fixtures import PirSetup, generate_test_db

pytestmark = pytest.mark.gpu

CHAINS = {
    "4096/36": (4096, list(oracle.BFV_DEFAULT[4096])),                                   # [36, 36] + 37
    "4096/60": (4096, oracle.coeff_modulus_create(4096, [60, 60, 60])),
    "8192/43": (8192, oracle.coeff_modulus_create(8192, [43, 43, 44, 44])),              # cfg 4's chain
    "16384/48": (16384, oracle.coeff_modulus_create(16384, [48, 48, 48, 49, 49])),       # cfg 5's chain
    "32768/49": (32768, oracle.coeff_modulus_create(32768, [49, 49, 50])),
}


def product_params(s, r):
    pp = to_product_params(s.params)
    pp.result_primes = r
    return pp


def server(s, r, **kw):
    pp = product_params(s, r)
    db = pir_amd.PIRDatabase.Create(pp, **kw)
    db.populate(s.raw)
    srv = pir_amd.PIRServer(db, pp)
    srv.set_galois_keys(s.galois_keys)
    return db, srv


def check_shape(db, s, r, d, planes=1):
    e = M.expansion_ratio_level(s.orc, r)
    assert db.expansion_ratio() == e
    assert db.reply_ct_count() == planes * (2 * e) ** (d - 1)
    assert db.reply_ct_words() == 2 * r * s.orc.N


# ------------------------------------------------------------------------------------------------ the kernel alone

@pytest.mark.parametrize("name,r", [("4096/36", 1), ("4096/60", 1), ("8192/43", 1), ("8192/43", 2), ("16384/48", 1),
                                    ("16384/48", 2), ("16384/48", 3), ("32768/49", 1)])
def test_mod_switch_hook_matches_the_model(name, r):
    N, moduli = CHAINS[name]
    q = [int(x) for x in moduli[:-1]]
    enc = P.EncryptionParams(N, [int(x) for x in moduli], oracle.plain_modulus_batching(N, 20))
    db = pir_amd.PIRDatabase.Create(P.create_pir_parameters(4, 0, 1, enc))        # (its own result_primes is 0)
    cts = M.switch_inputs(q, N, np.random.default_rng(N + r))
    got = db.mod_switch(cts, r)
    want = M.switch_residues(cts, q, r)
    assert got.shape == want.shape == (4, 2, r, N)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first mismatch at [ct, poly, residue, coefficient] = %s" % bad[:1].tolist()
    with pytest.raises(PirGpuError) as e:
        db.mod_switch(cts, len(q))
    assert e.value.code == capi.INVALID_ARGUMENT
    with pytest.raises(PirGpuError):
        db.mod_switch(cts, 0)
    db.close()


# ------------------------------------------------------------------------------------------------ whole replies

def expected(s, query, r, keys=None):
    return M.process_query_switched(s.orc, s.db_ntt, s.params.dimensions, query, keys or s.galois_keys, r)


def setup(name, dbsize, d, dims=None, plain_bits=24, **kw):
    N, moduli = CHAINS[name]
    s = PirSetup(dbsize, 0, d, N=N, plain_bits=plain_bits, moduli=moduli, **kw)
    if dims is not None:
        assert math.prod(dims) >= s.params.num_pt
        s.params.dimensions = list(dims)
    return s


def test_d2_single_query_and_batch_under_two_key_sets():
    """10 x 10 plaintexts at N = 4096, r = 1: the int8-MFMA scan and the fused upper level; a batch of 9 (a group of 8
    and a group of 1) whose queries alternate between two clients' key sets."""
    s = setup("4096/36", 100, 2)
    p = s.params
    assert p.dimensions == [10, 10]
    db, srv = server(s, 1)
    check_shape(db, s, 1, 2)
    assert srv.scan_info()["mfma"] == 1
    q = s.client.create_query_for(p, 98)
    want = expected(s, q, 1)
    got = srv.process_query(q)
    assert got.shape == want.shape == (4, 2, 1, 4096) and np.array_equal(got, want)
    assert np.array_equal(M.process_reply_level(s.client, 2, got, 1), M.process_reply_level(s.client, 2, want, 1))
    other = Client(s.orc, seed=7)
    clients = [(s.client, s.galois_keys), (other, other.galois_keys())]
    slots = [srv.install_keyset(b"client-%d" % i, keys) for i, (_, keys) in enumerate(clients)]
    idx = [(11 * i + 3) % 100 for i in range(9)]
    qs = np.stack([clients[i % 2][0].create_query_for(p, x) for i, x in enumerate(idx)])
    srv.set_concurrency(8)
    srv.stage_batch(qs)
    srv.set_batch_keysets([slots[i % 2] for i in range(9)])
    srv.run_batch()
    out = srv.fetch_batch()
    assert out.shape == (9, 4, 2, 1, 4096)
    for i in range(9):
        assert np.array_equal(out[i], expected(s, qs[i], 1, clients[i % 2][1])), "query %d of the batch" % i
    db.close()


@pytest.mark.parametrize("dbsize,d", [(9, 2), (9, 1)])
def test_small_shapes_64_bit_scan_and_d1(dbsize, d):
    """3 x 3 plaintexts (fewer than 8 rows: the 64-bit scan kernels) and d = 1 with 9 plaintexts (only the reply is
    switched: the scan's sums are level 0)."""
    s = setup("4096/36", dbsize, d)
    db, srv = server(s, 1)
    check_shape(db, s, 1, d)
    assert srv.scan_info()["mfma"] == 0
    for index in (0, dbsize - 2):
        q = s.client.create_query_for(s.params, index)
        assert np.array_equal(srv.process_query(q), expected(s, q, 1))
    # the batch pipeline's path for contexts without the int8 scan
    qs = np.stack([s.client.create_query_for(s.params, i) for i in (1, 5, 8)])
    out = srv.process_batch(qs, n_workers=4)
    for i in range(3):
        assert np.array_equal(out[i], expected(s, qs[i], 1))
    db.close()


@pytest.mark.parametrize("r", [2, 1])
def test_d3_switches_the_intermediate_level_twice(r):
    s = setup("8192/43", 27, 3, plain_bits=20)
    assert s.params.dimensions == [3, 3, 3] and s.orc.k == 3
    db, srv = server(s, r)
    check_shape(db, s, r, 3)
    q = s.client.create_query_for(s.params, 14)
    want = expected(s, q, r)
    got = srv.process_query(q)
    assert got.shape == want.shape and np.array_equal(got, want)
    db.close()


@pytest.mark.parametrize("name,r", [("16384/48", 2), ("32768/49", 1)])
def test_large_rings_split_and_integer_upper_level(name, r):
    """8 x 2 plaintexts: N = 16384 takes the split upper level (transform to scratch + multiply-accumulate), N = 32768
    its integer form; single query and a group of 3."""
    s = setup(name, 16, 2, dims=[8, 2])
    db, srv = server(s, r)
    check_shape(db, s, r, 2)
    q = s.client.create_query_for(s.params, 13)
    want = expected(s, q, r)
    got = srv.process_query(q)
    assert got.shape == want.shape and np.array_equal(got, want)
    qs = np.stack([q, s.client.create_query_for(s.params, 2), q])
    out = srv.process_batch(qs, n_workers=8)
    assert np.array_equal(out[0], want) and np.array_equal(out[2], want)
    assert np.array_equal(out[1], expected(s, qs[1], r))
    db.close()


def test_wide_items_switch_every_plane():
    """Two planes at N = 4096, r = 1: plane j's part of the reply is the switched reply of plane j's own database."""
    N, moduli = CHAINS["4096/36"]
    t = oracle.plain_modulus_batching(N, 24)
    enc = P.EncryptionParams(N, list(moduli), t)
    n = 100
    op = oracle.create_pir_parameters(n, 0, 2, N=N, plain_bits=24, moduli=list(moduli), t=t)
    B = op.bytes_per_item
    pp = P.create_pir_parameters(n, B + 1000, 2, enc, max_plaintexts_per_item=2, result_primes=1)
    assert pp.planes == 2 and list(pp.dimensions) == list(op.dimensions) == [10, 10]
    raw = generate_test_db(n, B + 1000, seed=3)
    orc = oracle.Oracle.from_params(op)
    client = Client(orc, seed=21)
    keys = client.galois_keys()
    db = pir_amd.PIRDatabase.Create(pp, raw)
    srv = pir_amd.PIRServer(db, pp)
    srv.set_galois_keys(keys)
    assert db.reply_ct_count() == 2 * 4 and db.reply_ct_words() == 2 * N and db.expansion_ratio() == 2
    q = client.create_query_for(op, 57)
    got = srv.process_query(q)
    assert got.shape == (8, 2, 1, N)
    rc, sv = orc.oblivious_expansion_multi(q, op.dim_sum, keys)
    assert rc == 0
    for j in range(2):
        chunk = np.ascontiguousarray(raw[:, j * B:(j + 1) * B])
        rc, plane = orc.db_encode(chunk.tobytes(), n, chunk.shape[1], 1, op.eff_bits_per_coeff, n)
        assert rc == 0
        assert np.array_equal(got[4 * j:4 * j + 4], M.multiply_switched(orc, plane, op.dimensions, sv, 1)), "plane %d" % j
    db.close()


def test_streamed_database_serves_switched_replies():
    s = setup("4096/36", 100, 2)
    db, srv = server(s, 1, streamed=True)
    check_shape(db, s, 1, 2)
    q = s.client.create_query_for(s.params, 42)
    assert np.array_equal(srv.process_query(q), expected(s, q, 1))
    db.close()


# ------------------------------------------------------------------------------------------------ wire round trip

def test_wire_round_trip_with_the_product_client():
    """pirgpu_process_request -> pirclient_process_response: a lone request and a window of 9 queries (d = 2, 10 x 10
    plaintexts, N = 4096, 20-bit t, r = 1 -- tests/test_modswitch_model.py checks the noise these parameters leave)."""
    N = 4096
    enc = P.generate_encryption_params(N, 20)
    pp = P.create_pir_parameters(100, 0, 2, enc, result_primes=1)
    raw = generate_test_db(100, pp.bytes_per_item, seed=8)
    db = pir_amd.PIRDatabase.Create(pp, raw)
    srv = pir_amd.PIRServer.Create(db, pp)
    client = pir_amd.PIRClient.Create(pp, seed=b"modswitch-rt")
    e = db.expansion_ratio()
    assert e == 2 and client.reply_ct_count == db.reply_ct_count() == 4
    payload = (2 * e) * 2 * 1 * N * 8                                 # E'^(d-1) ciphertexts of 2 r N words
    for indexes in ([98], [(11 * i + 3) % 100 for i in range(9)]):
        response = srv.ProcessRequest(client.CreateRequest(indexes))
        assert client.ProcessResponse(indexes, response) == [raw[i].tobytes() for i in indexes]
        extra = len(response) - len(indexes) * payload                 # SEAL headers, parms_id, protobuf framing
        assert 0 < extra <= len(indexes) * (2 * e * 160 + 16)
        replies = client.LoadResponse(response)
        assert replies.shape == (len(indexes), 4, 2, 1, N)
        assert client.noise_budget_level(replies[0, 0], 1) >= 2
    db.close()


# ------------------------------------------------------------------------------------------------ off and refused

def test_result_primes_zero_is_the_reference_path():
    """The control: with the field at 0 the reply is the oracle's processQuery, at the full modulus."""
    s = setup("4096/36", 100, 2)
    db, srv = server(s, 0)
    assert db.reply_ct_words() == 2 * 2 * 4096 and db.expansion_ratio() == s.orc.expansion_ratio()
    q = s.client.create_query_for(s.params, 98)
    rc, want = s.orc.process_query(s.db_ntt, s.params.dimensions, q, s.galois_keys)
    assert rc == 0 and np.array_equal(srv.process_query(q), want)
    db.close()


def test_create_refuses_what_cannot_be_switched():
    s = setup("4096/36", 100, 2)
    for r, kw in [(2, {}), (3, {}), (1, {"shard": (0, 5)}), (1, {"slots": (0, 4096)})]:
        with pytest.raises(PirGpuError) as e:
            pir_amd.PIRDatabase.Create(product_params(s, r), **kw)
        assert e.value.code == capi.INVALID_ARGUMENT, (r, kw)
    one = PirSetup(9, 0, 1, N=4096, plain_bits=20, moduli=oracle.coeff_modulus_create(4096, [54, 55]))   # k = 1
    with pytest.raises(PirGpuError) as e:
        pir_amd.PIRDatabase.Create(product_params(one, 1))
    assert e.value.code == capi.INVALID_ARGUMENT


def test_multi_gpu_entry_points_refuse_a_switched_context():
    s = setup("4096/36", 100, 2)
    db, srv = server(s, 1)
    lib, h = db.lib, db.handle
    calls = {
        "batch_expand_packed": lambda: lib.pirgpu_batch_expand_packed(h, 0, 0, None, None, None, 0),
        "batch_expand_packed_async": lambda: lib.pirgpu_batch_expand_packed_async(h, 0, 0, None, None, None, 0),
        "batch_run_packed": lambda: lib.pirgpu_batch_run_packed(h, None, 0, 0, None),
        "slots_expand_async": lambda: lib.pirgpu_slots_expand_async(h, 0, 0, None, None, None, 0, None, None),
        "slots_scan_async": lambda: lib.pirgpu_slots_scan_async(h, None, 0, 0, None, None, None),
        "slots_finish_async": lambda: lib.pirgpu_slots_finish_async(h, None, 0, None, None, 0, None, None, None),
        "reduce_fixup_device": lambda: lib.pirgpu_reduce_fixup_device(h, None, 0),
        "reduce_fixup_device_async": lambda: lib.pirgpu_reduce_fixup_device_async(h, None, 0, None),
        "reply_copy_to_device": lambda: lib.pirgpu_reply_copy_to_device(h, None, 0),
        "batch_reply_copy_to_device": lambda: lib.pirgpu_batch_reply_copy_to_device(h, None, 0),
        "batch_reply_copy_to_device_async": lambda: lib.pirgpu_batch_reply_copy_to_device_async(h, None, 0),
    }
    for name, call in calls.items():
        assert call() == capi.FAILED_PRECONDITION, name
        assert b"result_primes" in lib.pirgpu_last_error(h), name
    db.close()
