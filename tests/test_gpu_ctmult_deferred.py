"""Deferred rounding of the ciphertext-multiplication mode on the GPU (PIRGPU_CREATE_CT_DEFERRED),
bit for bit against the CPU model of tests/ctmult_deferred_model.py:

  1. pirgpu_ct_multiply_sum -- one row of n children through the blocks of the query path: row-sum kernel at Q and at B,
     one scale -- against multiply_ct_sum on five rungs of the ladder (three random pairs and the extremes of the hook's
     family, summed), and with n = 1 against pirgpu_ct_multiply;
  2. the lazy fold of the row-sum kernel at its limit: lazy_limit / 2 + 2 copies of the pair whose every dyadic product is
     the maximal (q - 1)^2, summed by ONE thread per word (a large scratch, no split over workgroups), then split, then in
     blocks of eight with the accumulator carried;
  3. whole replies against process_query_ct_deferred with the counters CT_BLOCKS and CT_RELINS read: one row in one block
     and in two, rows cut by blocks in a group of three at d = 3, nine queries under two clients' keys;
  4. the item recovered on the reference's first tuple, through the model's client and once over the wire;
  5. the refusals.

Every test fails without the feature: the flag, pirgpu_ct_multiply_sum and the option CT_RELINS do not exist there."""
import numpy as np
import pytest

import ctmult_deferred_model as D
import ctmult_model as M
import oracle
import pir_amd
import test_gpu_ctmult as T
from gpu_helpers import chain, to_product_params
from oracle.client import Client
from pir_amd import capi
from pir_amd import parameters as P
from pir_amd.server import PirGpuError
from pir_fixtures import generate_test_db

pytestmark = pytest.mark.gpu


def ct_server(s, keys=True, ct_scratch_mb=None, ct_deferred=True, **kw):
    pp = T.ct_params(s.params)
    db = pir_amd.PIRDatabase.Create(pp, ct_multiplication=True, ct_deferred=ct_deferred, **kw)
    if ct_scratch_mb is not None:
        db.set_option("ct_scratch_mb", ct_scratch_mb)       # (shapes the workspace: before the first use)
    db.populate(s.raw)
    srv = pir_amd.PIRServer(db, pp)
    if keys:
        srv.set_galois_keys(s.galois_keys)
        srv.set_relin_key(s.rk)
    return db, srv


def expected(s, q, keys=None, rk=None):
    rc, out = D.process_query_ct_deferred(s.orc, s.db_ntt, s.params.dimensions, q, keys or s.galois_keys,
                                          s.rk if rk is None else rk)
    assert rc == 0
    return out


def first_mismatch(got, want):
    bad = np.argwhere(got != want)
    return None if bad.size == 0 else bad[0].tolist()


def rung_chain(rung):
    _, N, bits, t_bits = next(c for c in M.LADDER if c[0] == rung)
    moduli = [int(x) for x in chain(N, bits)]
    return N, moduli, oracle.plain_modulus_batching(N, t_bits)


def hook_db(N, moduli, t, **options):
    pp = P.create_pir_parameters(4, 0, 1, P.EncryptionParams(N, moduli, t), True)
    db = pir_amd.PIRDatabase.Create(pp, ct_multiplication=True)      # (the hook works on any context of the mode)
    for name, value in options.items():
        db.set_option(name, value)
    return db, pp


def random_pair(q, N, rng):
    """A random pair with b1 = b0: two big products in the model instead of four."""
    A, B = np.empty((2, len(q), N), dtype=np.uint64), np.empty((2, len(q), N), dtype=np.uint64)
    for j, qj in enumerate(q):
        A[:, j, :] = rng.integers(0, qj, size=(2, N), dtype=np.uint64)
        B[:, j, :] = rng.integers(0, qj, size=N, dtype=np.uint64)
    return A, B


# ------------------------------------------------------------------------------------------------ 1. the hook

SUM_RUNGS = ["k1", "k3-mixed", "k3-wide", "k6-f64", "k6-int"]
_SUM_CASE = {}


def sum_case(rung):
    """chain, inputs and the model's (D0, D1, D2) of one rung's row, computed once (tests/test_gpu_ctmult_shared.py runs
    the same row on the shared-selector path)."""
    if rung not in _SUM_CASE:
        N, moduli, t = rung_chain(rung)
        q = moduli[:-1]
        rng = np.random.default_rng(N + 31 * len(q))
        names, A, B = M.hook_inputs(q, t, N, rng, names=M.SUB_FAMILY)       # one random pair and the extremes
        extra = [random_pair(q, N, rng) for _ in range(2)]
        A = np.concatenate([A, np.stack([e[0] for e in extra])])
        B = np.concatenate([B, np.stack([e[1] for e in extra])])
        n = A.shape[0]
        assert n == len(M.SUB_FAMILY) + 2 and D.plan_terms(N, q, moduli[-1], t, n)[1]
        want = D.multiply_ct_sum(A, B, q, t)
        for x in (A, B, want):
            x.setflags(write=False)
        _SUM_CASE[rung] = (N, moduli, t, names, A, B, want)
    return _SUM_CASE[rung]


@pytest.mark.parametrize("rung", SUM_RUNGS)
def test_sum_hook_matches_the_model(rung):
    N, moduli, t, names, A, B, want = sum_case(rung)
    q = moduli[:-1]
    db, _ = hook_db(N, moduli, t)
    got = db.ct_multiply_sum(A, B)
    assert got.shape == want.shape == (3, len(q), N)
    assert first_mismatch(got, want) is None, "first mismatch at [component, residue, coefficient] = %s" % first_mismatch(got, want)
    for i in (0, names.index("full h")):                                # a row of one child: the per-child product
        assert np.array_equal(db.ct_multiply_sum(A[i:i + 1], B[i:i + 1]), db.ct_multiply(A[i:i + 1], B[i:i + 1])[0]), names[i]
    db.close()


# ------------------------------------------------------------------------------------------------ 2. the lazy fold

def test_lazy_fold_at_its_limit():
    """k6-int, 60-bit primes.  The pair whose four polynomials are the constant -1 (residue q_j - 1 in coefficient 0) has
    the NTT form q - 1 at every slot of Q and b_i - 1 at every slot of B: every dyadic product is the maximal (q - 1)^2,
    and x1 takes two per child.  n = lazy_limit / 2 + 2 such children give x1 lazy_limit + 4 products: 260 (q - 1)^2 >
    2^128 for primes just below 2^60, so a sum that is not folded after lazy_limit PRODUCTS wraps.  Two random pairs are
    added so that the result is no constant.  Model: X = n (1, 2, 1) as constant polynomials + the two random tensors.

    First with a scratch that holds the whole row in one block and the split over workgroups off: one thread sums all the
    children of a word, the case the fold is there for.  Then as the library chooses (default scratch: three blocks, each
    split), and with ct_scratch_mb = 1: blocks of eight children, the accumulators carried sixteen times.

    (The wrap this row would cause is the same 2^128 at every modulus of Q and B, which these six 60-bit primes round
    away: a fold that comes too late is caught by test_lazy_fold_when_one_modulus_alone_would_wrap[four-polynomial] of
    tests/test_gpu_ctmult_shared.py, not here.)"""
    N, moduli, t = rung_chain("k6-int")
    q = moduli[:-1]
    k = len(q)
    rng = np.random.default_rng(60)
    db, pp = hook_db(N, moduli, t, ct_scratch_mb=1024, ct_rowsum_splits=1)
    lazy = pir_amd.PIRServer(db, pp).arith_info()["lazy_limit"]
    assert lazy == 1 << (128 - 2 * 60)
    n = lazy // 2 + 2
    assert (lazy + 4) * (min(q) - 1) ** 2 >= 1 << 128          # x1 unfolded does wrap
    minus_one = np.zeros((2, k, N), dtype=np.uint64)
    for j, qj in enumerate(q):
        minus_one[:, j, 0] = qj - 1
    extra = [random_pair(q, N, rng) for _ in range(2)]
    A = np.stack([minus_one] * n + [e[0] for e in extra])
    B = np.stack([minus_one] * n + [e[1] for e in extra])
    assert D.plan_terms(N, q, moduli[-1], t, n + 2)[1]
    X = [list(x) for x in D.tensor_sum(A[n:], B[n:], q)]
    for m, c in enumerate((1, 2, 1)):
        X[m][0] += n * c
    assert M.tensor(minus_one, minus_one, q)[1][:2] == [2, 0]
    want = M.scaled_residues(X, q, t)
    got = db.ct_multiply_sum(A, B)
    assert first_mismatch(got, want) is None, "one thread per word: first mismatch at %s" % first_mismatch(got, want)
    db.close()
    for options in ({}, {"ct_scratch_mb": 1}):
        db, _ = hook_db(N, moduli, t, **options)
        again = db.ct_multiply_sum(A, B)
        assert first_mismatch(again, want) is None, "%s: first mismatch at %s" % (options, first_mismatch(again, want))
        db.close()


# ------------------------------------------------------------------------------------------------ 3. whole replies

_WANT = {}


def single_deferred(dbsize):
    """T.single_case's setup, index and query with the deferred model's reply, computed once."""
    if dbsize not in _WANT:
        s, index, q, per_child = T.single_case(dbsize, 2)
        _WANT[dbsize] = (s, index, q, expected(s, q), per_child)
    return _WANT[dbsize]


def counters(db):
    return db.get_option("ct_blocks"), db.get_option("ct_relins")


def test_one_row_in_one_block_and_in_two():
    """d = 2, 10 x 10 plaintexts, one query for an item of row 9.  Default scratch: one block, one key switch.
    ct_scratch_mb = 1 (8 pairs): blocks {0 .. 7} and {8, 9}, the NTT-domain accumulators at Q and at B carried from the
    first to the second, still one key switch.  The per-child form switches ten ciphertexts on the same query."""
    s, index, q, want, per_child = single_deferred(100)
    assert s.params.dimensions == [10, 10] and index // 10 == 9
    assert not np.array_equal(want, per_child)
    replies = []
    for mb, blocks in ((None, 1), (1, 2)):
        db, srv = ct_server(s, ct_scratch_mb=mb)
        assert db.reply_ct_count() == 1
        got = srv.process_query(q)
        assert counters(db) == (blocks, 1), mb
        assert first_mismatch(got, want) is None, "scratch %s: first mismatch at %s" % (mb, first_mismatch(got, want))
        replies.append(got)
        db.close()
    assert np.array_equal(replies[0], replies[1])
    db, srv = ct_server(s, ct_deferred=False)
    assert np.array_equal(srv.process_query(q), per_child)
    assert counters(db) == (1, 10)
    db.set_option("ct_relins", 0)
    assert db.get_option("ct_relins") == 0
    db.close()


def test_rows_cut_by_blocks_in_a_group_of_three():
    """The shape of tests/test_gpu_ctmult_blocks.py: d = 3, dims [3, 3, 2], 15 plaintexts at N = 2048 on two 27-bit primes,
    a group of 3 queries, ct_scratch_mb = 1 (8 pairs, bj = 2).  Level 1 has 8 children in rows of 3:

      {0, 1} row 0, cut | {2, 3} row 0 carried and finished, row 1 begun behind it and moved to the front | {4, 5} row 1
      carried and finished, rows 0 and 2 untouched | {6, 7} the short last row, which ends with the database

    and level 0 three children in {0, 1} | {2}.  Key switches: 3 rows x 3 queries + 1 row x 3 queries = 12."""
    N = 2048
    s = T.setup(15, 3, N=N, moduli=[int(x) for x in chain(N, 27)])
    assert s.params.dimensions == [3, 3, 2] and s.params.num_pt == 15
    idx = [14, 7, 3]
    qs = np.stack([s.client.create_query_for(s.params, i) for i in idx])
    want = [expected(s, q) for q in qs]
    replies = []
    for mb, blocks in ((1, 6), (None, 2)):
        db, srv = ct_server(s, ct_scratch_mb=mb)
        assert srv.scan_info()["mfma"] == 1
        srv.set_concurrency(8)
        srv.stage_batch(qs)
        srv.run_batch()
        out = srv.fetch_batch()
        assert counters(db) == (blocks, 12), mb
        assert out.shape == (3, 1, 2, s.orc.k, N)
        for i in range(3):
            assert first_mismatch(out[i], want[i]) is None, "scratch %s, query %d: first mismatch at %s" % (
                mb, i, first_mismatch(out[i], want[i]))
        replies.append(out)
        db.close()
    assert np.array_equal(replies[0], replies[1])


def test_batch_of_nine_under_two_clients_keys():
    """8 x 2 plaintexts, nine queries alternating two clients' key sets, groups of 8 + 1 on the lanes: the finished rows
    are ordered row-major, query-minor, so every query's row is relinearised with its own key.  Nine key switches."""
    s = T.setup(16, 2, dims=[8, 2])
    other = Client(s.orc, seed=7)
    clients = [(s.client, s.galois_keys, s.rk), (other, other.galois_keys(), M.relin_key(other))]
    idx = [(5 * i + 3) % 16 for i in range(9)]
    qs = np.stack([clients[i % 2][0].create_query_for(s.params, x) for i, x in enumerate(idx)])
    db, srv = ct_server(s)
    assert srv.scan_info()["mfma"] == 1
    out = T.run_nine(srv, clients, qs)
    assert out.shape == (9, 1, 2, s.orc.k, s.orc.N)
    assert counters(db) == (2, 9)
    for i in range(9):
        want = expected(s, qs[i], clients[i % 2][1], clients[i % 2][2])
        assert first_mismatch(out[i], want) is None, "query %d of the batch: first mismatch at %s" % (
            i, first_mismatch(out[i], want))
    db.close()


# ------------------------------------------------------------------------------------------------ 4. round trips

def test_reference_tuple_recovers_the_item():
    """correctness_test.cpp:99 (9 items, 16-bit t, 10 bits per coefficient, index 5) on a deferred context."""
    s, index, q, want, _ = single_deferred(9)
    db, srv = ct_server(s)
    got = srv.process_query(q)
    assert np.array_equal(got, want)
    T.check_item(s.client, s, index, got)
    db.close()


def test_wire_round_trip_on_the_reference_tuple():
    enc = P.generate_encryption_params(4096, 16)
    pp = P.create_pir_parameters(9, 0, 2, enc, True, 10)
    raw = generate_test_db(9, pp.bytes_per_item)
    db = pir_amd.PIRDatabase.Create(pp, raw, ct_multiplication=True, ct_deferred=True)
    server = pir_amd.PIRServer.Create(db, pp)
    client = pir_amd.PIRClient.Create(pp, seed=b"ct-deferred-wire")
    indexes = [1, 5]
    db.set_option("ct_relins", 0)
    response = server.ProcessRequest(client.CreateRequest(indexes))
    assert db.get_option("ct_relins") == len(indexes)
    assert client.LoadResponse(response).shape[:2] == (len(indexes), 1)
    assert client.ProcessResponse(indexes, response) == [raw[i].tobytes() for i in indexes]
    db.close()


# ------------------------------------------------------------------------------------------------ 5. refusals

def test_refusals_at_create():
    enc = P.generate_encryption_params(4096, 16)
    pp = P.create_pir_parameters(100, 0, 2, enc, True)
    code, msg = T.create_error(pp, ct_deferred=True)                        # the flag without the mode's flag
    assert code == capi.INVALID_ARGUMENT and "PIRGPU_CREATE_CT_MULTIPLY" in msg and "PIRGPU_CREATE_CT_DEFERRED" in msg
    both = dict(ct_multiplication=True, ct_deferred=True)
    for kw, word in [(dict(shard=(0, 5)), "row shard"), (dict(slots=(0, 4096)), "slot shard"), (dict(streamed=True), "STREAMED")]:
        code, msg = T.create_error(pp, **both, **kw)
        assert code == capi.INVALID_ARGUMENT and word in msg, (kw, msg)
    for field, value in [("plaintexts_per_item", 2), ("result_primes", 1), ("tables", 2)]:
        bad = P.create_pir_parameters(100, 0, 2, enc, True)
        setattr(bad, field, value)
        code, msg = T.create_error(bad, **both)
        assert code == capi.INVALID_ARGUMENT and field in msg, (field, msg)
    big = P.EncryptionParams(32768, oracle.coeff_modulus_create(32768, [49, 49, 50]), oracle.plain_modulus_batching(32768, 20))
    code, msg = T.create_error(P.create_pir_parameters(100, 0, 2, big, True), **both)
    assert code == capi.INVALID_ARGUMENT and "32768" in msg
    # k2-tight: the auxiliary base holds one product at this plain modulus, not a row of ten
    _, N, bits, t_bits = next(c for c in M.LADDER if c[0] == "k2-tight")
    tight = P.EncryptionParams(N, [int(x) for x in chain(N, bits)], oracle.plain_modulus_batching(N, t_bits))
    tp = P.create_pir_parameters(100, 0, 2, tight, True)
    assert not D.plan_terms(N, tight.coeff_modulus[:-1], tight.coeff_modulus[-1], tight.plain_modulus, tp.dimensions[0])[1]
    code, msg = T.create_error(tp, **both)
    assert code == capi.INVALID_ARGUMENT and "PIRGPU_CREATE_CT_DEFERRED" in msg and "auxiliary base" in msg
    pir_amd.PIRDatabase.Create(tp, ct_multiplication=True).close()          # ... which the per-child form serves


def test_sum_hook_refusals():
    s = T.setup(9, 2)
    q = s.client.create_query_for(s.params, 1)
    plain = pir_amd.PIRDatabase.Create(to_product_params(s.params))
    with pytest.raises(PirGpuError) as e:
        plain.ct_multiply_sum(q[:1], q[:1])
    assert e.value.code == capi.FAILED_PRECONDITION
    plain.close()
    # the hook checks the bound for its own n: k2-tight holds one product
    N, moduli, t = rung_chain("k2-tight")
    db, _ = hook_db(N, moduli, t)
    pair = np.zeros((8, 2, 2, N), dtype=np.uint64)
    assert not D.plan_terms(N, moduli[:-1], moduli[-1], t, 8)[1]
    with pytest.raises(PirGpuError) as e:
        db.ct_multiply_sum(pair, pair)
    assert e.value.code == capi.INVALID_ARGUMENT and "auxiliary base" in e.value.message
    assert not db.ct_multiply_sum(pair[:1], pair[:1]).any()
    db.close()
