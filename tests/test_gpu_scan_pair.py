"""The paired database pass (pir_amd/csrc/scan_mfma_pair.hip, PIRGPU_SCAN_MFMA_PAIR): two groups of up to 8 queries per
database read, the second group's selector tiles in LDS.  Every reply is compared bit for bit with the CPU oracle;
SCAN_LAUNCHES proves which launches a batch took (a pair counts one).

Shapes, N = 4096 (36-bit primes: 5 digits):
  [17, 18]   1 k-step, a last row tile of one row, a quarter-full k-step
  [18, 70]   2 k-steps, 5 column groups: a partial last k-step
  [33, 130]  3 k-steps, 9 column groups, three row tiles
Batches with 16 workers (two lanes of 8): 9 and 15 (a second group of 1 and of 7), 16, 17 (a pair, then a lone group on
the single kernel), 24 (a pair on one lane, a single on the other), 3 (no pair)."""
import functools

import numpy as np
import pytest

import pir_amd
import scan_fold_model as M
from gpu_helpers import device_to_seal_order, to_product_params
from oracle.client import Client
from test_gpu_mfma_scan import setup_with_dims
from test_gpu_scan_worst_case import N, ROWS, case_of, context

pytestmark = pytest.mark.gpu

SHAPES = {"17x18": ([17, 18], 1), "18x70": ([18, 70], 2), "33x130": ([33, 130], 3)}
# batch -> database-pass launches with pairing / without: groups of 8 over two lanes
LAUNCHES = {9: (1, 2), 15: (1, 2), 16: (1, 2), 17: (2, 3), 24: (2, 3), 3: (1, 1)}
NQ = 24
PAIR = "PIRGPU_SCAN_MFMA_PAIR"      # read when a context builds its workspace (conftest.py opens PIRGPU_ALLOW_ENV)
DISTINCT = 12


@functools.lru_cache(maxsize=None)
def shape_case(name):
    """Setup, 24 queries and their expected replies for one shape: computed once, shared by every variant."""
    dims, _ = SHAPES[name]
    s = setup_with_dims(2, 2048, dims, N=4096, plain_bits=24)
    n = s.params.num_items
    # 12 distinct queries, position i of a batch holds query i mod 12: the 8 queries of a group are distinct, and so are
    # the two queries at the same place of the two groups of a pair (the oracle's replies are the slow part of this file)
    idx = [(97 * i + 13) % n for i in range(DISTINCT - 2)] + [0, n - 1]
    distinct = [s.client.create_query_for(s.params, i) for i in idx]
    replies = []
    for q in distinct:
        rc, exp = s.orc.process_query(s.db_ntt, s.params.dimensions, q, s.galois_keys)
        assert rc == 0
        replies.append(exp)
    queries = np.stack([distinct[i % DISTINCT] for i in range(NQ)])
    expected = [replies[i % DISTINCT] for i in range(NQ)]
    queries.setflags(write=False)
    return s, queries, expected


def make(s, **options):
    pp = to_product_params(s.params)
    db = pir_amd.PIRDatabase.Create(pp)
    for name, value in options.items():
        db.set_option(name, value)
    db.populate(s.raw)
    srv = pir_amd.PIRServer(db, pp)
    srv.set_galois_keys(s.galois_keys)
    return db, srv


@pytest.mark.parametrize("fold", [1, 0], ids=["fp64 fold", "integer fold"])
@pytest.mark.parametrize("top4", [1, 0], ids=["top digit nibble", "top digit byte"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_paired_pass_matches_the_oracle(shape, top4, fold, monkeypatch):
    monkeypatch.setenv(PAIR, "2")
    s, queries, expected = shape_case(shape)
    db, srv = make(s, scan_mfma_top4=top4, scan_f64_fold_batch=fold, scan_f64_fold=0)
    info = srv.scan_info()
    assert info["mfma"] and info["digits"] == 5 and info["chunks"] == 1 and info["ksteps"] == SHAPES[shape][1], info
    assert info["top_digit_nibble"] == bool(top4) and srv.arith_info()["scan_f64_fold_batch"] == bool(fold)
    for count, (paired, _) in LAUNCHES.items():
        before = db.get_option("SCAN_LAUNCHES")
        got = srv.process_batch(queries[:count].copy(), n_workers=16)
        assert db.get_option("SCAN_LAUNCHES") - before == paired, (count, db.get_option("SCAN_LAUNCHES") - before)
        for i in range(count):
            assert np.array_equal(got[i], expected[i]), (count, i)
    db.close()


def test_pairing_off_and_short_calls_keep_one_pass_per_group(monkeypatch):
    """PIRGPU_SCAN_MFMA_PAIR = 0 never pairs; 1 pairs only in calls that queue at least four groups."""
    s, queries, expected = shape_case("17x18")
    for mode, counts in ((0, {16: 2, 24: 3}), (1, {16: 2, 24: 3})):
        monkeypatch.setenv(PAIR, str(mode))
        db, srv = make(s)
        for count, launches in counts.items():
            before = db.get_option("SCAN_LAUNCHES")
            got = srv.process_batch(queries[:count].copy(), n_workers=16)
            assert db.get_option("SCAN_LAUNCHES") - before == launches, (mode, count)
            for i in range(count):
                assert np.array_equal(got[i], expected[i]), (mode, count, i)
        db.close()
    # four groups and a fifth: two pairs and a single under value 1
    monkeypatch.delenv(PAIR)                                     # the default is 1
    db, srv = make(s)
    q40 = np.concatenate([queries, queries[:16]])
    before = db.get_option("SCAN_LAUNCHES")
    got = srv.process_batch(q40, n_workers=16)
    assert db.get_option("SCAN_LAUNCHES") - before == 3
    for i in range(40):
        assert np.array_equal(got[i], expected[i % NQ]), i
    db.close()


def test_two_clients_mixed_inside_each_group(monkeypatch):
    """Queries of two clients alternate inside both groups of a pair: every query is expanded with its own client's keys."""
    monkeypatch.setenv(PAIR, "2")
    s, _, _ = shape_case("17x18")
    db, srv = make(s)
    other = Client(s.orc, seed=7)
    clients = [(s.client, s.galois_keys), (other, other.galois_keys())]
    slots = [srv.install_keyset(b"pair-client-%d" % i, keys) for i, (_, keys) in enumerate(clients)]
    n = s.params.num_items
    idx = [(53 * i + 5) % n for i in range(16)]
    who = [(i + i // 8) % 2 for i in range(16)]
    qs = np.stack([clients[w][0].create_query_for(s.params, x) for w, x in zip(who, idx)])
    srv.set_concurrency(16)
    srv.stage_batch(qs)
    srv.set_batch_keysets([slots[w] for w in who])
    before = db.get_option("SCAN_LAUNCHES")
    srv.run_batch()
    out = srv.fetch_batch()
    assert db.get_option("SCAN_LAUNCHES") - before == 1
    for i in range(16):
        rc, exp = s.orc.process_query(s.db_ntt, s.params.dimensions, qs[i], clients[who[i]][1])
        assert rc == 0 and np.array_equal(out[i], exp), i
    db.close()


# ---- structured extremes (the operands of tests/test_gpu_scan_worst_case.py): group 0's column selectors all at the
# residue whose digits are all +127 / top +7, group 1's all at the -128 / -8 end -- a B tile or an accumulator that leaks
# from one group into the other cannot cancel
@functools.lru_cache(maxsize=None)
def extremes_of(bits, low_end, top4):
    """The operands below for two data primes of `bits` bits at either end of the size, either top-digit form."""
    case = case_of(bits, 5, low_end, top4, 192)                 # 9 rows x 192 columns: 3 k-steps, one chunk
    k = 2
    rng = np.random.default_rng(2024)
    members = {0: 3, 1: 0}                                      # group -> member: (+127, top max), (-128, top min)
    sv = np.empty((4, ROWS + case.cols, 2, k, N), dtype=np.uint64)
    expected = []
    for v in range(4):                                          # two distinct selection vectors per group
        m = case.members[members[v // 2]]
        for j, q in enumerate(case.qs):
            sv[v, :ROWS, :, j, :] = rng.integers(0, q, size=(ROWS, 2, N), dtype=np.uint64)
            sv[v, ROWS:, :, j, :] = np.uint64(m % q)
        seal = sv[v].copy()
        seal[:ROWS] = device_to_seal_order(sv[v, :ROWS])
        rc, exp = case.orc.db_multiply(case.db_ntt, case.params.dimensions, seal, sv_is_ntt=np.ones(ROWS + case.cols, np.uint8))
        assert rc == 0 and exp.any()
        expected.append(exp)
    order = [0, 1] * 4 + [2, 3] * 4                             # queries 0-7: group 0, 8-15: group 1
    return case, sv, expected, order


def extremes():
    return extremes_of(36, True, True)


def run_selectors(srv, sv_dev, count):
    srv.stage_batch(np.zeros((count, 1, 2, 2, N), dtype=np.uint64))     # sizes the reply buffers
    srv.batch_run_selectors(sv_dev.data_ptr(), count)


def opposite_extremes(operands, top4, fold):
    """One pair per orientation, group 0 at one end of the digits and group 1 at the other."""
    import torch
    case, sv, expected, order = operands
    db, srv = context(case, scan_mfma_top4=1 if top4 else 0, scan_f64_fold_batch=fold)
    info, arith = srv.scan_info(), srv.arith_info()
    assert info["mfma"] and info["digits"] == 5 and info["chunks"] == 1 and info["ksteps"] == 3, info
    assert info["top_digit_nibble"] == top4 and arith["scan_f64_fold_batch"] == bool(fold), (info, arith)
    srv.set_concurrency(16)
    for flip in (False, True):                                  # either group at either end
        o = order[8:] + order[:8] if flip else order
        sv_dev = torch.from_numpy(np.stack([sv[v] for v in o]).view(np.int64)).cuda()
        before = db.get_option("SCAN_LAUNCHES")
        run_selectors(srv, sv_dev, 16)
        got = srv.fetch_batch()
        assert db.get_option("SCAN_LAUNCHES") - before == 1
        for i, v in enumerate(o):
            assert np.array_equal(got[i], expected[v]), (flip, i)
    db.close()


@pytest.mark.parametrize("fold", [1, 0], ids=["fp64 fold", "integer fold"])
def test_groups_at_opposite_extremes(fold, monkeypatch):
    monkeypatch.setenv(PAIR, "2")
    opposite_extremes(extremes(), True, fold)


@pytest.mark.parametrize("fold", [1, 0], ids=["fp64 fold", "integer fold"])
@pytest.mark.parametrize("low_end", [True, False], ids=["smallest primes", "largest primes"])
def test_groups_at_opposite_extremes_of_the_byte_form(low_end, fold, monkeypatch):
    """39-bit primes: the top digit is a full byte because it has to be (it reaches -64 / +63 where the 36-bit primes'
    stays inside a nibble), so the TOP4 = false loaders, the LDS round trip of group 1's top-digit tile and both folds
    meet top digits at both ends of the centring -- one group at each end, either way round."""
    monkeypatch.setenv(PAIR, "2")
    operands = extremes_of(39, low_end, False)
    case = operands[0]
    tops = [M.to_digits(case.members[m] % q, q, 5, False)[0][4] for m in (3, 0) for q in case.qs]
    assert min(tops) <= -31 and max(tops) >= 31, tops          # four times what a nibble holds
    opposite_extremes(operands, False, fold)


def assert_one_lane(srv):
    """A pass that has the chip to itself (0 = all CUs) although its call queued two groups: the call had ONE lane
    (batch_run_mfma shares the chip as soon as two groups meet two lanes), so every pair of the context ran on lane 0."""
    t = srv.batch_scan_timings()
    assert t["launches"] >= 1 and t["workgroups"] == 0 and t["queries"] == 16, t


def test_two_calls_back_to_back_without_a_host_wait(monkeypatch):
    """The lane-owned packed selectors and row sums of a pair's second group are reused by the next call: ordered by the
    lane's stream alone.  8 workers are one lane of 8 (lanes in use = min(2, workers / 8)), so the waited reference call,
    call 1 and call 2 all run on lane 0.  Call 1's replies are copied aside on the device (no host wait), call 2 is queued
    right behind it with the groups swapped: its sel_pack overwrites the buffers call 1's pass reads."""
    import torch
    monkeypatch.setenv(PAIR, "2")
    case, sv, expected, order = extremes()
    db, srv = context(case)
    srv.set_concurrency(8)
    srv.set_profiling(True)
    flipped = order[8:] + order[:8]
    sv1 = torch.from_numpy(np.stack([sv[v] for v in order]).view(np.int64)).cuda()
    sv2 = torch.from_numpy(np.stack([sv[v] for v in flipped]).view(np.int64)).cuda()
    words = 16 * db.reply_ct_count() * db.reply_ct_words()
    ref = torch.zeros(words, dtype=torch.int64, device="cuda")
    aside = torch.zeros(words, dtype=torch.int64, device="cuda")
    # reference: call 1 alone, waited for
    run_selectors(srv, sv1, 16)
    srv.batch_reply_copy_to_device(ref.data_ptr())
    srv.device_synchronize()
    before = db.get_option("SCAN_LAUNCHES")
    run_selectors(srv, sv1, 16)
    srv.batch_reply_copy_to_device_async(aside.data_ptr())      # main stream: behind the lane, no host wait
    srv.fork()                                                  # the lane: behind that copy
    srv.batch_run_selectors(sv2.data_ptr(), 16)
    got = srv.fetch_batch()
    assert db.get_option("SCAN_LAUNCHES") - before == 2
    srv.device_synchronize()
    assert torch.equal(aside, ref) and bool(ref.any())
    for i, v in enumerate(flipped):
        assert np.array_equal(got[i], expected[v]), i
    assert_one_lane(srv)
    db.close()


def test_expanding_pairs_back_to_back_on_one_lane(monkeypatch):
    """The expanding path: the second group's selection vectors live in the lane's own buffer too.  One lane (8 workers),
    32 staged queries: two pairs run right behind one another on lane 0, the second pair's expansion, packing and pass
    overwrite what the first pair's read, with nothing but the lane's stream between them -- and every reply of both pairs
    is checked.  Then the same batch twice more without a fetch or a wait between the calls."""
    monkeypatch.setenv(PAIR, "2")
    s, queries, expected = shape_case("17x18")
    db, srv = make(s)
    srv.set_concurrency(8)
    srv.set_profiling(True)
    q32 = np.stack([queries[i % NQ] for i in range(32)])        # groups: queries 0-7, 8-15, 16-23, 0-7
    want = [expected[i % NQ] for i in range(32)]
    srv.stage_batch(q32)
    before = db.get_option("SCAN_LAUNCHES")
    srv.run_batch()
    got = srv.fetch_batch()
    assert db.get_option("SCAN_LAUNCHES") - before == 2
    for i in range(32):
        assert np.array_equal(got[i], want[i]), i
    srv.run_batch()
    srv.run_batch()
    got = srv.fetch_batch()
    assert db.get_option("SCAN_LAUNCHES") - before == 6
    for i in range(32):
        assert np.array_equal(got[i], want[i]), ("again", i)
    assert_one_lane(srv)
    db.close()
