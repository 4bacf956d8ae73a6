"""The paired database pass (pir_amd/csrc/scan_mfma_pair.hip, the two-half step of batch_run_mfma in ctx.hip) on
every path that reaches it and on every path that must not -- what tests/test_gpu_scan_pair.py leaves out:

  A  moduli and rings   byte-form top digits that need the byte (37 / 38 / 39-bit primes), three data primes (the unit walk
                        crosses two modulus boundaries), N = 8192 (another shift from slot to modulus)
  B  workgroup counts   the persistent walk with one workgroup, ragged shares (1024 units over 7 and 96) and a request
                        above the CU count, through the live option SCAN_MFMA_WGS_BATCH: the pair kernel, the single
                        kernel's group launches and scan_mfma_runs_kernel
  C  queueing           d = 3, the head stream (both head slots of a lane taken by one pair), per-group host downloads,
                        SEL_F64 = 0, a streamed database, an in-place item update between two paired batches
  D  no pairing         every context may_pair excludes serves the same launches with the switch at 0 and at 2

Every reply is compared bit for bit with the CPU oracle (or with the mode's model); SCAN_LAUNCHES, scan_info, arith_info
and batch_scan_timings prove the path.  The oracle's process_query is the slow part: a shape computes at most 4 distinct
queries, batches repeat them so that neighbours in a group differ and so do the two queries at the same place of a
pair's two groups (position i holds query (i + i // 8) mod 4).  PIRGPU_SCAN_MFMA_PAIR = 2 unless a test says otherwise."""
import ctypes as C
import functools

import numpy as np
import pytest

import pir_amd
from gpu_helpers import chain, to_product_params
from test_gpu_mfma_scan import setup_with_dims
from test_gpu_scan_pair import LAUNCHES, PAIR, SHAPES, make, shape_case

pytestmark = pytest.mark.gpu


def spread(distinct, count):
    """Positions of a batch -> which of the `distinct` queries: neighbours differ, and so do positions i and i + 8."""
    return [(i + i // 8) % distinct for i in range(count)]


def fill(distinct_queries, replies, count):
    which = spread(len(distinct_queries), count)
    return np.stack([distinct_queries[w] for w in which]), [replies[w] for w in which]


@functools.lru_cache(maxsize=None)
def small_case(ring, shape, distinct=4):
    """Setup, `distinct` queries and the oracle's replies for one (modulus chain, matrix): computed once."""
    N, bits = RINGS[ring]
    s = setup_with_dims(2, 2048, SHAPE_DIMS[shape], N=N, plain_bits=24 if len(SHAPE_DIMS[shape]) == 2 else 20,
                        moduli=None if bits is None else chain(N, bits))
    n = s.params.num_items
    queries = [s.client.create_query_for(s.params, i) for i in (n - 1, 110 % n, 0, (n // 2 + 7) % n)[:distinct]]
    replies = []
    for q in queries:
        rc, exp = s.orc.process_query(s.db_ntt, s.params.dimensions, q, s.galois_keys)
        assert rc == 0
        replies.append(exp)
    return s, queries, replies


def run_counted(db, srv, queries, workers=16, **kw):
    before = db.get_option("SCAN_LAUNCHES")
    got = srv.process_batch(queries.copy(), n_workers=workers, **kw)
    return got, db.get_option("SCAN_LAUNCHES") - before


def assert_replies(got, want, what=None):
    assert len(got) == len(want)
    for i in range(len(want)):
        assert np.array_equal(got[i], want[i]), (what, i)


# ---------------------------------------------------------------------------------------------- A: moduli and rings

RINGS = {"N=4096 3x39 bits": (4096, [39] * 3), "N=4096 2x37 bits": (4096, 37), "N=8192 2x38 bits": (8192, 38),
         "N=4096 2x36 bits": (4096, None), "N=4096 2x44 bits": (4096, 44)}
SHAPE_DIMS = {"17x18": [17, 18], "18x70": [18, 70], "4x4x40": [4, 4, 40], "9x200": [9, 200]}
# the oracle costs twice as much at N = 8192: its smaller matrix only
UNSEEN = [(r, sh) for r in ("N=4096 3x39 bits", "N=4096 2x37 bits") for sh in ("17x18", "18x70")] + [("N=8192 2x38 bits", "17x18")]


@pytest.mark.parametrize("fold", [1, 0], ids=["fp64 fold", "integer fold"])
@pytest.mark.parametrize("ring,shape", UNSEEN, ids=["%s %s" % c for c in UNSEEN])
def test_byte_form_moduli_and_other_rings(ring, shape, fold, monkeypatch):
    """The TOP4 = false instantiations on moduli that take them by default: nothing forces the byte form here."""
    monkeypatch.setenv(PAIR, "2")
    s, queries, replies = small_case(ring, shape)
    db, srv = make(s, scan_f64_fold_batch=fold, scan_f64_fold=0)
    info = srv.scan_info()
    assert info["mfma"] and info["digits"] == 5 and info["chunks"] == 1 and info["ksteps"] == SHAPES[shape][1], info
    assert not info["top_digit_nibble"] and srv.arith_info()["scan_f64_fold_batch"] == bool(fold), info
    assert s.orc.k == (3 if "3x" in ring else 2) and s.orc.N == RINGS[ring][0]
    for count in (16, 9):
        q, want = fill(queries, replies, count)
        got, launches = run_counted(db, srv, q)
        assert launches == LAUNCHES[count][0] == 1, (count, launches)        # one launch per pair
        assert_replies(got, want, count)
    db.close()


# ---------------------------------------------------------------------------------------------- B: workgroup counts

WGS = (1, 7, 96, 100000)            # one workgroup walks all 1024 units; 1024 = 146 * 7 + 2 = 10 * 96 + 64; above the CU count


@pytest.mark.parametrize("mode,launches,per_launch", [(2, 1, 16), (0, 2, 8)], ids=["pair kernel", "two single-group launches"])
def test_workgroup_counts_of_a_pass_that_shares_the_chip(mode, launches, per_launch, monkeypatch):
    """16 queries on 16 workers: two groups on two lanes, so the call shares the chip and the pass runs on
    SCAN_MFMA_WGS_BATCH workgroups -- set anew before every batch of one context."""
    monkeypatch.setenv(PAIR, str(mode))
    s, queries, expected = shape_case("17x18")
    db, srv = make(s)
    srv.set_profiling(True)
    assert s.orc.k * s.orc.N // 8 == 1024
    for wgs in WGS:
        db.set_option("SCAN_MFMA_WGS_BATCH", wgs)
        got, delta = run_counted(db, srv, queries[:16])
        t = srv.batch_scan_timings()
        print("workgroups %d: %s" % (wgs, t))
        assert delta == launches, (wgs, delta)
        assert t["launches"] == launches and t["workgroups"] == wgs and t["queries"] == per_launch, (wgs, t)
        assert_replies(got, expected[:16], wgs)
    db.close()


@functools.lru_cache(maxsize=None)
def two_tables():
    """test_gpu_tables.py's world with T = 2 (9 x 9 plaintexts each), two queries: four (table, query) replies."""
    import test_gpu_tables as T
    w = T.World(2, 3000, N=T.N, plain_bits=24)
    idx = [T.index_of(0, 3000), T.index_of(1, 3000)]
    return w, idx


def test_seven_workgroups_under_the_runs_kernel():
    """11 queries of two tables on 16 workers, served as [0 x 8] [0 1 1]: the second group holds two tables and takes
    scan_mfma_runs_kernel (one launch for both runs), on 7 workgroups because the call has two groups for two lanes."""
    w, idx = two_tables()
    tables = [0] * 9 + [1, 1]
    queries = np.stack([w.query(idx[i % 2]) for i in range(11)])
    db, srv = w.server()
    info = srv.scan_info()
    assert info["mfma"] and info["rows"] == 9 and info["chunks"] == 1, info
    srv.set_profiling(True)
    db.set_option("SCAN_MFMA_WGS_BATCH", 7)
    got, delta = run_counted(db, srv, queries, tables=tables)
    t = srv.batch_scan_timings()
    assert delta == 2 and t["launches"] == 2, (delta, t)          # (TABLES_ONE_LAUNCH = 0 would take three)
    assert t["workgroups"] == 7 and t["queries"] == 3, t          # the last launch: the group of three, two runs
    assert_replies(got, [w.want(tables[i], idx[i % 2]) for i in range(11)])
    db.close()


# ---------------------------------------------------------------------------------------------- C: queueing paths

@pytest.mark.parametrize("count", [16, 24])
def test_three_dimensions(count, monkeypatch):
    """d = 3: the two halves of a pair share the lane's middle level, the second half starts from its own row sums."""
    monkeypatch.setenv(PAIR, "2")
    s, queries, replies = small_case("N=4096 2x36 bits", "4x4x40")
    db, srv = make(s)
    info = srv.scan_info()
    assert info["mfma"] and (info["rows"], info["cols"], info["ksteps"]) == (16, 40, 1), info
    q, want = fill(queries, replies, count)
    got, launches = run_counted(db, srv, q)
    assert launches == LAUNCHES[count][0], launches
    assert_replies(got, want)
    db.close()


def test_head_stream_with_both_slots_taken_by_one_pair(monkeypatch):
    """HEAD_MODE = 2: the first 5 levels of every group's expansion run on the head stream, in one of the lane's two
    head slots -- a pair takes both.  dim_sum = 88 leaves the lane two levels.  16 queries on two lanes; then 32 on
    one lane: two pairs behind one another reuse both slots, twice more without a fetch or a wait in between."""
    monkeypatch.setenv(PAIR, "2")
    s, queries, expected = shape_case("18x70")
    assert s.params.dim_sum == 88
    db, srv = make(s, head_mode=2)
    got, launches = run_counted(db, srv, queries[:16])
    assert launches == 1
    assert_replies(got, expected[:16], "two lanes")
    srv.set_concurrency(8)
    q32 = np.stack([queries[i % 24] for i in range(32)])
    want = [expected[i % 24] for i in range(32)]
    srv.stage_batch(q32)
    before = db.get_option("SCAN_LAUNCHES")
    srv.run_batch()
    assert_replies(srv.fetch_batch(), want, "one lane")
    srv.run_batch()
    srv.run_batch()
    got = srv.fetch_batch()
    assert db.get_option("SCAN_LAUNCHES") - before == 6
    assert_replies(got, want, "again")
    db.close()


def test_host_downloads_once_per_half(monkeypatch):
    """pirgpu_batch_set_host_replies with 24 queries: a pair on one lane (its halves download separately), a lone group
    on the other.  The groups are reported in ascending order, and what is reported is the oracle's already."""
    monkeypatch.setenv(PAIR, "2")
    s, queries, expected = shape_case("17x18")
    db, srv = make(s)
    srv.set_concurrency(16)
    batch, n = 24, db.reply_ct_count()
    lib, h = srv.lib, db.handle
    host = lib.pirgpu_host_reply_buffer(h, batch)
    assert host
    view = np.ctypeslib.as_array(C.cast(host, C.POINTER(C.c_uint64)), shape=(batch, n, 2, srv.k, srv.N))
    view[:] = 0
    assert lib.pirgpu_batch_set_host_replies(h, C.c_void_p(host), batch * n) == 0
    srv.stage_batch(queries.copy())
    before = db.get_option("SCAN_LAUNCHES")
    srv.run_batch()
    assert db.get_option("SCAN_LAUNCHES") - before == LAUNCHES[24][0] == 2
    seen, ready = [], C.c_uint32(0)
    while not seen or seen[-1] < batch:
        assert lib.pirgpu_batch_next_host_replies(h, C.byref(ready)) == 0
        assert ready.value > (seen[-1] if seen else 0), (seen, ready.value)
        for i in range(ready.value):
            assert np.array_equal(view[i], expected[i]), (ready.value, i)
        seen.append(ready.value)
    assert seen == [8, 16, 24], seen
    assert lib.pirgpu_batch_next_host_replies(h, C.byref(ready)) == 0 and ready.value == batch
    cnt = C.c_uint64(0)
    assert lib.pirgpu_batch_fetch(h, C.cast(host, C.POINTER(C.c_uint64)), batch * n, C.byref(cnt)) == 0
    assert cnt.value == batch * n
    assert_replies(view, expected)
    assert lib.pirgpu_batch_set_host_replies(h, None, 0) == 0
    db.close()


def test_selectors_as_integers(monkeypatch):
    """SEL_F64 = 0: the lane's own selectors reach sel_pack and the upper level as 64-bit words."""
    monkeypatch.setenv(PAIR, "2")
    s, queries, expected = shape_case("17x18")
    db, srv = make(s, sel_f64=0)
    assert db.get_option("SEL_F64") == 0
    for count in (16, 9):
        got, launches = run_counted(db, srv, queries[:count])
        assert launches == 1
        assert_replies(got, expected[:count], count)
    db.close()


def test_streamed_database(monkeypatch):
    """A database loaded in row bands straight into the operand layout (17 rows: a band of 16 and a band of one)."""
    monkeypatch.setenv(PAIR, "2")
    s, queries, expected = shape_case("17x18")
    pp = to_product_params(s.params)
    db = pir_amd.PIRDatabase.Create(pp, streamed=True)
    db.set_option("DB_STREAM_MB", 1)
    db.populate(s.raw)
    srv = pir_amd.PIRServer(db, pp)
    srv.set_galois_keys(s.galois_keys)
    mem = db.memory()
    assert mem["staging"] == 0 and mem["band"] == 16 * 18 * s.orc.k * s.orc.N * 8 and s.params.dimensions[0] > 16, mem
    for count in (16, 24):
        got, launches = run_counted(db, srv, queries[:count])
        assert launches == LAUNCHES[count][0]
        assert_replies(got, expected[:count], count)
    db.close()


def test_items_updated_in_place_between_two_paired_batches(monkeypatch):
    """A paired batch, update_items on the items two of its queries ask for (and two bystanders), a paired batch again:
    the replies of a freshly populated context with the new items, and the oracle's on the new database."""
    monkeypatch.setenv(PAIR, "2")
    s, queries, expected = shape_case("17x18")
    p = s.params
    n = p.num_items
    asked = [(97 * i + 13) % n for i in range(4)]                # the items of shape_case's first four queries
    which = spread(4, 16)
    q16 = np.stack([queries[w] for w in which])
    db, srv = make(s)
    got, launches = run_counted(db, srv, q16)
    assert launches == 1
    assert_replies(got, [expected[w] for w in which], "before")
    touched = [asked[0], asked[2], asked[2] + 1, n - 1]
    items = np.random.default_rng(77).integers(0, 256, size=(len(touched), p.bytes_per_item), dtype=np.uint8)
    db.update_items(touched, items)
    raw = s.raw.copy()                                           # (the shared setup stays as it is)
    raw[touched] = items
    rc, db_ntt = s.orc.db_encode(raw.tobytes(), n, p.bytes_per_item, p.items_per_plaintext, p.eff_bits_per_coeff, p.num_pt)
    assert rc == 0
    want = []
    for i in range(4):
        rc, exp = s.orc.process_query(db_ntt, p.dimensions, queries[i], s.galois_keys)
        assert rc == 0
        want.append(exp)
    assert not np.array_equal(want[0], expected[0]) and not np.array_equal(want[2], expected[2])
    got, launches = run_counted(db, srv, q16)
    assert launches == 1
    assert_replies(got, [want[w] for w in which], "after")
    db.close()
    pp = to_product_params(p)
    fresh_db = pir_amd.PIRDatabase.Create(pp, raw)
    fresh = pir_amd.PIRServer(fresh_db, pp)
    fresh.set_galois_keys(s.galois_keys)
    again, launches = run_counted(fresh_db, fresh, q16)
    assert launches == 1 and np.array_equal(again, got)
    assert s.client.process_response(p, asked[0], got[which.index(0)]) == items[0].tobytes()
    fresh_db.close()


# ---------------------------------------------------------------------------------------------- D: contexts that must not pair

def _tables():
    w, idx = two_tables()
    tables = [0, 0, 1, 1] * 4                                    # served as [0 x 8] [1 x 8]: a batch ordered by table
    queries = np.stack([w.query(idx[i % 2]) for i in range(16)])
    want = [w.want(tables[i], idx[i % 2]) for i in range(16)]
    return w.server, queries, want, dict(tables=tables), dict(rows=9), 2


def _result_primes():
    import test_gpu_modswitch as MS
    s = _cached("rp", lambda: MS.setup("4096/36", 100, 2))
    qs = [s.client.create_query_for(s.params, i) for i in (98, 5)]
    reps = _cached("rp replies", lambda: [MS.expected(s, q, 1) for q in qs])
    queries, want = fill(qs, reps, 16)
    return (lambda: MS.server(s, 1)), queries, want, {}, dict(rows=10), 2


def _wide_items():
    import test_gpu_wide_items as W
    s = _cached("wide", lambda: W.WideSetup(100, 15000, 2, N=4096, plain_bits=20))
    assert s.planes == 2
    qs = [s.query(i) for i in (57, 99)]
    reps = _cached("wide replies", lambda: [s.expected(q) for q in qs])
    queries, want = fill(qs, reps, 16)
    return s.server, queries, want, {}, dict(rows=20, cols=10), 2


def _ctmult():
    import test_gpu_ctmult as CT
    s = _cached("ct", lambda: CT.setup(16, 2, dims=[8, 2]))
    qs = [s.client.create_query_for(s.params, i) for i in (3, 14)]
    reps = _cached("ct replies", lambda: [CT.expected(s, q) for q in qs])
    queries, want = fill(qs, reps, 16)
    return (lambda: CT.ct_server(s)), queries, want, {}, dict(rows=8), 2


def _plain(ring, shape, info, launches, **options):
    """An ordinary database whose geometry or group size the pair kernel is not built for."""
    def case():
        if (ring, shape) == ("N=4096 2x36 bits", "17x18"):
            s, q24, e24 = shape_case(shape)                      # (already computed for the tests above)
            queries, replies = [q24[0], q24[1]], e24[:2]
        else:
            s, queries, replies = small_case(ring, shape, 2)
        q, want = fill(queries, replies, 16)
        return (lambda: make(s, **options)), q, want, {}, info, launches
    return case


def _one_dimension():
    from pir_fixtures import PirSetup
    s = _cached("d1", lambda: PirSetup(120, 288, 1, N=4096, plain_bits=24))
    qs = [s.client.create_query_for(s.params, i) for i in (7, 119)]

    def replies():
        out = []
        for q in qs:
            rc, exp = s.orc.process_query(s.db_ntt, s.params.dimensions, q, s.galois_keys)
            assert rc == 0
            out.append(exp)
        return out
    queries, want = fill(qs, _cached("d1 replies", replies), 16)
    return (lambda: make(s)), queries, want, {}, dict(mfma=False), 0


_CACHE = {}


def _cached(key, compute):
    if key not in _CACHE:
        _CACHE[key] = compute()
    return _CACHE[key]


NO_PAIR = {
    "tables": _tables,
    "result_primes": _result_primes,
    "wide items": _wide_items,
    "ciphertext multiplication": _ctmult,
    "groups of four": _plain("N=4096 2x36 bits", "17x18", dict(queries_per_pass=4), 4, scan_mfma_nq=4),
    "six digits": _plain("N=4096 2x44 bits", "17x18", dict(digits=6), 2),
    "four-wave kernel": _plain("N=4096 2x36 bits", "9x200", dict(digits=5, chunks=1, ksteps=4), 2),
    "two chunks": _plain("N=4096 2x36 bits", "9x200", dict(digits=5, chunks=2, ksteps=2), 2, scan_mfma_wide=0),
    "one dimension": _one_dimension,
}


@pytest.mark.parametrize("name", list(NO_PAIR))
def test_contexts_that_keep_one_pass_per_group(name, monkeypatch):
    """Every term of may_pair (ctx.hip): 16 queries on 16 workers with the switch at 0 and at 2 queue the same database
    passes, and both contexts answer what the mode's model answers -- the paired pass (scan_pair_mfma in ctx.hip) knows
    nothing of tables, of the buffer result_primes switches from, of planes or of ciphertext products.  One dimension: the int8 scan and its counter need
    d >= 2, the batch takes the 64-bit scan and SCAN_LAUNCHES stays where it is -- only the replies say anything there."""
    build, queries, want, run_kw, info, launches = NO_PAIR[name]()
    deltas = []
    for mode in (0, 2):
        monkeypatch.setenv(PAIR, str(mode))
        db, srv = build()
        have = srv.scan_info()
        assert have["mfma"] == info.get("mfma", True), have
        for key, value in info.items():
            assert have[key] == value, (key, have)
        got, delta = run_counted(db, srv, queries, **run_kw)
        assert_replies(got, want, mode)
        deltas.append(delta)
        db.close()
    assert deltas[0] == deltas[1] == launches, deltas
