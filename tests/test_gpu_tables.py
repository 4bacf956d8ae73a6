"""Tables (pirgpu_params.tables) on the GPU: one context holds T databases of one shape, every
query names its table, and every reply is compared BIT FOR BIT with the oracle's processQuery (reference
server.cpp:173-195) on the database made of that table's items alone.  Tables get different seeds: a reply computed from
the wrong table differs from the expected one."""
import numpy as np
import pytest

import oracle
from oracle.client import Client

pytestmark = pytest.mark.gpu

N = 4096
ISSUE_BATCH = [2, 0, 1, 1, 0, 2, 2, 2, 2, 2, 2, 2, 2, 2, 0, 1, 2, 0, 1]


class World:
    """T tables of `items` items each (one PirSetup per table: its raw items and the oracle's encoded database), one
    client whose parameters are those of ONE table, and the oracle's replies, computed once per (table, index, keys)."""

    def __init__(self, T, items, elem=288, d=2, **kw):
        from gpu_helpers import to_product_params
        from pir_fixtures import PirSetup
        self.T, self.items = T, items
        self.tabs = [PirSetup(items, elem, d, seed=1000 + 17 * t, **kw) for t in range(T)]
        s = self.tabs[0]
        self.s, self.p, self.orc, self.client, self.keys = s, s.params, s.orc, s.client, s.galois_keys
        self.pp = to_product_params(s.params)
        self.pp.tables = T
        self.raw = np.concatenate([t.raw for t in self.tabs])
        self._queries, self._want = {}, {}

    def query(self, index, client=None):
        c = client or self.client
        key = (index, id(c))
        if key not in self._queries:
            self._queries[key] = c.create_query_for(self.p, index)
        return self._queries[key]

    def want(self, table, index, client=None, keys=None):
        c = client or self.client
        key = (table, index, id(c))
        if key not in self._want:
            rc, w = self.orc.process_query(self.tabs[table].db_ntt, self.p.dimensions, self.query(index, c),
                                           keys if keys is not None else self.keys)
            assert rc == 0
            self._want[key] = w
        return self._want[key]

    def server(self, raw="all", params=None, **kw):
        import pir_amd
        pp = params or self.pp
        db = pir_amd.PIRDatabase.Create(pp, self.raw if isinstance(raw, str) else raw, **kw)
        srv = pir_amd.PIRServer.Create(db, pp)
        srv.set_galois_keys(self.keys)
        return db, srv


@pytest.fixture(scope="module")
def w3():
    return World(3, 3000, N=N, plain_bits=24)


def index_of(i, items):
    return (items - 1 - 131 * i) % items


# ------------------------------------------------------------------------------------------------ d = 2, int8 scan

def test_single_queries_and_a_mixed_batch_under_two_key_sets(w3):
    w = w3
    db, srv = w.server()
    assert db.tables() == 3 and db.size() == 3 * w.p.num_pt
    assert srv.scan_info()["mfma"] and srv.scan_info()["rows"] == 9
    for t in (1, 0, 2):                                            # sticky selection, every table
        srv.use_table(t)
        for i in (5, 2999 - t):
            assert np.array_equal(srv.process_query(w.query(i)), w.want(t, i)), (t, i)
    got = srv.process_query(w.query(5))
    assert np.array_equal(got, w.want(2, 5)) and not np.array_equal(got, w.want(0, 5))
    assert w.client.process_response(w.p, 5, got) == w.tabs[2].item(5)
    # 19 queries: runs of several lengths, more than 8 of one table, mixed groups -- every query with its client's keys
    other = Client(w.orc, seed=7)
    other_keys = other.galois_keys()
    clients = [w.client, other]
    slots = [srv.install_keyset(b"table-client-a", w.keys), srv.install_keyset(b"table-client-b", other_keys)]
    srv.set_concurrency(16)
    idx = [index_of(i, 3000) for i in range(19)]
    who = [i % 2 for i in range(19)]
    queries = np.stack([w.query(idx[i], clients[who[i]]) for i in range(19)])
    srv.use_table(1)                                               # the batch's own tables win over the selection
    for rep in range(2):
        srv.stage_batch(queries, tables=ISSUE_BATCH)
        srv.set_batch_keysets([slots[c] for c in who])
        srv.run_batch()
        got = srv.fetch_batch()
        for i in range(19):                                        # replies in SUBMISSION order
            want = w.want(ISSUE_BATCH[i], idx[i], clients[who[i]], [w.keys, other_keys][who[i]])
            assert np.array_equal(got[i], want), (rep, i)
    assert clients[1].process_response(w.p, idx[3], got[3]) == w.tabs[1].item(idx[3])
    # a staged batch without tables of its own goes to the selected table
    srv.stage_batch(queries[:4])
    srv.set_batch_keysets([slots[c] for c in who[:4]])
    srv.run_batch()
    got = srv.fetch_batch()
    for i in range(4):
        assert np.array_equal(got[i], w.want(1, idx[i], clients[who[i]], [w.keys, other_keys][who[i]])), i
    db.close()


def test_permuted_batch_downloads_its_replies_group_by_group(w3):
    """pirgpu_batch_set_host_replies on a batch served in another order than it was submitted (ISSUE_BATCH: three groups,
    served as 1 4 14 17 2 3 15 18 | 0 5 .. 11 | 12 13 16): every group downloads its own replies, one copy each, and
    reports how many LEADING queries of the batch are complete with it -- 0, 12, 19.  What has been reported is in the
    host buffer before the batch as a whole is; the replies are those of the plain fetch (pinned to the oracle by
    test_single_queries_and_a_mixed_batch_under_two_key_sets)."""
    import ctypes as C
    w = w3
    db, srv = w.server()
    srv.set_concurrency(16)
    batch = len(ISSUE_BATCH)
    queries = np.stack([w.query(index_of(i, 3000)) for i in range(batch)])
    srv.stage_batch(queries, tables=ISSUE_BATCH)
    srv.run_batch()
    plain = srv.fetch_batch()
    n = db.reply_ct_count()
    lib, h = srv.lib, db.handle
    host = lib.pirgpu_host_reply_buffer(h, batch)
    assert host
    view = np.ctypeslib.as_array(C.cast(host, C.POINTER(C.c_uint64)), shape=(batch, n, 2, srv.k, srv.N))
    assert view.shape == plain.shape
    view[:] = 0
    assert lib.pirgpu_batch_set_host_replies(h, C.c_void_p(host), batch * n) == 0
    srv.stage_batch(queries, tables=ISSUE_BATCH)
    srv.run_batch()
    seen, ready = [], C.c_uint32(0)
    for _ in range(3):                                             # one report per group
        assert lib.pirgpu_batch_next_host_replies(h, C.byref(ready)) == 0
        assert ready.value >= (seen[-1] if seen else 0)
        assert np.array_equal(view[:ready.value], plain[:ready.value])
        seen.append(ready.value)
    assert seen == [0, 12, 19]
    assert lib.pirgpu_batch_next_host_replies(h, C.byref(ready)) == 0 and ready.value == batch   # nothing left: the total
    cnt = C.c_uint64(0)
    assert lib.pirgpu_batch_fetch(h, C.cast(host, C.POINTER(C.c_uint64)), batch * n, C.byref(cnt)) == 0
    assert cnt.value == batch * n
    assert np.array_equal(view, plain)
    assert lib.pirgpu_batch_set_host_replies(h, None, 0) == 0
    db.close()


def test_many_tiny_tables_take_one_launch_per_group():
    """T = 12, 16 queries on 12 distinct tables: served as [0 0 1 1 2 2 3 3][4 .. 11] -- a group of 4 runs and a group of
    8 runs of one query.  One database-pass launch per group; with TABLES_ONE_LAUNCH = 0 one per run; identical replies."""
    w = World(12, 3000, N=N, plain_bits=24)
    tables = list(range(12)) + [0, 1, 2, 3]
    idx = [index_of(i, 3000) for i in range(16)]
    queries = np.stack([w.query(i) for i in idx])
    replies = []
    for one_launch, launches in ((1, 2), (0, 12)):
        db, srv = w.server()
        assert srv.scan_info()["mfma"]
        db.set_option("tables_one_launch", one_launch)
        srv.set_concurrency(16)
        for rep in range(2):
            db.set_option("scan_launches", 0)
            got = srv.process_batch(queries, tables=tables)
            srv.sync()
            assert db.get_option("scan_launches") == launches, (one_launch, rep)
        replies.append(got)
        db.close()
    assert np.array_equal(replies[0], replies[1])
    for i in range(16):
        assert np.array_equal(replies[0][i], w.want(tables[i], idx[i])), i


# ------------------------------------------------------------------------------------------------ the other scans / shapes

M8 = oracle.BFV_DEFAULT[8192]
SHAPES = {
    "rows<8": dict(T=5, items=200, elem=288, d=2, mfma=False, kw=dict(N=N, plain_bits=24)),          # [3, 2]: 64-bit scan
    "d1": dict(T=3, items=120, elem=288, d=1, mfma=False, kw=dict(N=N, plain_bits=24)),
    "d3": dict(T=2, items=27, elem=0, d=3, mfma=True, kw=dict(N=N, plain_bits=24)),      # test_gpu_parity's d = 3: 9 rows x 3
    "N8192": dict(T=2, items=1203, elem=1024, d=2, mfma=True,                                         # k = 3, fp64, L = 6
                  kw=dict(N=8192, moduli=M8[:3] + [M8[4]], t=oracle.plain_modulus_batching(8192, 24))),
}


@pytest.mark.parametrize("case", list(SHAPES))
def test_tables_on_every_scan_family(case):
    c = SHAPES[case]
    w = World(c["T"], c["items"], c["elem"], c["d"], **c["kw"])
    db, srv = w.server()
    info = srv.scan_info()
    assert info["mfma"] == c["mfma"], info
    if case == "N8192":
        assert info["digits"] == 6 and srv.ntt_mode() == 1
    idx = [index_of(i, c["items"]) for i in range(3)]
    for t in range(c["T"]):
        srv.use_table(t)
        assert np.array_equal(srv.process_query(w.query(idx[t % 3])), w.want(t, idx[t % 3])), t
    # a batch over all tables, unsorted, with a repeat (the 64-bit passes serve up to 4 queries of ONE table)
    tables = [(c["T"] - 1 - i) % c["T"] for i in range(c["T"] + 2)]
    queries = np.stack([w.query(idx[i % 3]) for i in range(len(tables))])
    got = srv.process_batch(queries, n_workers=8, tables=tables)
    for i, t in enumerate(tables):
        assert np.array_equal(got[i], w.want(t, idx[i % 3])), (i, t)
    db.close()


def test_result_primes_with_tables(w3):
    """result_primes = 1, T = 3, on the int8 scan: every table against the model's switched processQuery on it alone."""
    import modswitch_model as M
    from gpu_helpers import to_product_params
    w = w3
    pp = to_product_params(w.p)
    pp.tables, pp.result_primes = 3, 1
    db, srv = w.server(params=pp)
    assert srv.scan_info()["mfma"]
    idx = [7, 2999, 1500]
    want = [M.process_query_switched(w.orc, w.tabs[t].db_ntt, w.p.dimensions, w.query(idx[t]), w.keys, 1) for t in range(3)]
    for t in range(3):
        srv.use_table(t)
        got = srv.process_query(w.query(idx[t]))
        assert got.shape == want[t].shape and np.array_equal(got, want[t]), t
    queries = np.stack([w.query(idx[t]) for t in (2, 0, 1)])
    got = srv.process_batch(queries, n_workers=8, tables=[2, 0, 1])
    for i, t in enumerate((2, 0, 1)):
        assert np.array_equal(got[i], want[t]), t
    db.close()


# ------------------------------------------------------------------------------------------------ storage

def test_storage_load_table_finalize(w3):
    w = w3
    P = w.p.num_pt
    db, srv = w.server()
    for t in range(3):
        for pt in (0, 1, P - 1):
            assert np.array_equal(db.read_plaintext(t * P + pt), w.tabs[t].db_ntt[pt]), (t, pt)
    srv.use_table(0)
    srv.process_query(w.query(5))                                  # packs
    mem = db.memory()
    per_table = mem["operand"] // 3
    assert mem["operand"] == 3 * per_table and srv.scan_bytes() == per_table
    before = [db.read_operand(t * per_table, per_table).copy() for t in range(3)]
    assert not np.array_equal(before[0], before[1])
    # reload table 1 alone with other items
    from pir_fixtures import generate_test_db
    new_raw = generate_test_db(3000, w.p.bytes_per_item, seed=4242)
    rc, new_ntt = w.orc.db_encode(new_raw.tobytes(), 3000, w.p.bytes_per_item, w.p.items_per_plaintext,
                                  w.p.eff_bits_per_coeff, P)
    assert rc == 0
    db.load_table(1, new_raw)
    srv.use_table(1)
    got = srv.process_query(w.query(5))
    rc, want = w.orc.process_query(new_ntt, w.p.dimensions, w.query(5), w.keys)
    assert np.array_equal(got, want) and not np.array_equal(got, w.want(1, 5))
    after = [db.read_operand(t * per_table, per_table) for t in range(3)]
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[2], before[2])
    assert not np.array_equal(after[1], before[1])
    assert np.array_equal(db.read_plaintext(P + 3), new_ntt[3])
    # release the staging copy, then queries on every table and plaintexts out of the operand layout
    db.finalize(release_staging=True)
    assert db.memory()["staging"] == 0 and db.memory()["operand"] == 3 * per_table
    for t, wnt in ((0, w.want(0, 5)), (1, want), (2, w.want(2, 5))):
        srv.use_table(t)
        assert np.array_equal(srv.process_query(w.query(5)), wnt), t
    assert np.array_equal(db.read_plaintext(2 * P + P - 1), w.tabs[2].db_ntt[P - 1])
    assert np.array_equal(db.read_plaintext(P + 3), new_ntt[3])
    from pir_amd.server import PirGpuError
    with pytest.raises(PirGpuError) as e:
        db.load_table(0, new_raw)                                  # no staging copy to load into
    assert e.value.code == 9
    db.close()


@pytest.mark.parametrize("release", [False, True])
def test_update_items_in_two_tables_equals_a_fresh_populate(w3, release):
    w = w3
    P, items = w.p.num_pt, 3000
    rng = np.random.default_rng(5)
    touched = [0 * items + 7, 0 * items + 8, 2 * items + 2999, 2 * items + 41, 0 * items + 7]     # a later entry wins
    new = rng.integers(0, 256, size=(len(touched), w.p.bytes_per_item), dtype=np.uint8)
    db, srv = w.server()
    srv.use_table(2)
    srv.process_query(w.query(41))                                 # packed before the update: updated in place
    if release:
        db.finalize(release_staging=True)
    db.update_items(touched, new)
    raw = w.raw.copy()
    for i, ix in enumerate(touched):
        raw[ix] = new[i]
    fresh_db, fresh = w.server(raw=raw)
    fresh_db.finalize(release_staging=release)
    n = db.memory()["operand"]
    assert n == fresh_db.memory()["operand"]
    assert np.array_equal(db.read_operand(0, n), fresh_db.read_operand(0, n))
    ipp = w.p.items_per_plaintext
    for ix in touched:
        t, pt = ix // items, (ix % items) // ipp
        assert np.array_equal(db.read_plaintext(t * P + pt), fresh_db.read_plaintext(t * P + pt)), ix
    for t, i in ((0, 7), (2, 2999), (1, 7)):
        srv.use_table(t)
        fresh.use_table(t)
        got = srv.process_query(w.query(i))
        assert np.array_equal(got, fresh.process_query(w.query(i))), (t, i)
        assert w.client.process_response(w.p, i, got) == raw[t * items + i].tobytes()
    assert np.array_equal(srv.process_query(w.query(7)), w.want(1, 7))          # table 1 untouched
    from pir_amd.server import PirGpuError
    with pytest.raises(PirGpuError) as e:
        db.update_items([3 * items], new[:1])
    assert e.value.code == 3
    db.close()
    fresh_db.close()


# ------------------------------------------------------------------------------------------------ transparent rule, refusals

def test_zero_plaintext_fails_its_own_table_only(w3):
    from pir_amd.server import PirGpuError
    w = w3
    ipp, items = w.p.items_per_plaintext, 3000
    raw = w.raw.copy()
    raw[items + 2 * ipp: items + 3 * ipp] = 0                      # plaintext 2 of table 1
    db, srv = w.server(raw=raw)
    assert srv.zero_plaintexts() == 1
    assert [db.table_zero_plaintexts(t) for t in range(4)] == [0, 1, 0, 0]
    for t in (0, 2):
        srv.use_table(t)
        srv.check_ready()
        assert np.array_equal(srv.process_query(w.query(5)), w.want(t, 5)), t
    srv.use_table(1)
    for call in (srv.check_ready, lambda: srv.process_query(w.query(5))):
        with pytest.raises(PirGpuError) as e:
            call()
        assert e.value.code == 13 and "transparent" in e.value.message
    srv.use_table(0)
    queries = np.stack([w.query(5)] * 3)
    db.set_option("scan_launches", 0)
    srv.stage_batch(queries, tables=[0, 1, 2])
    with pytest.raises(PirGpuError) as e:
        srv.run_batch()                                            # as a whole, before anything runs
    assert e.value.code == 13 and db.get_option("scan_launches") == 0
    got = srv.process_batch(queries[:2], tables=[2, 0])
    assert np.array_equal(got[0], w.want(2, 5)) and np.array_equal(got[1], w.want(0, 5))
    db.close()


def test_refusals_and_partial_loads(w3):
    import pir_amd
    from pir_amd import parameters as PP
    from pir_amd.server import PirGpuError
    w = w3
    for kw in (dict(shard=(0, 4)), dict(slots=(0, 4096)), dict(streamed=True)):
        with pytest.raises(PirGpuError) as e:
            pir_amd.PIRDatabase(w.pp, **kw)
        assert e.value.code == 3 and "tables" in e.value.message, kw
    enc = PP.generate_encryption_params(N, 24)
    wide = PP.create_pir_parameters(50, 20000, 2, enc, max_plaintexts_per_item=4)
    wide.tables = 2
    with pytest.raises(PirGpuError) as e:
        pir_amd.PIRDatabase(wide)
    assert e.value.code == 3 and "tables" in e.value.message
    # only table 2 loaded: it serves, the others are FailedPrecondition; then out-of-range tables; it still serves
    db = pir_amd.PIRDatabase(w.pp)
    db.load_table(2, w.tabs[2].raw)
    assert db.size() == w.p.num_pt
    srv = pir_amd.PIRServer.Create(db, w.pp)
    srv.set_galois_keys(w.keys)
    srv.use_table(2)
    assert np.array_equal(srv.process_query(w.query(5)), w.want(2, 5))
    srv.use_table(0)
    with pytest.raises(PirGpuError) as e:
        srv.process_query(w.query(5))
    assert e.value.code == 9
    queries = np.stack([w.query(5)] * 2)
    srv.stage_batch(queries, tables=[2, 1])
    with pytest.raises(PirGpuError) as e:
        srv.run_batch()
    assert e.value.code == 9
    with pytest.raises(PirGpuError) as e:
        srv.use_table(3)
    assert e.value.code == 3
    with pytest.raises(PirGpuError) as e:
        srv.stage_batch(queries, tables=[2, 3])
    assert e.value.code == 3
    with pytest.raises(PirGpuError) as e:
        db.load_table(3, w.tabs[0].raw)
    assert e.value.code == 3
    db.load_table(0, w.tabs[0].raw)
    got = srv.process_batch(queries, tables=[2, 0])                # table 1 is still empty
    assert np.array_equal(got[0], w.want(2, 5)) and np.array_equal(got[1], w.want(0, 5))
    db.close()


# ------------------------------------------------------------------------------------------------ T = 0 / 1, wire

def test_one_table_equals_a_context_without_the_field(w3):
    from gpu_helpers import to_product_params
    w = w3
    seen = []
    queries = np.stack([w.query(index_of(i, 3000)) for i in range(3)])
    for T in (None, 0, 1):
        pp = to_product_params(w.p)                                # parameters built without a word about tables
        if T is not None:
            pp.tables = T
        db, srv = w.server(raw=w.tabs[0].raw, params=pp)
        assert db.tables() == 1
        single = srv.process_query(w.query(5))
        batch = srv.process_batch(queries, n_workers=8)
        seen.append((single, batch, db.memory(), srv.scan_info(), srv.scan_bytes(), db.size()))
        db.close()
    assert np.array_equal(seen[0][0], w.want(0, 5))
    for other in seen[1:]:
        assert np.array_equal(other[0], seen[0][0]) and np.array_equal(other[1], seen[0][1])
        assert other[2:] == seen[0][2:]


def test_wire_requests_of_three_clients_on_three_tables(w3):
    import pir_amd
    from gpu_helpers import to_product_params
    w = w3
    one = to_product_params(w.p)                                   # the client's parameters: ONE table
    clients = [pir_amd.PIRClient.Create(one, seed=b"tables-wire-%d" % i) for i in range(3)]
    wants = [[5, 2999], [77], [1234, 0, 41]]
    tables = [2, 0, 1]
    requests = [c.CreateRequest(ix) for c, ix in zip(clients, wants)]
    db, srv = w.server()
    out = srv.ProcessRequests(requests, tables=tables)
    for (st, resp), c, ix, t in zip(out, clients, wants, tables):
        assert st == 0
        assert c.ProcessResponse(ix, resp) == [w.tabs[t].item(i) for i in ix]      # 3000 items: inside the noise budget
    # the bytes a one-table context holding that table answers with
    for r, t, (st, resp) in zip(requests, tables, out):
        sdb, single = w.server(raw=w.tabs[t].raw, params=one)
        assert single.ProcessRequest(r) == resp, t
        sdb.close()
    assert srv.ProcessRequest(requests[1], table=0) == out[1][1]
    assert srv.ProcessRequest(requests[1]) == out[1][1]                            # the existing entry: table 0
    assert srv.ProcessRequest(requests[1], table=2) != out[1][1]
    bad = srv.ProcessRequests(requests[:2], tables=[1, 3])
    assert bad[0][0] == 0 and bad[1][0] == 3 and "table" in srv.request_errors[1]
    db.close()
