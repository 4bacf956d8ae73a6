"""In-place database updates (pirgpu_db_update_items / pirgpu_db_update_plaintexts, PIRDatabase.update_items /
update_plaintexts).  No reference counterpart: the contract is that after an update the context is indistinguishable
from one populated from scratch with the updated raw database.  The expected values are always the oracle's on the
UPDATED raw database (orc.db_encode over the modified items, then orc.process_query / db_multiply)."""
import numpy as np
import pytest

import oracle
import pir_amd
from gpu_helpers import to_product_params
from pir_amd.server import PirGpuError
from pir_fixtures import PirSetup

pytestmark = pytest.mark.gpu


def setup_with_dims(short, elem, dims, **kw):
    """PirSetup with an explicit dimension vector, prod(dims) plaintexts and `short` items fewer than they hold."""
    probe = oracle.create_pir_parameters(10, elem, 1, **{k: v for k, v in kw.items() if k in
                                                          ("N", "plain_bits", "moduli", "t")})
    pts = int(np.prod(dims))
    s = PirSetup(pts * probe.items_per_plaintext - short, elem, len(dims), **kw)
    assert s.params.num_pt == pts
    s.params.dimensions = list(dims)
    return s


def make(s, release=None, shard=None, slots=None):
    """Server populated with s.raw; release None: no finalize, False / True: finalize keeping / releasing staging."""
    pp = to_product_params(s.params)
    db = pir_amd.PIRDatabase.Create(pp, s.raw, shard=shard, slots=slots)
    if release is not None:
        db.finalize(release_staging=release)
    srv = pir_amd.PIRServer(db, pp)
    srv.set_galois_keys(s.galois_keys)
    return db, srv


def reencode(s):
    p = s.params
    rc, s.db_ntt = s.orc.db_encode(s.raw.tobytes(), p.num_items, p.bytes_per_item, p.items_per_plaintext,
                                   p.eff_bits_per_coeff, p.num_pt)
    assert rc == 0


def apply_to_raw(s, indices, items):
    for i, it in zip(indices, items):      # a later entry wins, as in the library
        s.raw[i] = it
    reencode(s)


def new_items(s, n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, s.params.bytes_per_item), dtype=np.uint8)


def edge_indices(s, cols):
    """The update list every geometry gets: first item, last item (in a partial last plaintext), two items of one
    plaintext, a duplicated index, the plaintexts in columns 2 and 6 of one 16-column group (one TOP4 nibble byte) and
    items whose bits share a coefficient with untouched neighbours (every item boundary here is inside a coefficient)."""
    p = s.params
    n, ipp = p.num_items, p.items_per_plaintext
    assert n % ipp, "the last plaintext must be partial"
    r = min(1, p.num_pt // cols - 1)
    pa, pb = r * cols + 2, r * cols + 6
    idx = [0, n - 1, 3 * ipp, 3 * ipp + 1, 5 * ipp + 1, pa * ipp + ipp // 2, pb * ipp, 5 * ipp + 1]
    return [i for i in idx if i < n]


def touched_and_neighbours(s, indices):
    ipp, P = s.params.items_per_plaintext, s.params.num_pt
    pts = set()
    for i in indices:
        for d in (-1, 0, 1):
            if 0 <= i // ipp + d < P:
                pts.add(i // ipp + d)
    return sorted(pts)


def check_plaintexts(s, db, pts):
    for pt in pts:
        assert np.array_equal(db.read_plaintext(pt), s.db_ntt[pt]), pt


def check_queries(s, srv, indexes, decode=True):
    for idx in indexes:
        q = s.client.create_query_for(s.params, idx)
        rc, exp = s.orc.process_query(s.db_ntt, s.params.dimensions, q, s.galois_keys)
        assert rc == 0
        got = srv.process_query(q)
        assert np.array_equal(got, exp), idx
        if decode:
            assert s.client.process_response(s.params, idx, got) == s.item(idx)


def check_batch_against_fresh(s, srv, indexes):
    queries = np.stack([s.client.create_query_for(s.params, i) for i in indexes])
    srv.stage_batch(queries)
    srv.run_batch()
    got = srv.fetch_batch()
    db2, srv2 = make(s)
    srv2.stage_batch(queries)
    srv2.run_batch()
    want = srv2.fetch_batch()
    db2.close()
    assert got.tobytes() == want.tobytes()


# (label, setup kwargs, digits, top digit as a nibble (None: whatever the moduli give), decode, PIRGPU_SCAN_MFMA_TOP4)
M8 = oracle.BFV_DEFAULT[8192]
M16 = oracle.BFV_DEFAULT[16384]
GEOMETRIES = [
    ("L5 TOP4 17x70", dict(short=2, elem=2048, dims=[17, 70], N=4096, plain_bits=24), 5, True, True, None),
    ("L5 byte top digit 17x70", dict(short=2, elem=2048, dims=[17, 70], N=4096, plain_bits=24), 5, False, True, "0"),
    ("L6 9x130 N=8192", dict(short=2, elem=1024, dims=[9, 130], N=8192, moduli=M8[:3] + [M8[4]],
                             t=oracle.plain_modulus_batching(8192, 24)), 6, None, True, None),
    ("L7 9x10 N=16384", dict(short=1, elem=288, dims=[9, 10], N=16384, moduli=M16[:4] + [M16[8]],
                             t=oracle.plain_modulus_batching(16384, 24)), 7, False, False, None),
]


@pytest.mark.parametrize("release", [False, True], ids=["staging kept", "staging released"])
@pytest.mark.parametrize("label,kw,digits,top4,decode,env", GEOMETRIES, ids=[g[0] for g in GEOMETRIES])
def test_update_items_mfma_geometries(label, kw, digits, top4, decode, env, release, monkeypatch):
    if env is not None:
        monkeypatch.setenv("PIRGPU_SCAN_MFMA_TOP4", env)
    kw = dict(kw)
    s = setup_with_dims(kw.pop("short"), kw.pop("elem"), kw.pop("dims"), **kw)
    p = s.params
    db, srv = make(s, release=release)
    info = srv.scan_info()
    assert info["mfma"] and info["digits"] == digits, info
    assert top4 is None or info["top_digit_nibble"] == top4, info
    check_queries(s, srv, [7], decode=decode)            # the operand layout is packed and in use
    idx = edge_indices(s, p.dimensions[-1])
    items = new_items(s, len(idx), 11)
    items[-1] = items[-1] ^ 0x5A                          # the duplicate's second value differs from its first
    db.update_items(idx, items)
    apply_to_raw(s, idx, items)
    check_plaintexts(s, db, touched_and_neighbours(s, idx))
    check_queries(s, srv, [0, p.num_items - 1, 3 * p.items_per_plaintext + 1, 5 * p.items_per_plaintext + 1,
                           4 * p.items_per_plaintext], decode=decode)
    n = p.num_items
    check_batch_against_fresh(s, srv, [idx[k % len(idx)] if k % 2 else (97 * k + 13) % n for k in range(8)])
    db.close()


@pytest.mark.parametrize("case", ["d1", "rows<8", "d3", "N8192"])
def test_update_items_other_scan_paths(case):
    if case == "d1":
        s, mfma = PirSetup(301, 2048, 1, N=4096, plain_bits=24), False
    elif case == "rows<8":
        s, mfma = PirSetup(101, 2048, 2, N=4096, plain_bits=24), False      # dims [5, 4]: the 64-bit scan
    elif case == "d3":
        s, mfma = setup_with_dims(1, 2048, [4, 4, 40], N=4096, plain_bits=20), True
    else:
        s, mfma = PirSetup(1203, 1024, 2, N=8192, plain_bits=24), None
    p = s.params
    db, srv = make(s, release=False)
    if mfma is not None:
        assert srv.scan_info()["mfma"] == mfma
    n, ipp = p.num_items, p.items_per_plaintext
    idx = sorted({0, n - 1, ipp, ipp + 1, (p.num_pt // 2) * ipp, n // 3})
    items = new_items(s, len(idx), 12)
    db.update_items(idx, items)
    apply_to_raw(s, idx, items)
    check_plaintexts(s, db, touched_and_neighbours(s, idx))
    check_queries(s, srv, idx[:3] + [ipp + 2])
    db.close()


def test_update_items_ring32k():
    m = oracle.coeff_modulus_create(32768, [49, 49, 49, 49, 50])
    s = PirSetup(21823, 288, 2, N=32768, plain_bits=24, moduli=m)
    p = s.params
    db, srv = make(s, release=True)
    idx = [0, 5, p.items_per_plaintext * 20 + 3, p.num_items - 1]
    items = new_items(s, len(idx), 13)
    db.update_items(idx, items)
    apply_to_raw(s, idx, items)
    check_plaintexts(s, db, [0, 1, 20, p.num_pt - 1])
    check_queries(s, srv, [5, p.items_per_plaintext * 20 + 3], decode=False)
    db.close()


@pytest.mark.parametrize("release", [False, True], ids=["staging kept", "staging released"])
def test_update_plaintexts_matches_db_from_coeffs(release):
    s = setup_with_dims(2, 2048, [17, 20], N=4096, plain_bits=24)
    p = s.params
    db, srv = make(s, release=release)
    rng = np.random.default_rng(14)
    pts = [0, 3, 5, 21, p.num_pt - 1, 3]
    rows = [rng.integers(0, p.t, size=p.N, dtype=np.uint64) for _ in pts]
    rows[2][p.N // 2:] = 0                                 # a short row (zero padded like populate_coeffs)
    db.update_plaintexts(pts, [r if i != 2 else r[: p.N // 2] for i, r in enumerate(rows)])
    new = s.db_ntt.copy()
    for pt, row in zip(pts, rows):                          # the later entry for plaintext 3 wins
        new[pt] = s.orc.db_from_coeffs([row])[0]
    s.db_ntt = new
    check_plaintexts(s, db, sorted(set(pts)) + [1, 4])
    check_queries(s, srv, [3 * p.items_per_plaintext, 7 * p.items_per_plaintext], decode=False)
    db.close()


def test_zero_plaintext_accounting():
    s = PirSetup(301, 2048, 2, N=4096, plain_bits=24)
    p = s.params
    ipp = p.items_per_plaintext
    db, srv = make(s, release=True)
    old = s.raw[3 * ipp: 4 * ipp].copy()
    zero = np.zeros((ipp, p.bytes_per_item), dtype=np.uint8)
    db.update_items(list(range(3 * ipp, 4 * ipp)), zero)
    apply_to_raw(s, range(3 * ipp, 4 * ipp), zero)
    fresh, _ = make(s)
    assert srv.zero_plaintexts() == 1 == int(fresh.lib.pirgpu_zero_plaintexts(fresh.handle))
    fresh.close()
    with pytest.raises(PirGpuError) as e:
        srv.check_ready()
    assert e.value.code == 13
    with pytest.raises(PirGpuError) as e:
        srv.process_query(s.client.create_query_for(p, 0))
    assert e.value.code == 13
    db.update_items(list(range(3 * ipp, 4 * ipp)), old)
    apply_to_raw(s, range(3 * ipp, 4 * ipp), old)
    assert srv.zero_plaintexts() == 0
    srv.check_ready()
    check_queries(s, srv, [3 * ipp + 1, 0])
    db.close()


def test_update_errors_change_nothing():
    s = PirSetup(301, 2048, 2, N=4096, plain_bits=24)
    p = s.params
    pp = to_product_params(p)
    empty = pir_amd.PIRDatabase.Create(pp)
    with pytest.raises(PirGpuError) as e:
        empty.update_items([0], new_items(s, 1, 1))
    assert e.value.code == 9
    with pytest.raises(PirGpuError) as e:
        empty.update_plaintexts([0], [np.zeros(p.N, dtype=np.uint64)])
    assert e.value.code == 9
    empty.close()
    db, srv = make(s, release=True)
    before = [db.read_plaintext(i) for i in range(3)]
    with pytest.raises(PirGpuError) as e:
        db.update_items([0, p.num_items], new_items(s, 2, 2))
    assert e.value.code == 3
    bad = np.zeros((1, p.bytes_per_item + 1), dtype=np.uint8)
    idx = np.zeros(1, dtype=np.uint64)
    rc = db.lib.pirgpu_db_update_items(db.handle, 1, idx.ctypes.data_as(pir_amd.capi.u64p),
                                       bad.ctypes.data_as(pir_amd.capi.u8p), p.bytes_per_item + 1)
    assert rc == 3
    row = np.zeros(p.N, dtype=np.uint64)
    row[5] = p.t
    with pytest.raises(PirGpuError) as e:
        db.update_plaintexts([0], [row])
    assert e.value.code == 3
    with pytest.raises(PirGpuError) as e:
        db.update_plaintexts([p.num_pt], [np.zeros(p.N, dtype=np.uint64)])
    assert e.value.code == 3
    db.update_items([], np.zeros((0, p.bytes_per_item), dtype=np.uint8))     # n = 0: no-op
    for i in range(3):
        assert np.array_equal(db.read_plaintext(i), before[i])
    check_queries(s, srv, [0])
    db.close()


def test_row_shards_take_the_same_full_list():
    from pir_amd import distributed as D
    s = PirSetup(300, 288, 2, N=4096, plain_bits=24)
    p = s.params
    world, count = 2, 4
    ranks = []
    for r in range(world):
        db, srv = make(s, release=True, shard=D.shard_range(p.dimensions[0], r, world))
        srv.set_concurrency(2)
        ranks.append((db, srv))
    idx = [0, 1, 150, 299, 151, 0]
    items = new_items(s, len(idx), 15)
    for db, srv in ranks:
        assert D.update_items(srv, idx, items, None, 1) == 0
    apply_to_raw(s, idx, items)
    indexes = [0, 150, 299, 7]
    queries = np.stack([s.client.create_query_for(p, i) for i in indexes])
    acc = None
    for db, srv in ranks:
        srv.stage_batch(queries)
        srv.run_batch()
        part = srv.fetch_batch()
        acc = part.copy() if acc is None else acc + part
    for j, qj in enumerate(s.orc.moduli[: s.orc.k]):
        acc[:, :, :, j, :] %= np.uint64(qj)
    for i, idx_i in enumerate(indexes):
        rc, exp = s.orc.process_query(s.db_ntt, p.dimensions, queries[i], s.galois_keys)
        assert rc == 0 and np.array_equal(acc[i], exp), i
        assert s.client.process_response(p, idx_i, acc[i]) == s.item(idx_i)
    for db, srv in ranks:
        db.close()


def _slots_step(srvs, s, queries, cuts, per):
    import torch
    from gpu_helpers import all_to_all_in_process
    from pir_amd import distributed as D
    G = len(srvs)
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
            rc, want = s.orc.process_query(s.db_ntt, s.params.dimensions, queries[g * per + i], s.galois_keys)
            assert rc == 0 and np.array_equal(mine[i], want), (g, i)


@pytest.mark.parametrize("release", [False, True], ids=["staging kept", "staging released"])
def test_slot_shards(release):
    from pir_amd import distributed as D
    s = PirSetup(3000, 288, 2, N=4096, plain_bits=24)
    p = s.params
    G, per = 2, 2
    cuts = D.slot_cuts(s.orc.k * p.N, G)
    srvs = [make(s, release=release, slots=(cuts[g], cuts[g + 1]))[1] for g in range(G)]
    for v in srvs:
        v.set_concurrency(16)
    idx = [0, 1, 2999, 1500]
    items = new_items(s, len(idx), 16)
    if release:
        for v in srvs:
            with pytest.raises(PirGpuError) as e:
                v.db.update_items(idx, items)
            assert e.value.code == 9
    else:
        for v in srvs:
            v.db.update_items(idx, items)
        apply_to_raw(s, idx, items)
    rng = np.random.default_rng(17)
    pts = [2, p.num_pt - 1]
    rows = [rng.integers(0, p.t, size=p.N, dtype=np.uint64) for _ in pts]
    for v in srvs:
        v.db.update_plaintexts(pts, rows)
    new = s.db_ntt.copy()
    for pt, row in zip(pts, rows):
        new[pt] = s.orc.db_from_coeffs([row])[0]
    s.db_ntt = new
    ipp = p.items_per_plaintext
    indexes = [0, 2 * ipp + 1, 1500, 2999]
    queries = np.stack([s.client.create_query_for(p, i) for i in indexes])
    _slots_step(srvs, s, queries, cuts, per)
    for v in srvs:
        v.db.close()


def test_update_between_begin_and_end():
    import seal_wire as W
    s = PirSetup(3000, 288, 2, N=4096, plain_bits=24)
    p, o = s.params, s.orc
    db, srv = make(s, release=True)
    gk = W.save_galois_keys(s.galois_keys, p.N, W.parms_id(p.N, o.moduli, o.t))
    pid = W.parms_id(p.N, o.moduli[: o.k], o.t)
    indexes = [5, 1500, 2999, 700, 5, 42]
    queries = [s.client.create_query_for(p, i) for i in indexes]
    requests = [W.save_request([q], gk, pid) for q in queries]
    old = s.db_ntt.copy()
    tok = srv.ProcessRequestsBegin(requests)
    idx = [5, 1500, 2999]
    items = new_items(s, len(idx), 18)
    db.update_items(idx, items)
    res = srv.ProcessRequestsEnd(tok)
    apply_to_raw(s, idx, items)
    for q, (rc, resp) in zip(queries, res):
        assert rc == 0
        got = W.load_response(resp)[0]
        _, want_old = o.process_query(old, p.dimensions, q, s.galois_keys)
        _, want_new = o.process_query(s.db_ntt, p.dimensions, q, s.galois_keys)
        assert np.array_equal(got, want_old) or np.array_equal(got, want_new)
    res = srv.ProcessRequests(requests[:3])
    for i, (q, (rc, resp)) in enumerate(zip(queries, res)):
        assert rc == 0
        got = W.load_response(resp)[0]
        _, want = o.process_query(s.db_ntt, p.dimensions, q, s.galois_keys)
        assert np.array_equal(got, want)
        assert s.client.process_response(p, indexes[i], got) == s.item(indexes[i])
    resp = srv.ProcessRequest(requests[3])
    assert np.array_equal(W.load_response(resp)[0], o.process_query(s.db_ntt, p.dimensions, queries[3], s.galois_keys)[1])
    db.close()
