"""Streamed database contexts (pirgpu_create_ex + PIRGPU_CREATE_STREAMED_DB, PIRDatabase(streamed=True)): loads go in row
bands straight into the scan's operand layout, the u64 staging copy is never allocated.  No reference counterpart; the
contract is that after a load the context is indistinguishable from a plain one that was populated and then given
finalize(release_staging=True) -- down to the bytes of the operand layout, padding included.

Expected values come from the oracle (orc.db_encode, orc.db_from_coeffs, orc.process_query) and from a plain
(non-streamed) context of the same parameters, never from the streamed path itself.  All comparisons are exact.  The
shapes are those of test_gpu_db_update.py: the smallest at which each digit count, the nibble top digit, a short last row
tile and a partial last plaintext occur."""
import numpy as np
import pytest

import oracle
import pir_amd
from gpu_helpers import to_product_params
from oracle.client import Client
from pir_amd import capi
from pir_amd import distributed as D
from pir_amd import parameters as P
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


def make(s, streamed, options=None, load=True, **create_kw):
    """Context (+ server with the setup's keys) of s.params; options are set before the first use; load: populate s.raw."""
    pp = to_product_params(s.params)
    db = pir_amd.PIRDatabase.Create(pp, streamed=streamed, **create_kw)
    for name, value in (options or {}).items():
        db.set_option(name, value)
    if load:
        db.populate(s.raw)
    srv = pir_amd.PIRServer(db, pp)
    srv.set_galois_keys(s.galois_keys)
    return db, srv


def operand(db, srv):
    n = srv.scan_bytes()
    assert db.memory()["operand"] == n
    return db.read_operand(0, n).tobytes()


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


def batch(srv, queries):
    srv.stage_batch(queries)
    srv.run_batch()
    return srv.fetch_batch().tobytes()


# (label, setup kwargs, digits, top digit as a nibble (None: whatever the moduli give), decode, option SCAN_MFMA_TOP4)
M8 = oracle.BFV_DEFAULT[8192]
M16 = oracle.BFV_DEFAULT[16384]
GEOMETRIES = [
    ("L5 TOP4 17x70", dict(short=2, elem=2048, dims=[17, 70], N=4096, plain_bits=24), 5, True, True, None),
    ("L5 byte top digit 17x70", dict(short=2, elem=2048, dims=[17, 70], N=4096, plain_bits=24), 5, False, True, 0),
    ("L6 9x130 N=8192", dict(short=2, elem=1024, dims=[9, 130], N=8192, moduli=M8[:3] + [M8[4]],
                             t=oracle.plain_modulus_batching(8192, 24)), 6, None, True, None),
    ("L7 9x10 N=16384", dict(short=1, elem=288, dims=[9, 10], N=16384, moduli=M16[:4] + [M16[8]],
                             t=oracle.plain_modulus_batching(16384, 24)), 7, False, False, None),
]
GEOM_IDS = [g[0] for g in GEOMETRIES]
_setups = {}


def geometry_setup(kw):
    """The oracle side of a geometry, computed once and left unchanged (the two 17x70 rows share it)."""
    key = repr(sorted(kw.items(), key=lambda e: e[0]))
    if key not in _setups:
        kw = dict(kw)
        _setups[key] = setup_with_dims(kw.pop("short"), kw.pop("elem"), kw.pop("dims"), **kw)
    return _setups[key]


def options_of(top4_option):
    """One band per chunk (a band of these shapes is 5 - 73 MB), so the last chunk is the short last row tile."""
    opts = {"DB_STREAM_MB": 1}
    if top4_option is not None:
        opts["SCAN_MFMA_TOP4"] = top4_option
    return opts


@pytest.mark.parametrize("label,kw,digits,top4,decode,top4_option", GEOMETRIES, ids=GEOM_IDS)
def test_operand_layout_is_identical_to_a_plain_context(label, kw, digits, top4, decode, top4_option):
    s = geometry_setup(kw)
    p = s.params
    rows, cols = p.dimensions
    opts = options_of(top4_option)
    db, srv = make(s, True, opts)
    info = srv.scan_info()
    assert info["mfma"] and info["single_query_mfma"] and info["digits"] == digits, info
    assert top4 is None or info["top_digit_nibble"] == top4, info
    mem = db.memory()
    assert mem["staging"] == 0 and mem["band"] == 16 * cols * s.orc.k * p.N * 8
    assert mem["band"] > 1 << 20 and rows % 16 in (1, 9)      # one band per chunk; the last band has 1 / 9 real rows
    plain_opts = {k: v for k, v in opts.items() if k != "DB_STREAM_MB"}
    pdb, psrv = make(s, False, plain_opts)
    pdb.finalize()
    assert psrv.scan_info() == info
    assert operand(db, srv) == operand(pdb, psrv)              # padding rows and columns included
    pdb.close()
    for r in (0, rows - 1):                                    # (the 9x10 matrix has no columns 15 and 16)
        check_plaintexts(s, db, [r * cols + c for c in sorted({0, 15, 16, cols - 1}) if c < cols])
    db.close()


@pytest.mark.parametrize("label,kw,digits,top4,decode,top4_option", GEOMETRIES, ids=GEOM_IDS)
def test_queries_and_a_batch(label, kw, digits, top4, decode, top4_option):
    s = geometry_setup(kw)
    p = s.params
    opts = options_of(top4_option)
    db, srv = make(s, True, opts)
    assert db.size() == p.num_pt
    srv.check_ready()
    check_queries(s, srv, [7, p.num_items - 1], decode=decode)
    n = p.num_items
    queries = np.stack([s.client.create_query_for(p, (97 * k + 13) % n) for k in range(8)])
    got = batch(srv, queries)
    db.close()
    pdb, psrv = make(s, False, {k: v for k, v in opts.items() if k != "DB_STREAM_MB"})
    want = batch(psrv, queries)
    pdb.close()
    assert got == want


def test_ragged_coefficient_loads_and_a_reload():
    s = geometry_setup(GEOMETRIES[0][1])
    p = s.params
    rows, cols = p.dimensions
    Pn = p.num_pt
    rng = np.random.default_rng(21)
    coeffs = rng.integers(0, p.t, size=(Pn, p.N), dtype=np.uint64)
    coeffs[7] = 0                                              # an identically zero plaintext
    cuts = [0, 5, cols + 3, 16 * cols, 16 * cols + 1, Pn]
    db, srv = make(s, True, {"DB_STREAM_MB": 1}, load=False)
    for lo, hi in reversed(list(zip(cuts[:-1], cuts[1:]))):
        assert db.size() == Pn - hi
        db.populate_coeffs(coeffs[lo:hi], first_pt=lo)
    assert db.size() == Pn
    pdb, psrv = make(s, False, load=False)
    pdb.populate_coeffs(coeffs)
    pdb.finalize()
    assert operand(db, srv) == operand(pdb, psrv)
    assert srv.zero_plaintexts() == psrv.zero_plaintexts() == 1
    want = s.orc.db_from_coeffs([coeffs[i] for i in (0, 4, 5, cols + 2, cols + 3, 16 * cols, Pn - 1)])
    for w, i in zip(want, (0, 4, 5, cols + 2, cols + 3, 16 * cols, Pn - 1)):
        assert np.array_equal(db.read_plaintext(i), w), i
    # a reload of one range with other values: a load overwrites, the neighbours in its row tiles survive
    lo, hi = 5, cols + 3
    new = rng.integers(0, p.t, size=(hi - lo, p.N), dtype=np.uint64)
    new[1] = 0                                                 # plaintext 6 becomes zero, 7 stops being zero
    db.populate_coeffs(new, first_pt=lo)
    pdb.populate_coeffs(new, first_pt=lo)
    pdb.finalize()
    assert operand(db, srv) == operand(pdb, psrv)
    assert srv.zero_plaintexts() == psrv.zero_plaintexts() == 1
    assert db.size() == Pn
    final = coeffs.copy()
    final[lo:hi] = new
    for w, i in zip(s.orc.db_from_coeffs([final[i] for i in (4, 5, 6, 7, hi - 1, hi)]), (4, 5, 6, 7, hi - 1, hi)):
        assert np.array_equal(db.read_plaintext(i), w), i
    pdb.close()
    db.close()


def test_row_shard_partial_reply():
    s = geometry_setup(GEOMETRIES[0][1])
    p = s.params
    db, srv = make(s, True, {"DB_STREAM_MB": 1}, shard=(5, 14))
    pdb, psrv = make(s, False, shard=(5, 14))
    pdb.finalize()
    assert db.memory()["staging"] == 0 and operand(db, srv) == operand(pdb, psrv)
    cols = p.dimensions[1]
    for pt in (5 * cols, 14 * cols - 1):                       # first and last plaintext of the shard
        assert np.array_equal(db.read_plaintext(pt), s.db_ntt[pt]), pt
    for idx in (0, 6 * cols * p.items_per_plaintext + 3, p.num_items - 1):
        q = s.client.create_query_for(p, idx)
        assert np.array_equal(srv.process_query(q), psrv.process_query(q)), idx
    pdb.close()
    db.close()


def _slots_step(srvs, s, queries, cuts, per):
    import torch
    from gpu_helpers import all_to_all_in_process
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


_slots_setup = []


@pytest.mark.parametrize("G", [2, 3])
def test_slot_shards(G):
    if not _slots_setup:
        _slots_setup.append(setup_with_dims(2, 2048, [17, 20], N=4096, plain_bits=24))
    s = _slots_setup[0]
    p = s.params
    per = 2 if G == 2 else 1
    kN = s.orc.k * p.N
    cuts = D.slot_cuts(kN, G)
    dbs, srvs = zip(*[make(s, True, {"DB_STREAM_MB": 1}, slots=(cuts[g], cuts[g + 1])) for g in range(G)])
    whole = None
    for g, (db, srv) in enumerate(zip(dbs, srvs)):
        srv.set_concurrency(16)
        mem = db.memory()                                      # only [slot0, slot0 + nslots) is packed
        assert mem["staging"] == 0 and mem["operand"] == srv.scan_bytes()
        whole = whole or mem["operand"] * kN // (cuts[g + 1] - cuts[g])
        assert mem["operand"] * kN == whole * (cuts[g + 1] - cuts[g])
    db_before = s.db_ntt
    if G == 2:
        # on a streamed slot shard update_plaintexts works (it needs no old content), update_items cannot
        items = np.random.default_rng(16).integers(0, 256, size=(2, p.bytes_per_item), dtype=np.uint8)
        rng = np.random.default_rng(17)
        pts = [2, p.num_pt - 1]
        rows = [rng.integers(0, p.t, size=p.N, dtype=np.uint64) for _ in pts]
        for db in dbs:
            with pytest.raises(PirGpuError) as e:
                db.update_items([0, 1500], items)
            assert e.value.code == 9
            with pytest.raises(PirGpuError) as e:
                db.read_plaintext(0)
            assert e.value.code == 9
            db.update_plaintexts(pts, rows)
        s.db_ntt = db_before.copy()
        for pt, w in zip(pts, s.orc.db_from_coeffs(rows)):
            s.db_ntt[pt] = w
    ipp = p.items_per_plaintext
    indexes = [0, 2 * ipp + 1, p.num_items - 1, 1500, 7, 20 * ipp][: G * per]
    queries = np.stack([s.client.create_query_for(p, i) for i in indexes])
    try:
        _slots_step(list(srvs), s, queries, cuts, per)
    finally:
        s.db_ntt = db_before                                   # the shared setup is left unchanged
        for db in dbs:
            db.close()


def edge_indices(s, cols):
    """The update list of test_gpu_db_update.py: first item, last item (in a partial last plaintext), two items of one
    plaintext, a duplicated index, the plaintexts in columns 2 and 6 of one 16-column group (one TOP4 nibble byte) and
    items whose bits share a coefficient with untouched neighbours."""
    p = s.params
    n, ipp = p.num_items, p.items_per_plaintext
    assert n % ipp, "the last plaintext must be partial"
    r = min(1, p.num_pt // cols - 1)
    pa, pb = r * cols + 2, r * cols + 6
    idx = [0, n - 1, 3 * ipp, 3 * ipp + 1, 5 * ipp + 1, pa * ipp + ipp // 2, pb * ipp, 5 * ipp + 1]
    return [i for i in idx if i < n]


def test_update_items_after_a_streamed_load():
    kw = dict(GEOMETRIES[0][1])
    s = setup_with_dims(kw.pop("short"), kw.pop("elem"), kw.pop("dims"), **kw)      # its own: the raw database changes
    p = s.params
    db, srv = make(s, True, {"DB_STREAM_MB": 1})
    idx = edge_indices(s, p.dimensions[-1])
    items = np.random.default_rng(11).integers(0, 256, size=(len(idx), p.bytes_per_item), dtype=np.uint8)
    items[-1] = items[-1] ^ 0x5A                          # the duplicate's second value differs from its first
    db.update_items(idx, items)
    for i, it in zip(idx, items):                         # a later entry wins, as in the library
        s.raw[i] = it
    rc, s.db_ntt = s.orc.db_encode(s.raw.tobytes(), p.num_items, p.bytes_per_item, p.items_per_plaintext,
                                   p.eff_bits_per_coeff, p.num_pt)
    assert rc == 0
    ipp = p.items_per_plaintext
    touched = sorted({i // ipp + d for i in idx for d in (-1, 0, 1) if 0 <= i // ipp + d < p.num_pt})
    check_plaintexts(s, db, touched)
    assert db.memory()["staging"] == 0
    check_queries(s, srv, [0, p.num_items - 1, 3 * ipp + 1, 5 * ipp + 1, 4 * ipp])
    n = p.num_items
    queries = np.stack([s.client.create_query_for(p, idx[k % len(idx)] if k % 2 else (97 * k + 13) % n)
                        for k in range(8)])
    got = batch(srv, queries)
    db.close()
    pdb, psrv = make(s, False)                            # a fresh plain context of the UPDATED raw database
    assert got == batch(psrv, queries)
    pdb.close()


def test_three_dimensions():
    s = setup_with_dims(1, 2048, [4, 4, 40], N=4096, plain_bits=20)
    p = s.params
    db, srv = make(s, True, {"DB_STREAM_MB": 1})
    info = srv.scan_info()
    assert info["mfma"] and (info["rows"], info["cols"]) == (16, 40), info
    pdb, psrv = make(s, False)
    pdb.finalize()
    assert operand(db, srv) == operand(pdb, psrv)
    pdb.close()
    check_plaintexts(s, db, [0, 39, 40, p.num_pt - 1])
    check_queries(s, srv, [0, p.num_items - 1, (p.num_pt // 2) * p.items_per_plaintext])
    db.close()


class WideSetup:
    """The `mfma` setup of test_gpu_wide_items.py: product parameters of a wide database + the `planes`
    one-plaintext-per-item oracle databases it must equal (B = 9 728, 19 bits, dims [10, 10], 3 planes: 30 scan rows,
    plane boundaries at rows 10 and 20 -- inside a row tile)."""

    def __init__(self, n_items=100, item_bytes=25000, d=2, N=4096, plain_bits=20, seed=5, client_seed=77):
        moduli = oracle.BFV_DEFAULT[N]
        t = oracle.plain_modulus_batching(N, plain_bits)
        self.pp = P.create_pir_parameters(n_items, item_bytes, d, P.EncryptionParams(N, list(moduli), t),
                                          max_plaintexts_per_item=8)
        self.op = oracle.create_pir_parameters(n_items, 0, d, N=N, plain_bits=plain_bits, moduli=list(moduli), t=t)
        assert list(self.op.dimensions) == list(self.pp.dimensions) and self.op.num_pt == self.pp.num_pt == n_items
        self.B, self.bits, self.planes = self.op.bytes_per_item, self.op.eff_bits_per_coeff, self.pp.planes
        self.n = n_items
        self.orc = oracle.Oracle.from_params(self.op)
        self.R = self.orc.reply_ct_count(d)
        self.raw = np.random.default_rng(seed).integers(0, 256, size=(n_items, item_bytes), dtype=np.uint8)
        self.db = []
        for j in range(self.planes):
            c = np.ascontiguousarray(self.raw[:, j * self.B:min((j + 1) * self.B, item_bytes)])
            rc, db = self.orc.db_encode(c.tobytes(), n_items, c.shape[1], 1, self.bits, n_items)
            assert rc == 0
            self.db.append(db)
        self.client = Client(self.orc, seed=client_seed)
        self.keys = self.client.galois_keys()


def test_wide_items():
    s = WideSetup()
    assert (s.planes, s.B, s.bits, list(s.pp.dimensions)) == (3, 9728, 19, [10, 10])
    db = pir_amd.PIRDatabase.Create(s.pp, streamed=True)
    db.set_option("DB_STREAM_MB", 1)
    db.populate(s.raw)
    srv = pir_amd.PIRServer.Create(db, s.pp)
    srv.set_galois_keys(s.keys)
    info = srv.scan_info()
    assert info["mfma"] and info["rows"] == 30 and info["cols"] == 10, info
    pdb = pir_amd.PIRDatabase.Create(s.pp, s.raw)
    pdb.finalize()
    psrv = pir_amd.PIRServer.Create(pdb, s.pp)
    assert db.memory()["staging"] == 0 and operand(db, srv) == operand(pdb, psrv)
    pdb.close()
    for j in range(s.planes):
        for i in (0, 9, 10, s.n - 1):
            assert np.array_equal(db.read_plaintext(j * s.n + i), s.db[j][i]), (j, i)
    for i in (0, 57, s.n - 1):
        q = s.client.create_query_for(s.op, i)
        got = srv.process_query(q)
        assert got.shape[0] == s.planes * s.R
        for j in range(s.planes):                              # plane by plane against the oracle
            rc, want = s.orc.process_query(s.db[j], s.op.dimensions, q, s.keys)
            assert rc == 0 and np.array_equal(got[j * s.R:(j + 1) * s.R], want), (i, j)
    db.close()


def test_ring32k():
    m = oracle.coeff_modulus_create(32768, [49, 49, 49, 49, 50])
    s = PirSetup(21823, 288, 2, N=32768, plain_bits=24, moduli=m)
    p = s.params
    db, srv = make(s, True)
    assert srv.scan_info()["mfma"] and db.memory()["staging"] == 0
    check_plaintexts(s, db, [0, 1, 20, p.num_pt - 1])
    check_queries(s, srv, [p.items_per_plaintext * 20 + 3], decode=False)
    db.close()


def test_memory_accounting():
    s = setup_with_dims(2, 2048, [80, 32], N=4096, plain_bits=24)
    p = s.params
    staging, operand_bytes, band = 2560 * 2 * 4096 * 8, 5 * 2 * 1152 * 8192, 16 * 32 * 65536
    assert (staging, operand_bytes, band) == (167772160, 94371840, 33554432)
    db, srv = make(s, True, {"DB_STREAM_MB": 1}, load=False)

    def check():
        mem = db.memory()
        assert mem["staging"] == 0, mem
        assert mem["operand"] == srv.scan_bytes() == operand_bytes, mem
        assert mem["band"] == band, mem
        assert mem["peak"] <= mem["operand"] + band + (16 << 20), mem
        assert mem["peak"] < staging, mem
        return mem

    check()
    db.populate(s.raw)
    after = check()
    raw_chunk = 16 * 32 * p.items_per_plaintext * p.bytes_per_item            # 6.3 MB: one band of raw bytes
    assert after["peak"] >= operand_bytes + band + raw_chunk, after           # the chunk really was counted
    check_queries(s, srv, [p.items_per_plaintext * 1234 + 1])
    db.close()
    pdb, psrv = make(s, False)
    pdb.finalize()
    mem = pdb.memory()
    assert mem["staging"] == staging and mem["operand"] == operand_bytes and mem["band"] == 0, mem
    assert mem["peak"] >= staging + operand_bytes, mem
    pdb.finalize(release_staging=True)
    mem2 = pdb.memory()
    assert mem2["staging"] == 0 and mem2["operand"] == operand_bytes and mem2["peak"] == mem["peak"], mem2
    pdb.close()


def test_refusals():
    pp2 = to_product_params(oracle.create_pir_parameters(300, 288, 1, N=4096, plain_bits=24))
    with pytest.raises(PirGpuError) as e:
        pir_amd.PIRDatabase.Create(pp2, streamed=True)                          # d = 1 scans the staging copy
    assert e.value.code == capi.INVALID_ARGUMENT
    # the int8 scan is off: create succeeds, the first load is refused before anything is allocated for the database
    small = PirSetup(101, 2048, 2, N=4096, plain_bits=24)                       # dims [5, 4]: the 64-bit scan
    s = _slots_setup[0] if _slots_setup else setup_with_dims(2, 2048, [17, 20], N=4096, plain_bits=24)
    for setup, opts in ((small, {}), (s, {"SCAN_MFMA": 0})):
        db, srv = make(setup, True, opts, load=False)
        with pytest.raises(PirGpuError) as e:
            db.populate(setup.raw)
        assert e.value.code == capi.FAILED_PRECONDITION and "int8" in e.value.message
        with pytest.raises(PirGpuError) as e:
            db.populate_coeffs([np.ones(4, dtype=np.uint64)])
        assert e.value.code == capi.FAILED_PRECONDITION
        assert not srv.scan_info()["mfma"]
        mem = db.memory()
        assert mem["operand"] == 0 and mem["staging"] == 0 and mem["peak"] == 0 and db.size() == 0, mem
        with pytest.raises(PirGpuError) as e:
            db.read_operand(0, 16)
        assert e.value.code == capi.FAILED_PRECONDITION
        db.close()
    p = s.params
    db, srv = make(s, True, {"DB_STREAM_MB": 1}, load=False)
    with pytest.raises(PirGpuError) as e:
        db.read_plaintext(0)
    assert e.value.code == capi.FAILED_PRECONDITION
    db.populate_coeffs(np.ones((5, p.N), dtype=np.uint64))                      # a first, partial load
    with pytest.raises(PirGpuError) as e:
        db.set_option("DB_STREAM_MB", 2)
    assert e.value.code == capi.FAILED_PRECONDITION
    q = s.client.create_query_for(p, 0)
    for call in (lambda: srv.process_query(q), srv.check_ready, db.finalize,
                 lambda: db.update_plaintexts([0], [np.ones(p.N, dtype=np.uint64)])):
        with pytest.raises(PirGpuError) as e:                                   # not fully loaded, as on a plain context
            call()
        assert e.value.code == capi.FAILED_PRECONDITION
    db.populate(s.raw)                                                          # the full load overwrites the partial one
    before = db.memory()
    db.finalize(True)
    db.finalize(False)
    assert db.memory() == before                                                # succeeds, frees nothing
    db.populate(s.raw)                                                          # and, unlike after a release: reloads
    check_queries(s, srv, [3])
    with pytest.raises(PirGpuError) as e:
        db.read_operand(before["operand"] - 8, 16)
    assert e.value.code == capi.INVALID_ARGUMENT
    db.close()
