"""Wide items on the GPU: an item of up to planes x B bytes (B = N * bits_per_coeff / 8) is stored as `planes` plaintexts,
one per plane, and one query is answered on all planes.  No reference counterpart (CreatePIRParameters refuses such an
item, parameters.cpp:81-85); the contract is that PLANE j BEHAVES AS ITS OWN REFERENCE DATABASE: reply ciphertexts
[j R, (j + 1) R) are bit-identical to the oracle's processQuery on the database made of chunk j of every item, with the
same query and keys.  The oracle is run plane by plane on databases this file builds itself.

Every case below was first checked on the CPU with the oracle alone: the oracle's client recovers the item from the
per-plane oracle replies (positive noise budget on every reply ciphertext)."""
import ctypes as C

import numpy as np
import pytest

import oracle
import pir_amd
from oracle.client import Client
from pir_amd import capi
from pir_amd import parameters as P
from pir_amd.server import PirGpuError

pytestmark = pytest.mark.gpu

N32K = 32768


class WideSetup:
    """Product parameters of a wide database + the `planes` one-plaintext-per-item oracle databases it must equal."""

    def __init__(self, n_items, item_bytes, d, N=4096, plain_bits=24, moduli=None, seed=5, client_seed=77,
                 max_planes=8):
        if moduli is None:
            moduli = oracle.BFV_DEFAULT[N]
        t = oracle.plain_modulus_batching(N, plain_bits)
        enc = P.EncryptionParams(N, list(moduli), t)
        self.pp = P.create_pir_parameters(n_items, item_bytes, d, enc, max_plaintexts_per_item=max_planes)
        # one plane = the reference's database of n_items one-plaintext items (bytes_per_item = 0: a full plaintext each)
        self.op = oracle.create_pir_parameters(n_items, 0, d, N=N, plain_bits=plain_bits, moduli=list(moduli), t=t)
        assert list(self.op.dimensions) == list(self.pp.dimensions) and self.op.num_pt == self.pp.num_pt == n_items
        self.B = self.op.bytes_per_item
        assert self.B == self.pp.max_bytes_per_plaintext
        self.bits = self.op.eff_bits_per_coeff
        self.planes = self.pp.planes
        self.n, self.item_bytes = n_items, item_bytes
        self.transparent_ok = False
        self.orc = oracle.Oracle.from_params(self.op)
        self.R = self.orc.reply_ct_count(d)
        self.raw = np.random.default_rng(seed).integers(0, 256, size=(n_items, item_bytes), dtype=np.uint8)
        self.encode()
        self.client = Client(self.orc, seed=client_seed)
        self.keys = self.client.galois_keys()

    def chunk(self, j):
        return self.raw[:, j * self.B:min((j + 1) * self.B, self.item_bytes)]

    def encode(self):
        """db_plane_j = StringEncoder + plain lift + NTT of chunk j of every item (orc.db_encode with one item per
        plaintext is orc.db_from_coeffs(string_encode(chunk)) for every item)."""
        self.db = []
        for j in range(self.planes):
            c = np.ascontiguousarray(self.chunk(j))
            rc, db = self.orc.db_encode(c.tobytes(), self.n, c.shape[1], 1, self.bits, self.n)
            assert rc == 0
            self.db.append(db)

    def query(self, index, client=None):
        return (client or self.client).create_query_for(self.op, index)

    def expected(self, query, keys=None):
        parts = []
        for j in range(self.planes):
            rc, rep = self.orc.process_query(self.db[j], self.op.dimensions, query, keys or self.keys)
            # (a plane with an all-zero plaintext: the oracle reports the reference's "transparent" failure, Internal,
            # and still hands out the mathematically defined reply -- what the transparent policy returns)
            assert (rc == 0 or (rc == capi.INTERNAL and self.transparent_ok)) and rep.shape[0] == self.R
            parts.append(rep)
        return np.concatenate(parts)

    def recover(self, reply, client=None):
        """The oracle's client on each plane's ciphertexts, chunks joined."""
        out = b""
        for j in range(self.planes):
            pt = (client or self.client).process_reply(self.op, reply[j * self.R:(j + 1) * self.R])
            rc, data = oracle.string_decode(pt, self.bits, self.chunk(j).shape[1], 0)
            assert rc == 0
            out += data
        return out

    def server(self, release=None, **create_kw):
        db = pir_amd.PIRDatabase.Create(self.pp, self.raw, **create_kw)
        if release is not None:
            db.finalize(release_staging=release)
        srv = pir_amd.PIRServer.Create(db, self.pp)
        srv.set_galois_keys(self.keys)
        return db, srv

    def check_plaintexts(self, db, items=None):
        for j in range(self.planes):
            for i in (range(self.n) if items is None else items):
                assert np.array_equal(db.read_plaintext(j * self.n + i), self.db[j][i]), (j, i)

    def check_queries(self, srv, indexes):
        for i in indexes:
            q = self.query(i)
            got = srv.process_query(q)
            assert got.shape[0] == self.planes * self.R
            assert np.array_equal(got, self.expected(q)), i
            assert self.recover(got) == self.raw[i].tobytes(), i


_cache = {}


def setup(name):
    if name not in _cache:
        _cache[name] = {
            # the issue's base case: B = 11 776, 23 bits, dims [5, 4], 8 reply ciphertexts per plane
            "base": lambda: WideSetup(20, 30000, 2, N=4096, plain_bits=24),
            # MFMA geometry: B = 9 728, 19 bits, dims [10, 10]: 30 scan rows, the last chunk's tail (5 544 bytes) ends
            # inside a coefficient
            "mfma": lambda: WideSetup(100, 25000, 2, N=4096, plain_bits=20),
            "d1": lambda: WideSetup(6, 20000, 1, N=4096, plain_bits=24),
            "d3": lambda: WideSetup(12, 15000, 3, N=4096, plain_bits=20),
            "n8192": lambda: WideSetup(30, 40000, 2, N=8192, plain_bits=24),
            "n32768": lambda: WideSetup(12, 150000, 2, N=N32K, plain_bits=24,
                                        moduli=oracle.coeff_modulus_create(N32K, [49, 49, 49, 49, 50])),
        }[name]()
    return _cache[name]


# ---------------------------------------------------------------- base case

def test_base_case_plaintexts_replies_and_wire_round_trip():
    s = setup("base")
    assert (s.planes, s.B, s.bits, list(s.pp.dimensions), s.R) == (3, 11776, 23, [5, 4], 8)
    db, srv = s.server()
    try:
        assert db.planes() == 3 and db.size() == 60 and db.reply_ct_count() == 24
        s.check_plaintexts(db)
        s.check_queries(srv, [0, 13, 19])
        # staged / asynchronous form of the same query
        q = s.query(7)
        srv.stage_query(q)
        srv.run_staged()
        assert np.array_equal(srv.fetch_reply(), s.expected(q))
        # wire path with the product's own client: request -> response -> the original 30 000 bytes
        client = pir_amd.PIRClient.Create(s.pp, seed=b"wide")
        assert client.reply_ct_count == 24
        idx = [0, 13, 19]
        response = srv.ProcessRequest(client.CreateRequest(idx))
        assert client.ProcessResponse(idx, response) == [s.raw[i].tobytes() for i in idx]
        replies = client.LoadResponse(response)
        assert replies.shape[:2] == (3, 24)
        # residue level through the product client: [planes, N] coefficients
        srv.set_galois_keys(client.galois_keys())
        reply = srv.process_query(client.create_query_for(13))
        pts = client.process_reply(reply)
        assert pts.shape == (3, 4096)
        for j in range(3):
            c = s.chunk(j)[13].tobytes()
            assert client.string_decode(pts[j], len(c), 0) == c
        # a response with a ciphertext missing: InvalidArgument from the client
        import seal_wire
        enc = s.pp.encryption_parameters
        pid = seal_wire.parms_id(4096, enc.coeff_modulus[:-1], enc.plain_modulus)
        assert client.ProcessResponse(idx, seal_wire.save_response(list(replies), pid)) == \
            [s.raw[i].tobytes() for i in idx]               # the re-serialized response is a good one ...
        short = seal_wire.save_response([replies[0], replies[1][:-1], replies[2]], pid)
        with pytest.raises(PirGpuError) as e:               # ... and with 23 ciphertexts in one reply it is refused
            client.ProcessResponse(idx, short)
        assert e.value.code == capi.INVALID_ARGUMENT and "does not match expected" in e.value.message
    finally:
        db.close()


# ---------------------------------------------------------------- MFMA scan geometry

def test_mfma_scan_runs_over_planes_times_rows():
    s = setup("mfma")
    assert (s.planes, s.B, s.bits, list(s.pp.dimensions)) == (3, 9728, 19, [10, 10])
    assert s.item_bytes - 2 * s.B == 5544 and (5544 * 8) % 19
    db, srv = s.server()
    try:
        info = srv.scan_info()
        assert info["mfma"] and info["rows"] == 30 and info["cols"] == 10, info
        s.check_plaintexts(db)
        s.check_queries(srv, [0, 57, 99])
    finally:
        db.close()


# ---------------------------------------------------------------- other depths and rings

@pytest.mark.parametrize("name,planes,indexes", [("d1", 2, [0, 5]), ("d3", 2, [0, 7, 11]), ("n8192", 2, [0, 29]),
                                                 ("n32768", 2, [0, 11])])
def test_other_depths_and_rings(name, planes, indexes):
    s = setup(name)
    assert s.planes == planes
    db, srv = s.server()
    try:
        s.check_plaintexts(db)
        s.check_queries(srv, indexes)
    finally:
        db.close()


# ---------------------------------------------------------------- batches

@pytest.mark.parametrize("name", ["mfma", "d1"])
def test_batches_equal_single_queries(name):
    s = setup(name)
    db, srv = s.server()
    try:
        srv.set_concurrency(16)
        for count in (8, 11):                       # one group; two groups
            idx = [(17 * i + 3) % s.n for i in range(count)]
            queries = np.stack([s.query(i) for i in idx])
            got = srv.process_batch(queries)
            assert got.shape[:2] == (count, s.planes * s.R)
            for b, i in enumerate(idx):
                assert np.array_equal(got[b], srv.process_query(queries[b])), (count, b)
            assert np.array_equal(got[0], s.expected(queries[0]))
            assert np.array_equal(got[-1], s.expected(queries[-1]))
            assert s.recover(got[-1]) == s.raw[idx[-1]].tobytes()
    finally:
        db.close()


def test_two_clients_key_sets_in_one_group():
    s = setup("mfma")
    other = Client(s.orc, seed=1234)
    other_keys = other.galois_keys()
    db, srv = s.server()
    try:
        srv.set_concurrency(16)
        slots = [srv.install_keyset(b"client-a", s.keys), srv.install_keyset(b"client-b", other_keys)]
        idx = [3, 98, 41, 0, 77, 12, 50, 99]
        who = [0, 1, 1, 0, 1, 0, 0, 1]
        clients, keys = [s.client, other], [s.keys, other_keys]
        queries = np.stack([s.query(i, clients[w]) for i, w in zip(idx, who)])
        srv.stage_batch(queries)
        srv.set_batch_keysets([slots[w] for w in who])
        srv.run_batch()
        got = srv.fetch_batch()
        for b in (0, 1, 7):
            assert np.array_equal(got[b], s.expected(queries[b], keys[who[b]])), b
        for b, (i, w) in enumerate(zip(idx, who)):
            assert s.recover(got[b], clients[w]) == s.raw[i].tobytes(), b
    finally:
        db.close()


def test_wire_requests_of_several_clients_through_the_pipeline():
    """pirgpu_process_requests: windows, two lanes, per-client key sets -- with 3 x the usual reply per query."""
    s = setup("mfma")
    db, srv = s.server()
    try:
        clients = [pir_amd.PIRClient.Create(s.pp, seed=b"wire-%d" % c) for c in range(3)]
        idx = [[0, 99, 5, 6, 7, 8, 9, 10, 11], [42], [13, 14, 15, 16, 17, 18, 19, 20, 21, 22]]
        responses = srv.ProcessRequests([c.CreateRequest(i) for c, i in zip(clients, idx)])
        for c, i, (status, r) in zip(clients, idx, responses):
            assert status == 0, srv.request_errors
            assert c.ProcessResponse(i, r) == [s.raw[x].tobytes() for x in i]
    finally:
        db.close()


# ---------------------------------------------------------------- updates

@pytest.mark.parametrize("release", [False, True], ids=["staging kept", "staging released"])
@pytest.mark.parametrize("which", [[57], [0, 99, 42, 43, 42]], ids=["one item", "several items"])
def test_update_items_equals_fresh_populate(which, release):
    s = WideSetup(100, 25000, 2, N=4096, plain_bits=20)      # its own copy: the raw database is modified
    s.client, s.keys = setup("mfma").client, setup("mfma").keys
    db, srv = s.server(release=release)
    try:
        assert srv.scan_info()["mfma"]
        s.check_queries(srv, [42])
        items = np.random.default_rng(len(which)).integers(0, 256, size=(len(which), s.item_bytes), dtype=np.uint8)
        if len(which) > 1:
            items[1, s.B:2 * s.B] = 0                        # plane 1 of item 99 becomes an all-zero plaintext
        db.update_items(which, items)
        for i, it in zip(which, items):                      # a later entry wins
            s.raw[i] = it
        s.encode()
        s.check_plaintexts(db)
        zeros = 1 if len(which) > 1 else 0
        assert srv.zero_plaintexts() == zeros
        assert db.size() == 300
        if zeros:
            with pytest.raises(PirGpuError) as e:
                srv.process_query(s.query(0))
            assert e.value.code == capi.INTERNAL
            db.set_transparent_policy(True)
            s.transparent_ok = True
        s.check_queries(srv, sorted(set(which)) + [1])
        # ... and equal to a context populated from scratch with the updated data, batch path included
        queries = np.stack([s.query(i) for i in (which[0], 1, 98)])
        got = srv.process_batch(queries)
        db2, srv2 = s.server()
        try:
            assert srv2.zero_plaintexts() == zeros
            if zeros:
                db2.set_transparent_policy(True)
            assert got.tobytes() == srv2.process_batch(queries).tobytes()
        finally:
            db2.close()
    finally:
        db.close()


def test_update_plaintexts_and_load_coeffs_use_plane_major_indices():
    s = WideSetup(20, 30000, 2, N=4096, plain_bits=24)
    s.client, s.keys = setup("base").client, setup("base").keys
    db = pir_amd.PIRDatabase.Create(s.pp)
    try:
        # populate through the coefficient path: plaintext plane * num_pt + i = string_encode(chunk_plane(item_i))
        rows = []
        for j in range(s.planes):
            for i in range(s.n):
                rc, co = oracle.string_encode(s.chunk(j)[i].tobytes(), s.bits, 4096)
                assert rc == 0
                rows.append(co)
        db.populate_coeffs(rows[:25], 0)                     # a range that crosses the plane boundary at 20
        db.populate_coeffs(rows[25:], 25)
        assert db.size() == 60
        s.check_plaintexts(db)
        srv = pir_amd.PIRServer.Create(db, s.pp)
        srv.set_galois_keys(s.keys)
        s.check_queries(srv, [13])
        # replace plane 2 of item 4 and plane 0 of item 19
        new = np.random.default_rng(3).integers(0, 1 << s.bits, size=(2, 4096), dtype=np.uint64)
        db.update_plaintexts([2 * s.n + 4, 19], list(new))
        want = s.orc.db_from_coeffs(list(new))
        assert np.array_equal(db.read_plaintext(2 * s.n + 4), want[0])
        assert np.array_equal(db.read_plaintext(19), want[1])
        s.db[2][4], s.db[0][19] = want[0], want[1]
        q = s.query(4)
        assert np.array_equal(srv.process_query(q), s.expected(q))
        with pytest.raises(PirGpuError) as e:
            db.read_plaintext(60)
        assert e.value.code == capi.INVALID_ARGUMENT
    finally:
        db.close()


# ---------------------------------------------------------------- planes = 1 through the new field

def test_planes_one_and_zero_equal_the_context_without_the_field():
    enc = P.generate_encryption_params(4096, 24)
    pp = P.create_pir_parameters(3000, 288, 2, enc)
    raw = np.random.default_rng(42).integers(0, 256, size=(3000, 288), dtype=np.uint8)
    client = pir_amd.PIRClient.Create(pp, seed=b"p1")
    keys = client.galois_keys()
    queries = np.stack([client.create_query_for(i) for i in (0, 1733, 2999)])
    replies = []
    for field in (None, 1, 0):
        db = pir_amd.PIRDatabase.__new__(pir_amd.PIRDatabase)     # PIRDatabase.__init__ with the struct set by hand
        cp = capi.make_params(pp)
        if field is not None:
            cp.plaintexts_per_item = field
        db.params, db.N, db.k, db.lib, db._cparams, db._h = pp, 4096, 2, capi.load(), cp, C.c_void_p()
        assert db.lib.pirgpu_create(C.byref(cp), C.byref(db._h)) == 0, db.lib.pirgpu_create_error()
        try:
            assert db.planes() == 1
            db.populate(raw)
            srv = pir_amd.PIRServer.Create(db, pp)
            srv.set_galois_keys(keys)
            single = srv.process_query(queries[1])
            batch = srv.process_batch(queries, n_workers=16)
            assert np.array_equal(batch[1], single)
            replies.append((single.tobytes(), batch.tobytes(), db.read_plaintext(74).tobytes()))
        finally:
            db.close()
    assert replies[0] == replies[1] == replies[2]


# ---------------------------------------------------------------- refusals

def _create_rc(cp):
    lib = capi.load()
    h = C.c_void_p()
    rc = lib.pirgpu_create(C.byref(cp), C.byref(h))
    msg = lib.pirgpu_create_error().decode()
    if rc == 0:
        lib.pirgpu_destroy(h)
    return rc, msg


def test_wide_refuses_shards_and_inconsistent_sizes():
    s = setup("mfma")
    with pytest.raises(PirGpuError) as e:
        pir_amd.PIRDatabase(s.pp, shard=(0, 5))
    assert e.value.code == capi.INVALID_ARGUMENT and "shard" in str(e.value)
    with pytest.raises(PirGpuError) as e:
        pir_amd.PIRDatabase(s.pp, slots=(0, 4096))
    assert e.value.code == capi.INVALID_ARGUMENT and "shard" in str(e.value)
    for planes, bpi, ipp in [(3, 2 * s.B, 1),        # fits two planes
                             (3, 3 * s.B + 1, 1),    # needs four
                             (2, 25000, 1),          # needs three
                             (3, 25000, 2)]:         # several items per plaintext
        cp = capi.make_params(s.pp)
        cp.plaintexts_per_item, cp.bytes_per_item, cp.items_per_plaintext = planes, bpi, ipp
        rc, msg = _create_rc(cp)
        assert rc == capi.INVALID_ARGUMENT, (planes, bpi, ipp, rc, msg)
    cp = capi.make_params(s.pp)                      # exactly planes x B is fine
    cp.bytes_per_item = 3 * s.B
    assert _create_rc(cp)[0] == 0


def test_multi_gpu_entry_points_refuse_a_wide_context():
    import torch
    s = setup("mfma")
    db, srv = s.server()
    try:
        srv.set_concurrency(16)
        assert srv.packed_selector_bytes() == 0 and srv.slots_packed_bytes(16) == 0
        queries = np.stack([s.query(i) for i in range(8)])
        srv.stage_batch(queries)
        buf = torch.zeros(1 << 20, dtype=torch.int64, device="cuda")
        p = buf.data_ptr()
        kN = 2 * 4096
        for call in (lambda: srv.batch_expand_packed(0, 8, p, p, [0, 10]),
                     lambda: srv.batch_expand_packed_async(0, 8, p, p, [0, 10]),
                     lambda: srv.batch_run_packed(p, 1, 8, p),
                     lambda: srv.slots_expand_async(0, 8, p, p, [0, kN]),
                     lambda: srv.slots_scan_async(p, 1, 8, p),
                     lambda: srv.slots_finish_async(p, 8, p, [0, kN], p)):
            with pytest.raises(PirGpuError) as e:
                call()
            assert e.value.code == capi.FAILED_PRECONDITION, e.value
            assert "wide items" in str(e.value)
        # the context still serves ordinary batches afterwards
        srv.run_batch()
        assert np.array_equal(srv.fetch_batch()[3], s.expected(queries[3]))
    finally:
        db.close()
