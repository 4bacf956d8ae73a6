"""Wide items in ciphertext-multiplication mode, and the shared-selector path (option CT_SHARED_SEL, counter CT_LIFTS;
DESIGN.md sections 6.2 and 6.6).  The contract is that PLANE j BEHAVES AS ITS OWN DATABASE IN THIS MODE: reply ciphertext
j of `planes` is bit-identical to the mode's reply -- tests/ctmult_model.py::process_query_ct, or with deferred rounding
tests/ctmult_deferred_model.py::process_query_ct_deferred -- on the database made of chunk j of every item, with the same
query, Galois keys and relinearisation key.  The models are run plane by plane on databases this file builds itself; the
zero plaintexts that pad a plane to the box of its dimensions do not exist for them.

The shared-selector path is exact modular arithmetic on the same canonical residues as the four-polynomial path: every
comparison of the two is a comparison of bits.

Every case that creates a wide context of the mode fails without the feature (InvalidArgument at create), the others on
the options CT_SHARED_SEL and CT_LIFTS, which do not exist there."""
import numpy as np
import pytest

import ctmult_deferred_model as D
import ctmult_model as M
import oracle
import pir_amd
import test_gpu_ctmult as T
from oracle.client import Client
from pir_amd import capi
from pir_amd import parameters as P
from pir_amd.server import PirGpuError

pytestmark = pytest.mark.gpu

FORMS = pytest.mark.parametrize("deferred", [False, True], ids=["per-child", "deferred"])


class WideCt:
    """Product parameters of a wide database of the mode + the `planes` one-plaintext-per-item databases it must equal."""

    def __init__(self, n_items, item_bytes, d, N=4096, plain_bits=16, bpc=0, moduli=None, seed=5, client_seed=77):
        moduli = [int(x) for x in (oracle.BFV_DEFAULT[N] if moduli is None else moduli)]
        t = oracle.plain_modulus_batching(N, plain_bits)
        self.enc = P.EncryptionParams(N, moduli, t)
        self.pp = P.create_pir_parameters(n_items, item_bytes, d, self.enc, True, bpc, max_plaintexts_per_item=8)
        # one plane = a database of n_items one-plaintext items (bytes_per_item = 0: a full plaintext each)
        self.op = oracle.create_pir_parameters(n_items, 0, d, N=N, plain_bits=plain_bits, moduli=moduli, t=t,
                                               use_ciphertext_multiplication=True, bits_per_coeff_=bpc)
        assert list(self.op.dimensions) == list(self.pp.dimensions) and self.op.num_pt == self.pp.num_pt == n_items
        self.B, self.bits = self.op.bytes_per_item, self.op.eff_bits_per_coeff
        assert self.B == self.pp.max_bytes_per_plaintext
        self.planes, self.n, self.item_bytes = self.pp.planes, n_items, item_bytes
        self.orc = oracle.Oracle.from_params(self.op)
        self.k = self.orc.k
        self.raw = np.random.default_rng(seed).integers(0, 256, size=(n_items, item_bytes), dtype=np.uint8)
        self.encode()
        self.client = Client(self.orc, seed=client_seed)
        self.keys = self.client.galois_keys()
        self.rk = M.relin_key(self.client)
        self._want = {}

    def chunk(self, j):
        return self.raw[:, j * self.B:min((j + 1) * self.B, self.item_bytes)]

    def encode(self):
        self.db = []
        for j in range(self.planes):
            c = np.ascontiguousarray(self.chunk(j))
            rc, db = self.orc.db_encode(c.tobytes(), self.n, c.shape[1], 1, self.bits, self.n)
            assert rc == 0
            self.db.append(db)

    def query(self, index, client=None):
        """One query per (index, client): encryption is randomised, and the model must answer the query the GPU got."""
        client = client or self.client
        made = client.__dict__.setdefault("_wide_ct_queries", {})      # (kept on the client: it lives as long as its keys)
        if (id(self), index) not in made:
            made[id(self), index] = client.create_query_for(self.op, index)
        return made[id(self), index]

    def expected(self, index, deferred):
        """The model's reply to query(index), plane by plane -> [planes][2][k][N]; computed once and left unchanged."""
        if (index, deferred) not in self._want:
            model = D.process_query_ct_deferred if deferred else M.process_query_ct
            parts = []
            for j in range(self.planes):
                rc, rep = model(self.orc, self.db[j], self.op.dimensions, self.query(index), self.keys, self.rk)
                assert rc == 0 and rep.shape == (1, 2, self.k, self.orc.N)
                parts.append(rep)
            want = np.concatenate(parts)
            want.setflags(write=False)
            self._want[index, deferred] = want
        return self._want[index, deferred]

    def recover(self, reply, client=None):
        """The model's client on each plane's ciphertext (noise budget, bytes), chunks joined."""
        out, budgets = b"", []
        for j in range(self.planes):
            budgets.append((client or self.client).noise_budget(reply[j]))
            rc, data = oracle.string_decode((client or self.client).decrypt(reply[j]), self.bits, self.chunk(j).shape[1], 0)
            assert rc == 0
            out += data
        return out, budgets

    def server(self, deferred, keys=True, **options):
        db = pir_amd.PIRDatabase.Create(self.pp, ct_multiplication=True, ct_deferred=deferred)
        for name, value in options.items():
            db.set_option(name, value)                   # (early options: before the first use)
        db.populate(self.raw)
        srv = pir_amd.PIRServer(db, self.pp)
        if keys:
            srv.set_galois_keys(self.keys)
            srv.set_relin_key(self.rk)
        return db, srv


_cache = {}


def setup(name):
    if name not in _cache:
        _cache[name] = {
            # 3 planes of 5 120 / 5 120 / 1 760 bytes, dims [3, 3], 9 scan rows; per plane the shape of the reference's first
            # tuple (tests/test_ctmult_model.py).  Checked on the CPU: at data seed 5, client seed 77, index 7 the model's
            # replies keep 2.35 - 3.39 bits of noise budget per plane in both forms
            "base": lambda: WideCt(9, 12000, 2, bpc=10),
            "seven": lambda: WideCt(7, 12000, 2, bpc=10),
            # dims [3, 2, 2], 2 planes: level 1 has 6 rows sharing 2 selectors
            "d3": lambda: WideCt(12, 15000, 3, plain_bits=20),
            # N = 8192, k = 4, dims [4, 3], 2 planes of 41 984 and 18 016 bytes
            "n8192": lambda: WideCt(12, 60000, 2, N=8192, plain_bits=42, moduli=T.CHAIN_8192),
        }[name]()
    return _cache[name]


def first_mismatch(got, want):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    return None if bad.size == 0 else bad[0].tolist()


def lifts(db):
    return db.get_option("ct_lifts")


# ------------------------------------------------------------------------------------------------ 1. base, both forms

@FORMS
def test_base_case_matches_the_model_plane_by_plane(deferred):
    s = setup("base")
    assert (s.planes, s.B, list(s.pp.dimensions)) == (3, 5120, [3, 3]) and s.item_bytes - 2 * s.B == 1760
    index = 7
    want = s.expected(index, deferred)
    q = s.query(index)
    db, srv = s.server(deferred)
    try:
        assert db.planes() == 3 and db.reply_ct_count() == 3 and db.get_option("ct_shared_sel") == 1
        assert srv.scan_info()["rows"] == 9
        got = srv.process_query(q)
        assert got.shape == (3, 2, 2, 4096)
        for j in range(3):
            assert first_mismatch(got[j], want[j]) is None, "plane %d: first mismatch at %s" % (j, first_mismatch(got[j], want[j]))
        item, budgets = s.recover(want)
        print("noise budget of the model's reply per plane: %s" % budgets)
        assert min(budgets) > 0
        assert item == s.recover(got)[0] == s.raw[index].tobytes()
        assert lifts(db) == 2 * 9 + 2 * 3
    finally:
        db.close()
    db, srv = s.server(deferred, ct_shared_sel=0)
    try:
        assert db.get_option("ct_shared_sel") == 0
        assert np.array_equal(srv.process_query(q), want)
        assert lifts(db) == 4 * 9
    finally:
        db.close()


# ------------------------------------------------------------------------------------------------ 2. the wire

def test_the_item_through_the_wire():
    s = setup("base")
    db = pir_amd.PIRDatabase.Create(s.pp, s.raw, ct_multiplication=True, ct_deferred=True)
    try:
        server = pir_amd.PIRServer.Create(db, s.pp)
        client = pir_amd.PIRClient.Create(s.pp, seed=b"wide-ct")
        assert client.reply_ct_count == 3
        indexes = [7, 0]
        response = server.ProcessRequest(client.CreateRequest(indexes))        # Request.relin_keys rides along
        assert client.LoadResponse(response).shape[:2] == (2, 3)
        assert client.ProcessResponse(indexes, response) == [s.raw[i].tobytes() for i in indexes]
        # residue level (pirclient_process_reply): [planes, N] coefficients from the three ciphertexts
        srv = pir_amd.PIRServer(db, s.pp)
        srv.set_galois_keys(client.galois_keys())
        srv.set_relin_key(client.relin_key())
        pts = client.process_reply(srv.process_query(client.create_query_for(7)))
        assert pts.shape == (3, 4096)
        for j in range(3):
            c = s.chunk(j)[7].tobytes()
            assert client.string_decode(pts[j], len(c), 0) == c
    finally:
        db.close()


# ------------------------------------------------------------------------------------------------ 3. a batch

@FORMS
def test_batch_of_nine_under_two_clients_keys(deferred):
    s = setup("base")
    other = Client(s.orc, seed=7)
    clients = [(s.client, s.keys, s.rk), (other, other.galois_keys(), M.relin_key(other))]
    idx = [(5 * i + 3) % 9 for i in range(9)]
    qs = np.stack([s.query(x, clients[i % 2][0]) for i, x in enumerate(idx)])
    db, srv = s.server(deferred, keys=False)
    try:
        singles = []
        for i in range(9):
            srv.set_galois_keys(clients[i % 2][1])
            srv.set_relin_key(clients[i % 2][2])
            singles.append(srv.process_query(qs[i]))
        db.set_option("ct_lifts", 0)
        out = T.run_nine(srv, clients, qs)                  # a group of 8 and a group of 1
        assert out.shape == (9, 3, 2, 2, 4096)
        assert lifts(db) == (2 * 72 + 2 * 3 * 8) + 24
        for i in range(9):
            assert first_mismatch(out[i], singles[i]) is None, "query %d of the batch" % i
        # (the single queries are the model's: query 0 asks client 0 for item 3)
        assert np.array_equal(singles[0], s.expected(idx[0], deferred))
        assert s.recover(out[8], clients[0][0])[0] == s.raw[idx[8]].tobytes()
        assert s.recover(out[7], clients[1][0])[0] == s.raw[idx[7]].tobytes()
    finally:
        db.close()


# ------------------------------------------------------------------------------------------------ 4. blocks

@FORMS
def test_blocks_that_straddle_planes_give_the_same_bits(deferred):
    """ct_scratch_mb = 1 floors the scratch at 8 pairs.  One query: the 9 children of level 0 -- 3 planes x 3 -- go in the
    blocks {0 .. 7} and {8}: the first ends inside the last plane's row, whose accumulator (deferred form: at Q and B, in the
    NTT domain) is carried.  A group of three queries: 2 children per block, {0, 1} {2, 3} {4, 5} {6, 7} {8}, rows cut
    mid-plane.  With the default scratch the deferred form shares a row's children out over workgroups and folds the
    partial sums; ct_rowsum_splits = 1 keeps one workgroup per row: both must run in the new row-sum kernel."""
    s = setup("base")
    want = s.expected(7, deferred)
    q = s.query(7)
    qs = np.stack([s.query(i) for i in (7, 0, 4)])
    group = None
    for options, blocks in [({}, (1, 1)), ({"ct_rowsum_splits": 1}, (1, 1)), ({"ct_scratch_mb": 1}, (2, 5)),
                            ({"ct_scratch_mb": 1, "ct_rowsum_splits": 1}, (2, 5))]:
        db, srv = s.server(deferred, **options)
        try:
            db.set_option("ct_blocks", 0)
            got = srv.process_query(q)
            assert db.get_option("ct_blocks") == blocks[0], options
            assert first_mismatch(got, want) is None, "%s: first mismatch at %s" % (options, first_mismatch(got, want))
            db.set_option("ct_blocks", 0)
            srv.set_concurrency(8)
            srv.stage_batch(qs)
            srv.run_batch()
            out = srv.fetch_batch()
            assert db.get_option("ct_blocks") == blocks[1], options
            assert np.array_equal(out[0], want), options
            if group is None:
                group = out
            assert np.array_equal(out, group), options
        finally:
            db.close()


# ------------------------------------------------------------------------------------------------ 5. d = 3

@FORMS
def test_three_dimensions_rows_share_the_selectors(deferred):
    """Bits only: two nested products leave this chain no budget."""
    s = setup("d3")
    assert s.planes == 2 and list(s.pp.dimensions) == [3, 2, 2]
    index = 7
    want = s.expected(index, deferred)
    replies = []
    for shared in (1, 0):
        db, srv = s.server(deferred, ct_shared_sel=shared)
        try:
            got = srv.process_query(s.query(index))
            # level 1: 2 planes x 3 rows of 2 children, level 0: 2 planes x 3 children
            assert lifts(db) == (2 * (12 + 6) + 2 * (2 + 3) if shared else 4 * (12 + 6))
            assert got.shape == (2, 2, 2, 4096)
            assert first_mismatch(got, want) is None, "shared %d: first mismatch at %s" % (shared, first_mismatch(got, want))
            replies.append(got)
        finally:
            db.close()
    assert np.array_equal(replies[0], replies[1])


def test_three_dimensions_on_a_context_without_wide_items():
    """27 plaintexts in [3, 3, 3] (tests/test_gpu_ctmult.py): the path is opt-in there, and changes no bit."""
    s, index, q, want = T.single_case(27, 3)
    for shared in (1, 0):
        db, srv = T.ct_server(s)
        try:
            if shared:                                   # (ct_server has populated the context: the option is still early)
                db.set_option("ct_shared_sel", 1)
            assert db.get_option("ct_shared_sel") == shared
            got = srv.process_query(q)
            assert lifts(db) == (2 * 12 + 2 * 6 if shared else 4 * 12)
            assert first_mismatch(got, want) is None, "shared %d: first mismatch at %s" % (shared, first_mismatch(got, want))
        finally:
            db.close()


# ------------------------------------------------------------------------------------------------ 6. N = 8192, k = 4

@pytest.mark.parametrize("mode", [None, 0], ids=["default", "integer"])
def test_second_ring_against_contexts_of_the_planes(monkeypatch, mode):
    """The wide context against two contexts without wide items that hold the planes' chunks (the existing path, pinned
    to the model in tests/test_gpu_ctmult.py and tests/test_gpu_ctmult_ladder.py): no model run at this size."""
    if mode is not None:
        monkeypatch.setenv("PIRGPU_ALLOW_ENV", "1")
        monkeypatch.setenv("PIRGPU_NTT_MODE", str(mode))
    s = setup("n8192")
    assert s.planes == 2 and list(s.pp.dimensions) == [4, 3] and s.k == 4
    plane_pp = P.create_pir_parameters(s.n, 0, 2, s.enc, True)
    assert plane_pp.bytes_per_item == s.B and list(plane_pp.dimensions) == [4, 3]
    q = s.query(10)
    for deferred in (False, True):
        db, srv = s.server(deferred)
        try:
            if mode is not None:
                assert db.lib.pirgpu_ntt_mode(db.handle) == mode
            got = srv.process_query(q)
            assert got.shape == (2, 2, 4, 8192)
            for j in range(2):
                chunk = np.zeros((s.n, s.B), dtype=np.uint8)       # (the string encoder left-aligns: zero bytes add zero bits)
                chunk[:, :s.chunk(j).shape[1]] = s.chunk(j)
                pdb = pir_amd.PIRDatabase.Create(plane_pp, ct_multiplication=True, ct_deferred=deferred)
                try:
                    pdb.populate(chunk)
                    assert np.array_equal(pdb.read_plaintext(5), s.db[j][5])
                    psrv = pir_amd.PIRServer(pdb, plane_pp)
                    psrv.set_galois_keys(s.keys)
                    psrv.set_relin_key(s.rk)
                    assert pdb.get_option("ct_shared_sel") == 0
                    ref = psrv.process_query(q)
                    assert ref.shape == (1, 2, 4, 8192)
                    assert first_mismatch(got[j], ref[0]) is None, (deferred, j, first_mismatch(got[j], ref[0]))
                finally:
                    pdb.close()
        finally:
            db.close()


# ------------------------------------------------------------------------------------------------ 7. a short database

@FORMS
def test_database_that_ends_inside_its_box(deferred):
    """7 items in [3, 3]: every plane is padded with two zero plaintexts, the model's planes have 7 -- its last row has one
    column and two children fewer.  A zero row sum gives a zero tensor, floor(h / Q) = 0 and a zero key switch."""
    s = setup("seven")
    assert list(s.pp.dimensions) == [3, 3] and s.planes == 3
    db, srv = s.server(deferred)
    try:
        for index in (6, 2):
            want = s.expected(index, deferred)
            got = srv.process_query(s.query(index))
            assert first_mismatch(got, want) is None, "item %d: first mismatch at %s" % (index, first_mismatch(got, want))
            assert s.recover(got)[0] == s.raw[index].tobytes()
    finally:
        db.close()


# ------------------------------------------------------------------------------------------------ 8. updates

def test_update_items_equals_a_fresh_context():
    s = WideCt(9, 12000, 2, bpc=10)                      # its own copy: the raw database is modified
    base = setup("base")
    s.client, s.keys, s.rk = base.client, base.keys, base.rk
    db, srv = s.server(True)
    try:
        q = s.query(4)
        before = srv.process_query(q)
        item = np.random.default_rng(8).integers(0, 256, size=(1, s.item_bytes), dtype=np.uint8)
        db.update_items([4], item)
        s.raw[4] = item[0]
        after = srv.process_query(q)
        assert not np.array_equal(after, before)
        assert s.recover(after)[0] == item[0].tobytes()
        other = srv.process_query(s.query(8))
        db2, srv2 = s.server(True)
        try:
            assert np.array_equal(srv2.process_query(q), after)
            assert np.array_equal(srv2.process_query(s.query(8)), other)
        finally:
            db2.close()
    finally:
        db.close()


# ------------------------------------------------------------------------------------------------ 9. refusals that stay

def test_refusals_that_stay():
    s = setup("base")
    both = dict(ct_multiplication=True, ct_deferred=True)
    for kw, word in [(dict(shard=(0, 2)), "row shard"), (dict(slots=(0, 4096)), "slot shard"), (dict(streamed=True), "STREAMED")]:
        code, msg = T.create_error(s.pp, **both, **kw)
        assert code == capi.INVALID_ARGUMENT and word in msg, (kw, msg)
    for field, value in [("result_primes", 1), ("tables", 2)]:
        bad = P.create_pir_parameters(9, 12000, 2, s.enc, True, 10, max_plaintexts_per_item=8)
        setattr(bad, field, value)
        code, msg = T.create_error(bad, **both)
        assert code == capi.INVALID_ARGUMENT and field in msg, (field, msg)
    big = P.EncryptionParams(32768, oracle.coeff_modulus_create(32768, [49, 49, 50]), oracle.plain_modulus_batching(32768, 20))
    wide32k = P.create_pir_parameters(12, 150000, 2, big, True, max_plaintexts_per_item=8)
    assert wide32k.planes == 2
    code, msg = T.create_error(wide32k, **both)
    assert code == capi.INVALID_ARGUMENT and "32768" in msg
    db, srv = s.server(True)
    try:
        srv.process_query(s.query(1))
        with pytest.raises(PirGpuError) as e:                # an early option: the workspace exists
            db.set_option("ct_shared_sel", 0)
        assert e.value.code == capi.FAILED_PRECONDITION and "CT_SHARED_SEL" in e.value.message
        assert db.get_option("ct_shared_sel") == 1
        assert db.lib.pirgpu_reply_copy_to_device(db.handle, None, 1) == capi.FAILED_PRECONDITION
        assert db.lib.pirgpu_reduce_fixup_device(db.handle, None, 1) == capi.FAILED_PRECONDITION
        assert db.lib.pirgpu_batch_reply_copy_to_device(db.handle, None, 1) == capi.FAILED_PRECONDITION
        assert np.array_equal(srv.process_query(s.query(7)), s.expected(7, True))      # ... and the context still serves
    finally:
        db.close()


# ------------------------------------------------------------------------------------------------ 10. the untouched default

def test_default_of_a_context_without_wide_items_is_untouched():
    """9 plaintexts in [3, 3], no wide items: the option reads 0, every pair lifts its four polynomials, the reply is the
    model's."""
    s, index, q, want = T.single_case(9, 2)
    db, srv = T.ct_server(s)
    try:
        assert db.get_option("ct_shared_sel") == 0
        db.set_option("ct_lifts", 5)
        assert lifts(db) == 5
        db.set_option("ct_lifts", 0)
        got = srv.process_query(q)
        assert db.get_option("ct_shared_sel") == 0 and lifts(db) == 4 * 3
        assert np.array_equal(got, want)
    finally:
        db.close()
