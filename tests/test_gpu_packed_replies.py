"""Packed replies on the GPU (PIRGPU_CREATE_PACKED_REPLIES), bit for bit against the model of
tests/reply_pack_model.py applied to the oracle's reply (modswitch_model.process_query_switched where result_primes is
set):

  * pirgpu_reply_pack (the launcher of the query path) and pirgpu_reply_unpack on every chain shape, every r, one and
    three ciphertexts, random and boundary residues;
  * whole replies at N = 4096, 24-bit t: d = 1, 2, 3, the 64-bit scan, a batch of 9 under two key sets, the host reply
    ring, wide items, tables, result_primes, a streamed database -- and the same queries on a context without the flag,
    which must give exactly unpack(packed reply);
  * the wire round trip with the product client; the refusals.

Every test but the unpacked control fails without the feature: flag 16 is InvalidArgument there and the exports do not
exist."""
import ctypes as C

import numpy as np
import pytest

import modswitch_model as M
import oracle
import pir_amd
import reply_pack_model as rpm
from gpu_helpers import to_product_params
from oracle.client import Client
from pir_amd import capi
from pir_amd import parameters as P
from pir_amd.server import PirGpuError
from pir_fixtures import PirSetup, generate_test_db

pytestmark = pytest.mark.gpu

N = 4096

# data primes + special prime
HOOK_CHAINS = {
    "2048/54": (2048, [54, 55]),
    "4096/36,36": (4096, [36, 36, 37]),
    "4096/30,36,40": (4096, [30, 36, 40, 40]),
    "4096/60,60": (4096, [60, 60, 60]),
    "4096/61": (4096, [61, 61]),
    "8192/43,43,44": (8192, [43, 43, 44, 44]),
    "32768/49,49,50": (32768, [49, 49, 50, 50]),
}


def hook_chain(name):
    n, bits = HOOK_CHAINS[name]
    if 61 in bits:      # one bit above what SEAL's CoeffModulus::Create hands out: the largest primes == 1 mod 2N below 2^61
        found, v = [], (1 << 61) - (((1 << 61) - 1) % (2 * n))
        while len(found) < len(bits):
            if oracle.is_prime(v):
                found.append(v)
            v -= 2 * n
        return n, found
    return n, [int(x) for x in oracle.coeff_modulus_create(n, bits)]


def patterns(q, n_ring, n, rng):
    """[(name, cts [n, 2, r, N])] for the moduli q[0..r-1]."""
    r = len(q)
    pos = np.arange(n_ring)
    out = []
    for name in ("random", "all q-1", "alternating 0 / q-1", "a single 1 in the last coefficient"):
        cts = np.zeros((n, 2, r, n_ring), dtype=np.uint64)
        for j, qj in enumerate(q):
            if name == "random":
                cts[:, :, j] = rng.integers(0, qj, size=(n, 2, n_ring), dtype=np.uint64)
            elif name == "all q-1":
                cts[:, :, j] = qj - 1
            elif name.startswith("alternating"):
                cts[:, :, j] = np.where(pos & 1, qj - 1, 0).astype(np.uint64)
            else:
                cts[:, :, j, n_ring - 1] = 1
        out.append((name, cts))
    return out


# ------------------------------------------------------------------------------------------------ the kernel alone

@pytest.mark.parametrize("name", list(HOOK_CHAINS))
def test_pack_hook_matches_the_model(name):
    n_ring, moduli = hook_chain(name)
    q = moduli[:-1]
    assert [rpm.width(v) for v in q] == HOOK_CHAINS[name][1][:-1]
    enc = P.EncryptionParams(n_ring, moduli, oracle.plain_modulus_batching(n_ring, 20))
    db = pir_amd.PIRDatabase.Create(P.create_pir_parameters(4, 0, 1, enc))        # (any context: this one does not pack)
    assert db.reply_packing() is False and db.reply_unpacked_words() == db.reply_ct_words() == 2 * len(q) * n_ring
    rng = np.random.default_rng(n_ring + len(q))
    for r in range(1, len(q) + 1):
        for n in (1, 3):
            for what, cts in patterns(q[:r], n_ring, n, rng):
                got = db.reply_pack(cts, r)
                want = rpm.pack(cts, q)
                assert got.shape == want.shape == (n, rpm.ct_words(n_ring, q, r))
                bad = np.argwhere(got != want)
                assert bad.size == 0, "%s, r = %d, n = %d: first mismatch at [ct, word] = %s" % (what, r, n, bad[:1].tolist())
                assert np.array_equal(db.reply_unpack(got, r), cts), (what, r, n)
    # arguments
    cts = patterns(q[:1], n_ring, 1, rng)[0][1]
    for bad_r in (0, len(q) + 1):
        with pytest.raises(PirGpuError) as e:
            db.reply_pack(cts, bad_r)
        assert e.value.code == capi.INVALID_ARGUMENT
    out = np.empty((1, rpm.ct_words(n_ring, q, 1)), dtype=np.uint64)
    over = cts.copy()
    over[0, 1, 0, 7] = q[0]                       # not a residue: the hook refuses it, the host unpack finds it
    rc = db.lib.pirgpu_reply_pack(db.handle, over.ctypes.data_as(capi.u64p), 1, 1, out.ctypes.data_as(capi.u64p))
    assert rc == capi.INVALID_ARGUMENT
    if q[0] & (q[0] - 1):                          # (q_0 itself fits the width unless q_0 - 1 is all ones)
        packed = rpm.pack(cts, q)
        w = rpm.width(q[0])
        packed[0, 0] |= np.uint64((1 << w) - 1)
        with pytest.raises(PirGpuError) as e:
            db.reply_unpack(packed, 1)
        assert e.value.code == capi.INVALID_ARGUMENT
    db.close()


# ------------------------------------------------------------------------------------------------ whole replies

class World:
    """One database at N = 4096, 24-bit t, 288-byte items, its oracle, and the oracle's replies computed once."""

    def __init__(self, items, d, moduli=None, n_ring=N, plain_bits=24, elem=288):
        self.s = PirSetup(items, elem, d, N=n_ring, plain_bits=plain_bits, moduli=moduli)
        self.items, self.d = items, d
        self.q = [int(x) for x in self.s.orc.moduli[:self.s.orc.k]]
        self._want = {}

    def query(self, index, client=None):
        return (client or self.s.client).create_query_for(self.s.params, index)

    def want(self, query, r=0, keys=None):
        """The reply before packing: the oracle's, or the model's switched one."""
        key = (query.tobytes(), r)
        if key not in self._want:
            s = self.s
            if r:
                rep = M.process_query_switched(s.orc, s.db_ntt, s.params.dimensions, query, keys or s.galois_keys, r)
            else:
                rc, rep = s.orc.process_query(s.db_ntt, s.params.dimensions, query, keys or s.galois_keys)
                assert rc == 0
            self._want[key] = rep
        return self._want[key]

    def want_packed(self, query, r=0, keys=None):
        return rpm.pack(self.want(query, r, keys), self.q)

    def server(self, r=0, packed=True, **kw):
        pp = to_product_params(self.s.params)
        pp.result_primes = r
        db = pir_amd.PIRDatabase.Create(pp, self.s.raw, packed_replies=packed, **kw)
        srv = pir_amd.PIRServer.Create(db, pp)
        srv.set_galois_keys(self.s.galois_keys)
        return db, srv

    def check_shape(self, db, r=0):
        k = r or len(self.q)
        n_ring = self.s.orc.N
        assert db.reply_packing() is True
        assert db.reply_unpacked_words() == 2 * k * n_ring
        assert db.reply_ct_words() == rpm.ct_words(n_ring, self.q, k) == 2 * sum(n_ring * rpm.width(v) // 64 for v in self.q[:k])


_worlds = {}


def world(name):
    if name not in _worlds:
        _worlds[name] = {
            "d1": lambda: World(120, 1),
            "d2": lambda: World(3000, 2),                  # 75 plaintexts, 9 x 9: the int8-MFMA scan
            "d2-small": lambda: World(300, 2),             # 8 plaintexts, 3 x 3: fewer than 8 rows, the 64-bit scan
            "d3": lambda: World(200, 3),
            "60": lambda: World(300, 2, moduli=oracle.coeff_modulus_create(N, [60, 60, 60])),
            "8192": lambda: World(27, 3, moduli=oracle.coeff_modulus_create(8192, [43, 43, 44, 44]), n_ring=8192,
                                  plain_bits=20, elem=0),
        }[name]()
    return _worlds[name]


@pytest.mark.parametrize("name,mfma", [("d1", 0), ("d2", 1), ("d2-small", 0), ("d3", 0)])
def test_single_queries_at_every_depth(name, mfma):
    w = world(name)
    db, srv = w.server()
    w.check_shape(db)
    assert int(srv.scan_info()["mfma"]) == mfma
    for index in (1, w.items - 2):
        q = w.query(index)
        got = srv.process_query(q)
        want = w.want_packed(q)
        assert got.shape == want.shape == (db.reply_ct_count(), db.reply_ct_words())
        assert np.array_equal(got, want), index
        residues = srv.unpack_replies(got)
        assert np.array_equal(residues, w.want(q))
        assert w.s.client.process_response(w.s.params, index, residues) == w.s.item(index)
    # the staged path and its fetch
    srv.stage_query(q)
    srv.run_staged()
    assert np.array_equal(srv.fetch_reply(), want)
    # the batch pipeline: the lanes with the int8 scan, the workers without it
    idx = [(7 * i + 3) % w.items for i in range(3)]
    qs = np.stack([w.query(i) for i in idx])
    out = srv.process_batch(qs, n_workers=4)
    assert out.shape == (3, db.reply_ct_count(), db.reply_ct_words())
    for i in range(3):
        assert np.array_equal(out[i], w.want_packed(qs[i])), i
    db.close()


def test_batch_of_nine_under_two_key_sets_and_the_host_reply_ring():
    """One full group and one partial one, the queries alternating between two clients' key sets; then the same batch with
    pirgpu_batch_set_host_replies: group-wise downloads of packed words into the pinned ring."""
    w = world("d2")
    s = w.s
    db, srv = w.server()
    other = Client(s.orc, seed=7)
    clients = [(s.client, s.galois_keys), (other, other.galois_keys())]
    slots = [srv.install_keyset(b"packed-client-%d" % i, keys) for i, (_, keys) in enumerate(clients)]
    idx = [(331 * i + 5) % w.items for i in range(9)]
    qs = np.stack([w.query(x, clients[i % 2][0]) for i, x in enumerate(idx)])
    want = np.stack([w.want_packed(qs[i], 0, clients[i % 2][1]) for i in range(9)])
    srv.set_concurrency(8)
    srv.stage_batch(qs)
    srv.set_batch_keysets([slots[i % 2] for i in range(9)])
    srv.run_batch()
    out = srv.fetch_batch()
    assert out.shape == want.shape == (9, 8, db.reply_ct_words())
    for i in range(9):
        assert np.array_equal(out[i], want[i]), "query %d of the batch" % i
    # the host reply ring
    lib, h = srv.lib, db.handle
    n, words = db.reply_ct_count(), db.reply_ct_words()
    host = lib.pirgpu_host_reply_buffer(h, 9)
    assert host
    view = np.ctypeslib.as_array(C.cast(host, C.POINTER(C.c_uint64)), shape=(9, n, words))
    view[:] = 0
    assert lib.pirgpu_batch_set_host_replies(h, C.c_void_p(host), 9 * n) == 0      # the capacity stays in ciphertexts
    srv.stage_batch(qs)
    srv.set_batch_keysets([slots[i % 2] for i in range(9)])
    srv.run_batch()
    seen, ready = [], C.c_uint32(0)
    while not seen or seen[-1] < 9:
        assert lib.pirgpu_batch_next_host_replies(h, C.byref(ready)) == 0
        assert ready.value > (seen[-1] if seen else 0)
        assert np.array_equal(view[:ready.value], want[:ready.value])
        seen.append(ready.value)
    assert seen == [8, 9]
    cnt = C.c_uint64(0)
    assert lib.pirgpu_batch_fetch(h, C.cast(host, C.POINTER(C.c_uint64)), 9 * n, C.byref(cnt)) == 0 and cnt.value == 9 * n
    assert np.array_equal(view, want)
    assert lib.pirgpu_batch_set_host_replies(h, None, 0) == 0
    db.close()


def test_the_same_queries_without_the_flag_give_the_unpacked_reply():
    """The control (passes without the feature's kernel): the reply before packing is what the context produces today, so
    a context without the flag returns exactly unpack(packed reply) -- single query and batch."""
    w = world("d2")
    db, srv = w.server(packed=False)
    assert db.reply_packing() is False and db.reply_ct_words() == db.reply_unpacked_words() == 2 * 2 * N
    pdb, psrv = w.server()
    idx = [(331 * i + 5) % w.items for i in range(9)]
    qs = np.stack([w.query(x) for x in idx])
    plain = srv.process_batch(qs, n_workers=8)
    packed = psrv.process_batch(qs, n_workers=8)
    assert plain.shape == (9, 8, 2, 2, N) and packed.shape == (9, 8, pdb.reply_ct_words())
    assert np.array_equal(psrv.unpack_replies(packed), plain)
    assert np.array_equal(rpm.unpack(packed, w.q, 2, N), plain)
    assert np.array_equal(psrv.unpack_replies(psrv.process_query(qs[0])), srv.process_query(qs[0]))
    db.close()
    pdb.close()


def test_wide_items_pack_every_plane():
    """7 items of 3 planes in 3 x 3: plane j's ciphertexts are the packed reply of plane j's own database, plane-major."""
    from test_gpu_wide_items import WideSetup
    ws = WideSetup(7, 2 * 11776 + 1000, 2, N=N, plain_bits=24)
    assert ws.planes == 3 and list(ws.pp.dimensions) == [3, 3]
    db, srv = ws.server(packed_replies=True)
    q = [int(x) for x in ws.orc.moduli[:2]]
    assert db.reply_ct_count() == 3 * ws.R and db.reply_ct_words() == rpm.ct_words(N, q)
    for index in (0, 6):
        query = ws.query(index)
        got = srv.process_query(query)
        want = ws.expected(query)
        assert np.array_equal(got, rpm.pack(want, q)), index
        assert ws.recover(srv.unpack_replies(got)) == ws.raw[index].tobytes()
    db.close()


def test_tables_mixed_in_one_group():
    from test_gpu_tables import World as Tables
    t = Tables(2, 3000, N=N, plain_bits=24)
    q = [int(x) for x in t.orc.moduli[:2]]
    db, srv = t.server(packed_replies=True)
    assert db.tables() == 2 and db.reply_packing()
    tabs = [1, 0, 0, 1, 1]
    idx = [2999 - 131 * i for i in range(5)]
    qs = np.stack([t.query(i) for i in idx])
    srv.set_concurrency(8)
    out = srv.process_batch(qs, tables=tabs)
    for i in range(5):
        assert np.array_equal(out[i], rpm.pack(t.want(tabs[i], idx[i]), q)), i
    srv.use_table(1)
    assert np.array_equal(srv.process_query(qs[0]), rpm.pack(t.want(1, idx[0]), q))
    db.close()


@pytest.mark.parametrize("name,r", [("60", 1), ("8192", 1), ("8192", 2)])
def test_result_primes_compose_with_packing(name, r):
    """The switch runs where level 0 lies (stride k kept) and the pack kernel reads its first r residues."""
    w = world(name)
    db, srv = w.server(r=r)
    w.check_shape(db, r)
    index = w.items - 3
    q = w.query(index)
    want = w.want(q, r)
    got = srv.process_query(q)
    assert got.shape == (want.shape[0], rpm.ct_words(w.s.orc.N, w.q, r))
    assert np.array_equal(got, rpm.pack(want, w.q))
    assert np.array_equal(srv.unpack_replies(got), want)
    qs = np.stack([q, w.query(1)])
    out = srv.process_batch(qs, n_workers=8)
    assert np.array_equal(out[0], got) and np.array_equal(out[1], rpm.pack(w.want(qs[1], r), w.q))
    db.close()


def test_streamed_database_serves_packed_replies():
    w = world("d2")
    db, srv = w.server(streamed=True)
    w.check_shape(db)
    q = w.query(1733)
    assert np.array_equal(srv.process_query(q), w.want_packed(q))
    db.close()


# ------------------------------------------------------------------------------------------------ wire round trip

def test_wire_round_trip_with_the_product_client():
    """ProcessRequest on a packed context -> pirclient_process_response: the items come back, and the response is shorter
    than the unpacked context's by exactly the computed byte count."""
    enc = P.generate_encryption_params(N, 24)
    pp = P.create_pir_parameters(3000, 288, 2, enc)
    raw = generate_test_db(3000, 288, seed=8)
    client = pir_amd.PIRClient.Create(pp, seed=b"packed-rt")
    q = [int(v) for v in enc.coeff_modulus[:-1]]
    n_cts, words = client.reply_ct_count, rpm.ct_words(N, q)
    assert client.packed_reply_ct_words == words
    responses = {}
    batches = [[1733], [(331 * i + 5) % 3000 for i in range(9)]]
    requests = [client.CreateRequest(indexes) for indexes in batches]      # the same bytes go to both contexts
    for packed in (True, False):
        db = pir_amd.PIRDatabase.Create(pp, raw, packed_replies=packed)
        srv = pir_amd.PIRServer.Create(db, pp)
        for indexes, request in zip(batches, requests):
            response = srv.ProcessRequest(request)
            assert client.ProcessResponse(indexes, response) == [raw[i].tobytes() for i in indexes], packed
            responses[packed, len(indexes)] = response
        db.close()
    for n in (1, 9):
        a, b = responses[False, n], responses[True, n]
        payload = n * n_cts * (2 * 2 * N - words) * 8
        # per ciphertext and per reply one length varint, each at most one byte shorter
        assert 0 <= len(a) - len(b) - payload <= n * (n_cts + 1) + 1, (n, len(a), len(b), payload)
        assert np.array_equal(client.LoadResponse(a), client.LoadResponse(b))


# ------------------------------------------------------------------------------------------------ refused

def test_create_refuses_what_cannot_be_packed():
    w = world("d2-small")
    pp = to_product_params(w.s.params)
    for kw, word in [({"shard": (0, 2)}, "row shard"), ({"slots": (0, 4096)}, "slot shard")]:
        with pytest.raises(PirGpuError) as e:
            pir_amd.PIRDatabase.Create(pp, packed_replies=True, **kw)
        assert e.value.code == capi.INVALID_ARGUMENT and "PIRGPU_CREATE_PACKED_REPLIES" in str(e.value) and word in str(e.value)
    cm = to_product_params(w.s.params)
    cm.use_ciphertext_multiplication = True
    with pytest.raises(PirGpuError) as e:
        pir_amd.PIRDatabase.Create(cm, packed_replies=True, ct_multiplication=True)
    assert e.value.code == capi.INVALID_ARGUMENT and "PIRGPU_CREATE_PACKED_REPLIES" in str(e.value)
    lib = capi.load()
    for flags in (2, 3, 16 | 2, 32 | 16):
        h = C.c_void_p()
        assert lib.pirgpu_create_ex(C.byref(capi.make_params(pp)), flags, C.byref(h)) == capi.INVALID_ARGUMENT, flags


def test_multi_gpu_entry_points_and_device_copies_refuse_a_packed_context():
    w = world("d2-small")
    db, srv = w.server()
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
        assert b"PIRGPU_CREATE_PACKED_REPLIES" in lib.pirgpu_last_error(h), name
    db.close()
