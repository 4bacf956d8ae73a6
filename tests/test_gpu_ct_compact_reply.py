"""Compact replies of the ciphertext-multiplication mode on the GPU (PIRGPU_CREATE_CT_COMPACT_REPLY, DESIGN.md section
6.6), bit for bit against the CPU models:

    reply = reply_pack_model.pack(modswitch_model.switch_residues(R, q, r), q)        (r = 0: pack(R, q))

with R the mode's reply at k primes -- ctmult_model.process_query_ct, or ctmult_deferred_model.process_query_ct_deferred
with PIRGPU_CREATE_CT_DEFERRED.  R is computed once per shape (the caches of tests/test_gpu_ctmult.py and
tests/test_gpu_ctmult_wide.py are shared with those files) and left unchanged.

  1. single queries on the default chain: d = 2 on the 64-bit and the int8-MFMA scan, d = 3, d = 1, r = 1, and r = 0;
  2. the item recovered at level 1 on the reference's two tuples;  3. the deferred form;
  4. several drop steps and mixed widths;  5. wide items;  6. a batch of 9 under two clients' keys, fetched and through
  the host reply ring;  7. a level multiplied in two product blocks (the row's sum carried in the `last` buffer);
  8. the wire;  9. the refusals;  10. the flag off.

Every test fails without the feature: flag 64 is an unknown bit there."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import ctmult_deferred_model as D
import modswitch_model as MS
import oracle
import pir_amd
import reply_pack_model as rpm
import seal_wire
import test_gpu_ctmult as T
import test_gpu_ctmult_wide as W
from gpu_helpers import chain, to_product_params
from pir_amd import capi
from pir_amd.server import PirGpuError

pytestmark = pytest.mark.gpu

FORMS = pytest.mark.parametrize("deferred", [False, True], ids=["per-child", "deferred"])


def moduli_of(s):
    return [int(v) for v in s.orc.moduli[:s.orc.k]]


def model(want_k, q, r):
    """The mode's reply at k primes [n][2][k][N] -> (residues at the reply's level, packed words)."""
    residues = MS.switch_residues(want_k, q, r) if r else np.asarray(want_k)
    return residues, rpm.pack(residues, q)


def compact_server(s, r, deferred=False, keys=True, ct_scratch_mb=None, compact=True):
    pp = T.ct_params(s.params)
    pp.result_primes = r
    db = pir_amd.PIRDatabase.Create(pp, ct_multiplication=True, ct_deferred=deferred, ct_compact_reply=compact)
    if ct_scratch_mb is not None:
        db.set_option("ct_scratch_mb", ct_scratch_mb)       # (shapes the workspace: before the first use)
    db.populate(s.raw)
    srv = pir_amd.PIRServer(db, pp)
    if keys:
        srv.set_galois_keys(s.galois_keys)
        srv.set_relin_key(s.rk)
    return db, srv


_DEFERRED = {}


def deferred_case(dbsize):
    """The setup, index and query of T.single_case(dbsize, 2) with the deferred model's reply, computed once."""
    if dbsize not in _DEFERRED:
        s, index, q, _ = T.single_case(dbsize, 2)
        rc, want = D.process_query_ct_deferred(s.orc, s.db_ntt, s.params.dimensions, q, s.galois_keys, s.rk)
        assert rc == 0
        _DEFERRED[dbsize] = (s, index, q, want)
    return _DEFERRED[dbsize]


_UNPACKERS = {}


def client_unpack(pp, packed):
    """pirclient_unpack_reply of a product client made with the context's parameters (any secret: unpacking has none)."""
    key = (tuple(pp.encryption_parameters.coeff_modulus), pp.result_primes)
    if key not in _UNPACKERS:
        _UNPACKERS[key] = pir_amd.PIRClient.Create(pp, seed=b"unpack")
    return _UNPACKERS[key].unpack_reply(packed)


def check_getters(db, s, r, planes=1):
    N, q = s.orc.N, moduli_of(s)
    assert db.reply_ct_count() == planes
    assert db.reply_ct_words() == rpm.ct_words(N, q, r or len(q))
    assert db.reply_packing() is True
    assert db.reply_unpacked_words() == 2 * (r or len(q)) * N


def check_reply(db, srv, s, got, want_k, r):
    """The packed words, and the words unpacked by the server library and by the client, against the models."""
    residues, packed = model(want_k, moduli_of(s), r)
    assert got.shape == packed.shape == (want_k.shape[0], db.reply_ct_words())
    bad = np.argwhere(got != packed)
    assert bad.size == 0, "first mismatch at [ct, word] = %s" % bad[:1].tolist()
    assert np.array_equal(srv.unpack_replies(got), residues)
    assert np.array_equal(client_unpack(srv.params, got), residues)
    return residues


def recover(s, index, ct, r):
    """noise_budget_level and the item's bytes of one reply ciphertext at level r, with the model's client."""
    p = s.params
    rc, data = oracle.string_decode(MS.decrypt_level(s.client, ct, r), p.eff_bits_per_coeff, p.bytes_per_item,
                                    oracle.calculate_item_offset(index, p.items_per_plaintext, p.bytes_per_item))
    assert rc == 0
    return MS.noise_budget_level(s.client, ct, r), data


# ------------------------------------------------------------------------------------------------ 1. single queries

@pytest.mark.parametrize("dbsize,d,mfma,r", [(9, 2, 0, 1), (100, 2, 1, 1), (27, 3, 1, 1), (10, 1, 0, 1), (9, 2, 0, 0)])
def test_single_queries_match_the_model(dbsize, d, mfma, r):
    s, index, q, want = T.single_case(dbsize, d)
    db, srv = compact_server(s, r, keys=d > 1)
    if d == 1:
        srv.set_galois_keys(s.galois_keys)      # d = 1 needs no relinearisation key: the row sum is what gets switched
    check_getters(db, s, r)
    assert srv.scan_info()["mfma"] == mfma
    db.set_option("ct_blocks", 0)
    got = srv.process_query(q)
    assert db.get_option("ct_blocks") == d - 1
    check_reply(db, srv, s, got, want, r)
    # the staged path and its fetch
    srv.stage_query(q)
    srv.run_staged()
    assert np.array_equal(srv.fetch_reply(), got)
    db.close()


# ------------------------------------------------------------------------------------------------ 2. item recovery

_MIDROW = []


def midrow_case():
    """500 plaintexts in 23 x 22, 6 bits per coefficient, index 125 (correctness_test.cpp:100), computed once."""
    if not _MIDROW:
        s = T.setup(500, 2, bpc=6)
        q = s.client.create_query_for(s.params, 125)
        _MIDROW.append((s, 125, q, T.expected(s, q)))
    return _MIDROW[0]


@pytest.mark.parametrize("case", ["9 items", "500 items"])
def test_item_is_recovered_at_level_one(case):
    """The reference's two d = 2 tuples at N = 4096: tools/ct_compact_noise_table.py finds 1.87 and 1.56 bits of budget
    at level 1 for these seeds, the same as at k primes."""
    s, index, q, want = T.single_case(9, 2) if case == "9 items" else midrow_case()
    db, srv = compact_server(s, 1)
    residues = check_reply(db, srv, s, srv.process_query(q), want, 1)
    budget, data = recover(s, index, residues[0], 1)
    print("%s: noise budget at level 1 %.2f bits" % (case, budget))
    assert budget > 0 and data == s.item(index)
    db.close()


# ------------------------------------------------------------------------------------------------ 3. deferred form

@pytest.mark.parametrize("dbsize,mfma", [(9, 0), (100, 1)])
def test_deferred_form_matches_the_deferred_model(dbsize, mfma):
    s, index, q, want = deferred_case(dbsize)
    db, srv = compact_server(s, 1, deferred=True)
    check_getters(db, s, 1)
    assert srv.scan_info()["mfma"] == mfma
    check_reply(db, srv, s, srv.process_query(q), want, 1)
    db.close()


# ------------------------------------------------------------------------------------------------ 4. drop steps, widths

_CHAINS = {}


def chain_case(name):
    if name not in _CHAINS:
        if name == "k3-mixed":      # N = 4096, [30, 36, 40 | 40]: three word offsets per polynomial pair
            s = T.setup(9, 2, N=4096, plain_bits=20, moduli=chain(4096, [30, 36, 40]))
        else:                       # N = 8192, [43, 43, 44, 44 | 44], 10 bits per coefficient
            s = T.setup(9, 2, N=8192, plain_bits=20, moduli=T.CHAIN_8192, bpc=10)
        q = s.client.create_query_for(s.params, 5)
        _CHAINS[name] = (s, 5, q, T.expected(s, q))
    return _CHAINS[name]


@pytest.mark.parametrize("name,r,item", [("k3-mixed", 2, False), ("k3-mixed", 1, False), ("8192", 1, True)])
def test_several_drop_steps_and_mixed_widths(name, r, item):
    """k3-mixed: bits only.  8192: three drop steps; tools/ct_compact_noise_table.py finds 15.61 bits at level 1 for these
    seeds, and the item comes back."""
    s, index, q, want = chain_case(name)
    widths = [rpm.width(v) for v in moduli_of(s)]
    assert widths == ([30, 36, 40] if name == "k3-mixed" else [43, 43, 44, 44])
    db, srv = compact_server(s, r)
    check_getters(db, s, r)
    residues = check_reply(db, srv, s, srv.process_query(q), want, r)
    if item:
        budget, data = recover(s, index, residues[0], r)
        assert budget > 0 and data == s.item(index)
    db.close()


# ------------------------------------------------------------------------------------------------ 5. wide items

@FORMS
def test_wide_items_every_plane(deferred):
    """The `base` shape of tests/test_gpu_ctmult_wide.py (9 items of 12 000 bytes, 3 planes, 10 bits per coefficient,
    data seed 5, client seed 77, index 7).  Checked on the CPU: the model's replies keep 2.37 / 2.35 / 3.39 bits of noise
    budget per plane at level 1, in both forms -- what they keep at k primes."""
    s = W.setup("base")
    index = 7
    want = s.expected(index, deferred)
    q = [int(v) for v in s.orc.moduli[:s.k]]
    pp = dataclasses.replace(s.pp, result_primes=1)
    db = pir_amd.PIRDatabase.Create(pp, ct_multiplication=True, ct_deferred=deferred, ct_compact_reply=True)
    try:
        db.populate(s.raw)
        srv = pir_amd.PIRServer(db, pp)
        srv.set_galois_keys(s.keys)
        srv.set_relin_key(s.rk)
        assert db.planes() == 3 and db.reply_ct_count() == 3 and db.reply_packing() is True
        assert db.reply_ct_words() == rpm.ct_words(4096, q, 1) and db.reply_unpacked_words() == 2 * 4096
        got = srv.process_query(s.query(index))
        assert got.shape == (3, db.reply_ct_words())
        unpacked = srv.unpack_replies(got)
        item = b""
        for j in range(3):
            residues, packed = model(want[j:j + 1], q, 1)
            assert np.array_equal(got[j], packed[0]), "plane %d" % j
            assert np.array_equal(unpacked[j], residues[0]), "plane %d" % j
            assert MS.noise_budget_level(s.client, unpacked[j], 1) > 0, "plane %d" % j
            rc, data = oracle.string_decode(MS.decrypt_level(s.client, unpacked[j], 1), s.bits, s.chunk(j).shape[1], 0)
            assert rc == 0
            item += data
        assert item == s.raw[index].tobytes()
    finally:
        db.close()


# ------------------------------------------------------------------------------------------------ 6. a batch

def test_batch_of_nine_fetched_and_through_the_host_reply_ring():
    """8 x 2 plaintexts, 9 queries (a group of 8 and a group of 1 on the lanes) alternating two clients' key sets."""
    s, clients, qs, want = T.nine_case()
    q = moduli_of(s)
    db, srv = compact_server(s, 1)
    assert srv.scan_info()["mfma"] == 1
    packed = np.stack([model(want[i], q, 1)[1] for i in range(9)])
    slots = [srv.install_keyset(b"client-%d" % i, keys, relin_key=rk) for i, (_, keys, rk) in enumerate(clients)]

    def run():
        srv.set_concurrency(8)
        srv.stage_batch(qs)
        srv.set_batch_keysets([slots[i % 2] for i in range(9)])
        srv.run_batch()

    run()
    out = srv.fetch_batch()                                  # pirgpu_batch_fetch
    assert out.shape == packed.shape == (9, 1, db.reply_ct_words())
    for i in range(9):
        assert np.array_equal(out[i], packed[i]), "query %d of the batch" % i
    # the group-wise host reply ring
    lib, h = srv.lib, db.handle
    words = db.reply_ct_words()
    host = lib.pirgpu_host_reply_buffer(h, 9)
    assert host
    view = np.ctypeslib.as_array(C.cast(host, C.POINTER(C.c_uint64)), shape=(9, 1, words))
    view[:] = 0
    assert lib.pirgpu_batch_set_host_replies(h, C.c_void_p(host), 9) == 0
    run()
    seen, ready = [], C.c_uint32(0)
    while not seen or seen[-1] < 9:
        assert lib.pirgpu_batch_next_host_replies(h, C.byref(ready)) == 0
        assert ready.value > (seen[-1] if seen else 0)
        assert np.array_equal(view[:ready.value], packed[:ready.value])
        seen.append(ready.value)
    assert seen == [8, 9]
    assert lib.pirgpu_batch_set_host_replies(h, None, 0) == 0
    # every reply is its single-query reply
    for i in range(9):
        srv.use_keyset(slots[i % 2])
        assert np.array_equal(srv.process_query(qs[i]), packed[i]), "query %d alone" % i
    db.close()


# ------------------------------------------------------------------------------------------------ 7. product blocks

@FORMS
def test_level_zero_in_two_product_blocks(deferred):
    """ct_scratch_mb = 1 on 10 x 10 plaintexts: the 10 children of level 0 are multiplied in the blocks {0 .. 7} and
    {8, 9}; the selected row is 9, so the reply is right only if the first block's sum is carried -- per child in the
    `last` buffer, where level 0 now lands, deferred in the accumulators of the scratch."""
    s, index, q, want = deferred_case(100) if deferred else T.single_case(100, 2)
    assert index // 10 == 9
    db, srv = compact_server(s, 1, deferred=deferred, ct_scratch_mb=1)
    db.set_option("ct_blocks", 0)
    got = srv.process_query(q)
    assert db.get_option("ct_blocks") == 2
    check_reply(db, srv, s, got, want, 1)
    db.close()


# ------------------------------------------------------------------------------------------------ 8. the wire

def _save(fn, pp, cts):
    lib = capi.load()
    f = getattr(lib, fn)
    f.argtypes = [C.POINTER(capi.Params), capi.u64p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    f.restype = C.c_int
    p = capi.make_params(pp)
    out, n = C.c_void_p(), C.c_size_t()
    cts = np.ascontiguousarray(cts)
    assert f(C.byref(p), cts.ctypes.data_as(capi.u64p), cts.shape[0], C.byref(out), C.byref(n)) == 0
    blob = C.string_at(out, n.value)
    lib.pirgpu_free(out)
    return blob


@pytest.mark.parametrize("seeded", [True, False], ids=["seeded", "expanded"])
def test_wire_round_trip_with_the_product_client(seeded):
    """The 9-item tuple, the product client of tests/test_ct_compact_reply_host.py (seed and index checked there on the
    CPU: positive budget at level 1): one ciphertext, parms_id of level 1, compression byte 0x80."""
    s, index, _, _ = T.single_case(9, 2)
    pp = T.ct_params(s.params)
    pp.result_primes = 1
    q = moduli_of(s)
    db = pir_amd.PIRDatabase.Create(pp, s.raw, ct_multiplication=True, ct_compact_reply=True)
    server = pir_amd.PIRServer.Create(db, pp)
    client = pir_amd.PIRClient.Create(pp, seed=b"ct-compact-host")
    client.set_seeded_keys(seeded)
    query = client.create_query_for(index)
    response = server.ProcessRequest(client.SaveRequest([query]))
    rc, want = T.M.process_query_ct(s.orc, s.db_ntt, s.params.dimensions, query, client.galois_keys(), client.relin_key())
    assert rc == 0
    residues, packed = model(want, q, 1)
    expect = _save("pirgpu_wire_save_reply_packed", pp, packed)
    assert len(response) == len(expect)
    assert 8 * packed.size < len(response) < 8 * packed.size + 160
    cts = seal_wire._parse(seal_wire._parse(response)[0][1])
    assert len(cts) == 1
    ct = bytes(cts[0][1])
    head = 16 + 32 + 1 + 4 * 8
    assert ct[16:48] == seal_wire.parms_id(4096, q[:1], s.orc.t)
    assert ct[head + 5] == 0x80
    assert int.from_bytes(ct[head + 16:head + 24], "little") == 2 * 1 * 4096
    assert response == expect
    assert np.array_equal(client.LoadResponse(response)[0], residues)
    assert client.ProcessResponse([index], response) == [s.item(index)]
    # CreateRequest's own query, keys resident
    assert client.ProcessResponse([index, 1], server.ProcessRequest(client.CreateRequest([index, 1]))) == [s.item(index), s.item(1)]
    db.close()


# ------------------------------------------------------------------------------------------------ 9. refusals

def create_error(pp, **kw):
    with pytest.raises(PirGpuError) as e:
        pir_amd.PIRDatabase.Create(pp, **kw)
    return e.value.code, e.value.message


def test_refusals_at_create():
    s, _, _, _ = T.single_case(100, 2)
    pp = T.ct_params(s.params)
    pp.result_primes = 1
    lib = capi.load()

    def create_ex(p, flags, **kw):
        h = C.c_void_p()
        rc = lib.pirgpu_create_ex(C.byref(capi.make_params(p, **kw)), flags, C.byref(h))
        msg = lib.pirgpu_create_error().decode()
        if h:
            lib.pirgpu_destroy(h)
        return rc, msg

    rc, msg = create_ex(to_product_params(s.params), 64)                    # 64 alone
    assert rc == capi.INVALID_ARGUMENT and "PIRGPU_CREATE_CT_COMPACT_REPLY" in msg and "PIRGPU_CREATE_CT_MULTIPLY" in msg
    rc, msg = create_ex(pp, 64 | 16 | 4)
    assert rc == capi.INVALID_ARGUMENT and "PIRGPU_CREATE_PACKED_REPLIES" in msg
    rc, msg = create_ex(pp, 4)                                              # result_primes without the flag
    assert rc == capi.INVALID_ARGUMENT and "result_primes" in msg
    for kw, word in [(dict(shard=(0, 5)), "row shard"), (dict(slots=(0, 4096)), "slot shard")]:
        rc, msg = create_ex(pp, 64 | 4, **kw)
        assert rc == capi.INVALID_ARGUMENT and word in msg, (kw, msg)
    rc, msg = create_ex(pp, 64 | 4 | 1)
    assert rc == capi.INVALID_ARGUMENT and "STREAMED" in msg
    tabs = T.ct_params(s.params)
    tabs.tables = 2
    code, msg = create_error(tabs, ct_multiplication=True, ct_compact_reply=True)
    assert code == capi.INVALID_ARGUMENT and "tables" in msg
    full = T.ct_params(s.params)
    full.result_primes = 2                                                  # r = k
    code, msg = create_error(full, ct_multiplication=True, ct_compact_reply=True)
    assert code == capi.INVALID_ARGUMENT and "result_primes" in msg
    for flags in (2, 3, 16 | 2, 32 | 16, 64 | 32):
        rc, msg = create_ex(pp, flags)
        assert rc == capi.INVALID_ARGUMENT and "flags" in msg, flags


def test_multi_gpu_entry_points_and_device_copies_refuse_a_live_context():
    s, index, q, want = T.single_case(9, 2)
    db, srv = compact_server(s, 1)
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
    check_reply(db, srv, s, srv.process_query(q), want, 1)                  # ... and the context still serves
    db.close()


# ------------------------------------------------------------------------------------------------ 10. the flag off

def test_flag_off_is_untouched():
    s, index, q, want = T.single_case(9, 2)
    db, srv = compact_server(s, 0, compact=False)
    assert db.reply_packing() is False and db.reply_ct_words() == db.reply_unpacked_words() == 2 * 2 * 4096
    got = srv.process_query(q)
    assert got.shape == (1, 2, 2, 4096) and np.array_equal(got, want)
    db.close()
    pp = to_product_params(s.params)
    plain = pir_amd.PIRDatabase.Create(pp, s.raw)
    psrv = pir_amd.PIRServer(plain, pp)
    psrv.set_galois_keys(s.galois_keys)
    rc, ref = s.orc.process_query(s.db_ntt, s.params.dimensions, q, s.galois_keys)
    assert rc == 0 and plain.reply_packing() is False
    assert np.array_equal(psrv.process_query(q), ref)
    plain.close()
    # (with the flag, the same query gives the packed k-prime reply: what makes this test need the feature)
    cdb, csrv = compact_server(s, 0)
    assert np.array_equal(csrv.unpack_replies(csrv.process_query(q)), want)
    cdb.close()
