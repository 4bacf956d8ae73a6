"""Packed replies (PIRGPU_CREATE_PACKED_REPLIES) -- the host-side contract, no GPU: the flag's
value and its neighbours, the exports, the refusals that are found before a device is looked for, the Python mirrors
against a recording library, and the wire form end to end on the CPU: the oracle's reply, packed by the model, saved by
the server's serialiser (device-free hook), read back by the product client."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
import pir_amd
import reply_pack_model as rpm
import seal_wire
from gpu_helpers import to_product_params
from pir_amd import capi
from pir_amd.server import PIRDatabase, PIRServer, PirGpuError
from pir_fixtures import PirSetup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096
HOOK = (C.c_int, [C.c_void_p, capi.u64p, C.c_uint64, C.c_uint32, capi.u64p])


def _params(d=2):
    return to_product_params(oracle.create_pir_parameters(300, 288, d, N=N, plain_bits=24))


def _create_ex(cp, flags):
    lib = capi.load()
    h = C.c_void_p()
    rc = lib.pirgpu_create_ex(C.byref(cp), flags, C.byref(h))
    msg = lib.pirgpu_create_error().decode()
    if h:
        lib.pirgpu_destroy(h)
    return rc, msg


def test_flag_value_exports_and_signatures():
    header = open(os.path.join(ROOT, "include", "pirgpu.h")).read()
    assert re.search(r"#define PIRGPU_CREATE_PACKED_REPLIES 16u\b", header)
    assert capi.CREATE_PACKED_REPLIES == 16
    lib = capi.load()
    for name, sig in [("pirgpu_reply_packing", (C.c_int, [C.c_void_p])),
                      ("pirgpu_reply_unpacked_words", (C.c_uint64, [C.c_void_p])),
                      ("pirgpu_reply_pack", HOOK), ("pirgpu_reply_unpack", HOOK)]:
        assert name in header and hasattr(lib, name) and capi.SIGNATURES[name] == sig, name
    assert lib.pirgpu_reply_packing(None) == 0 and lib.pirgpu_reply_unpacked_words(None) == 0
    assert lib.pirgpu_reply_pack(None, None, 0, 1, None) == capi.INVALID_ARGUMENT
    assert lib.pirgpu_reply_unpack(None, None, 0, 1, None) == capi.INVALID_ARGUMENT
    assert hasattr(lib, "pirgpu_wire_save_reply_packed")
    cheader = open(os.path.join(ROOT, "include", "pirclient.h")).read()
    clib = capi.load_client()
    assert "pirclient_unpack_reply" in cheader and hasattr(clib, "pirclient_unpack_reply")
    assert capi.CLIENT_SIGNATURES["pirclient_unpack_reply"] == (C.c_int, [C.c_void_p, capi.u64p, C.c_size_t, capi.u64p])
    assert clib.pirclient_unpack_reply(None, None, 0, None) == capi.INVALID_ARGUMENT


def test_flag_is_known_and_its_neighbours_stay_invalid():
    cp = capi.make_params(_params())
    h = C.c_void_p()
    lib = capi.load()
    plain = lib.pirgpu_create(C.byref(cp), C.byref(h))
    if h:
        lib.pirgpu_destroy(h)
    for flags in (16, 16 | capi.CREATE_STREAMED_DB):
        rc, msg = _create_ex(cp, flags)
        assert rc == plain, (flags, rc, msg)            # succeeds with a GPU; without one the same loud failure
        if rc:
            assert rc == capi.INTERNAL and "no HIP device" in msg
    for flags in (2, 3, 16 | 2, 32, 16 | 32, 0x80000000 | 16):
        rc, msg = _create_ex(cp, flags)
        assert rc == capi.INVALID_ARGUMENT and "flags" in msg, (flags, rc, msg)


def test_refusals_at_create_name_the_flag():
    pp = _params()
    cp = capi.make_params(pp, shard=(0, 5))
    rc, msg = _create_ex(cp, 16)
    assert rc == capi.INVALID_ARGUMENT and "PIRGPU_CREATE_PACKED_REPLIES" in msg and "row shard" in msg, (rc, msg)
    cp = capi.make_params(pp, slots=(0, 1024))
    rc, msg = _create_ex(cp, 16)
    assert rc == capi.INVALID_ARGUMENT and "PIRGPU_CREATE_PACKED_REPLIES" in msg and "slot shard" in msg, (rc, msg)
    cp = capi.make_params(pp)
    cp.use_ciphertext_multiplication = 1
    rc, msg = _create_ex(cp, 16 | capi.CREATE_CT_MULTIPLY)
    assert rc == capi.INVALID_ARGUMENT and "PIRGPU_CREATE_PACKED_REPLIES" in msg and "CT_MULTIPLY" in msg, (rc, msg)


class _RecordingLib:
    """Stands in for libpirgpu: records every call, succeeds."""

    def __init__(self, packing=0, words=0):
        self.calls, self.packing, self.words = [], packing, words

    def pirgpu_reply_packing(self, h):
        return self.packing

    def pirgpu_reply_ct_words(self, h):
        return self.words

    def pirgpu_reply_ct_count(self, h):
        return 8

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def test_python_mirrors_pass_the_flag_and_shape_the_replies(monkeypatch):
    pp = _params()
    q = [int(v) for v in pp.encryption_parameters.coeff_modulus[:-1]]
    words = rpm.ct_words(N, q)
    lib = _RecordingLib()
    monkeypatch.setattr(capi, "load", lambda: lib)
    for kw, flag in [({}, 0), ({"packed_replies": False}, 0), ({"packed_replies": True}, 16),
                     ({"packed_replies": True, "streamed": True}, 17)]:
        del lib.calls[:]
        db = PIRDatabase(pp, **kw)
        db._h = None        # nothing to destroy
        assert [(n, a[1]) for n, a in lib.calls] == [("pirgpu_create_ex", flag)]
    db = PIRDatabase.Create(pp, packed_replies=True)
    db._h = None
    assert lib.calls[-1][0] == "pirgpu_create_ex" and lib.calls[-1][1][1] == 16
    # an unpacked context: residue arrays as before
    assert db.reply_packing() is False and db.reply_ct_shape() == (2, len(q), N)
    srv = PIRServer(db, pp)
    query = np.zeros((1, 2, len(q), N), dtype=np.uint64)
    assert srv.process_query(query).shape[1:] == (2, len(q), N)
    # a packed one: (reply_cts, words) arrays from every reply path
    lib.packing, lib.words = 1, words
    assert db.reply_packing() is True and db.reply_ct_shape() == (words,)
    got = np.empty((8, words), dtype=np.uint64)
    del lib.calls[:]
    assert srv.process_query(query).shape[1:] == got.shape[1:]
    assert srv.fetch_reply().shape[1:] == (words,)
    srv._batch_count = 3
    assert srv.fetch_batch().shape == (3, 8, words)
    assert db._packed_words(len(q)) == words and db._packed_words(1) == rpm.ct_words(N, q, 1)
    # unpack_replies: any leading shape, through pirgpu_reply_unpack at the reply's primes
    del lib.calls[:]
    out = srv.unpack_replies(np.zeros((3, 8, words), dtype=np.uint64))
    assert out.shape == (3, 8, 2, len(q), N)
    (name, args), = lib.calls
    assert name == "pirgpu_reply_unpack" and args[2] == 24 and args[3] == len(q)
    with pytest.raises(PirGpuError):
        db.reply_unpack(np.zeros((1, words + 1), dtype=np.uint64), len(q))
    with pytest.raises(PirGpuError):
        db.reply_pack(np.zeros((1, 2, len(q), N), dtype=np.uint64), len(q) + 1)


@pytest.fixture(scope="module")
def world():
    """10 x 10 plaintexts at N = 4096, [36, 36] + 37, 20-bit t: the oracle's reply to a product client's query."""
    s = PirSetup(100, 0, 2, N=N, plain_bits=20)
    pp = to_product_params(s.params)
    client = pir_amd.PIRClient.Create(pp, seed=b"packed-api")
    index = 57
    rc, reply = s.orc.process_query(s.db_ntt, s.params.dimensions, client.create_query_for(index), client.galois_keys())
    assert rc == 0
    return s, pp, client, index, reply


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


def test_client_unpack_reply_is_the_models_unpack(world):
    s, pp, client, index, reply = world
    q = [int(x) for x in s.orc.moduli[:2]]
    packed = rpm.pack(reply, q)
    assert client.packed_reply_ct_words == packed.shape[1] == rpm.ct_words(N, q)
    assert np.array_equal(client.unpack_reply(packed), reply)
    assert np.array_equal(client.unpack_reply(packed.reshape(2, 4, -1)), reply.reshape(2, 4, 2, 2, N))
    bad = packed.copy()
    w0 = rpm.width(q[0])
    bad[3, 0] |= np.uint64((1 << w0) - 1)       # coefficient 0 of polynomial (0, 0): 2^w - 1 >= q_0
    with pytest.raises(PirGpuError) as e:
        client.unpack_reply(bad)
    assert e.value.code == capi.INVALID_ARGUMENT


def test_packed_wire_form_round_trips_and_is_shorter_by_the_computed_bytes(world):
    s, pp, client, index, reply = world
    q = [int(x) for x in s.orc.moduli[:2]]
    packed = rpm.pack(reply, q)
    plain = _save("pirgpu_wire_save_reply", pp, reply)
    blob = _save("pirgpu_wire_save_reply_packed", pp, packed)
    # per ciphertext: the coefficient words shrink, and with them two varint lengths may
    saved = reply.shape[0] * (2 * 2 * N - packed.shape[1]) * 8
    assert 0 <= len(plain) - len(blob) - saved <= 2 * (reply.shape[0] + 1)
    assert client.ProcessResponse([index], blob) == [s.item(index)]
    assert client.ProcessResponse([index], plain) == [s.item(index)]
    assert np.array_equal(client.LoadResponse(blob)[0], reply)
    assert np.array_equal(client.LoadResponse(blob + blob + blob), np.stack([reply] * 3))
    # the object: outer header, parms_id and shape fields as SEAL writes them; inner header byte 5 = 0x80, count 2 k N
    inner = seal_wire._parse(seal_wire._parse(blob)[0][1])
    inner_plain = seal_wire._parse(seal_wire._parse(plain)[0][1])
    assert len(inner) == len(inner_plain) == reply.shape[0]
    for i, ((_, a), (_, b)) in enumerate(zip(inner, inner_plain)):
        a, b = bytes(a), bytes(b)
        head = 16 + 32 + 1 + 4 * 8
        assert a[:8] == b[:8] and a[16:head] == b[16:head]
        assert int.from_bytes(a[8:16], "little") == len(a)
        assert a[head:head + 8] == b[head:head + 5] + b"\x80" + b[head + 6:head + 8]
        assert int.from_bytes(a[head + 8:head + 16], "little") == 16 + 8 + packed.shape[1] * 8
        assert int.from_bytes(a[head + 16:head + 24], "little") == 2 * 2 * N
        assert a[head + 24:] == packed[i].astype("<u8").tobytes()
    # a stock loader fails cleanly on it: the independent codec knows compression bytes 0 and 1 only
    with pytest.raises(Exception):
        seal_wire.load_response(blob)


def test_packed_wire_data_at_or_above_a_modulus_is_rejected(world):
    s, pp, client, index, reply = world
    q = [int(x) for x in s.orc.moduli[:2]]
    packed = rpm.pack(reply, q)
    packed[5, 0] |= np.uint64((1 << rpm.width(q[0])) - 1)
    blob = _save("pirgpu_wire_save_reply_packed", pp, packed)
    for call in (lambda: client.ProcessResponse([index], blob), lambda: client.LoadResponse(blob)):
        with pytest.raises(PirGpuError) as e:
            call()
        assert e.value.code == capi.INVALID_ARGUMENT and "out of range" in str(e.value)
    good = _save("pirgpu_wire_save_reply_packed", pp, rpm.pack(reply, q))
    with pytest.raises(PirGpuError):
        client.ProcessResponse([index], good[:-9])


def test_packed_wire_form_composes_with_result_primes(world):
    """r = 1: the reply's level, parms_id and count are those of result_primes; the words are the packed first prime."""
    import modswitch_model as M
    s, pp0, client0, index, _ = world
    pp = to_product_params(s.params)
    pp.result_primes = 1
    client = pir_amd.PIRClient.Create(pp, seed=b"packed-api-r1")
    rc, sv = s.orc.oblivious_expansion_multi(client.create_query_for(index), s.params.dim_sum, client.galois_keys())
    assert rc == 0
    reply = M.multiply_switched(s.orc, s.db_ntt, s.params.dimensions, sv, 1)
    q = [int(x) for x in s.orc.moduli[:1]]
    packed = rpm.pack(reply, q)
    assert packed.shape == (4, 2 * N * rpm.width(q[0]) // 64)
    blob = _save("pirgpu_wire_save_reply_packed", pp, packed)
    assert client.ProcessResponse([index], blob) == [s.item(index)]
    assert np.array_equal(client.LoadResponse(blob)[0], reply)
