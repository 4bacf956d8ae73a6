"""Compact replies of the ciphertext-multiplication mode (PIRGPU_CREATE_CT_COMPACT_REPLY) -- the
host-side contract, no GPU: the flag's value and its neighbours, the Python mirror, and the product client on replies
the CPU models build: process_query_ct on the reference's 9-item tuple (correctness_test.cpp:99: N = 4096, 16-bit t, 10
bits per coefficient, index 5), switched to one prime by modswitch_model.switch_residues, packed by reply_pack_model.pack
and saved by the server's serialiser (device-free hook).

The product client's seed is fixed; with it the model's reply keeps a positive budget at level 1 and at level k (the
module fixture asserts both), as with the oracle client's seeds of tools/ct_compact_noise_table.py.

Every test fails without the feature: the constant does not exist there, and the client decrypts a reply of the mode at
k primes whatever result_primes says."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

import ctmult_model as CM
import modswitch_model as M
import pir_amd
import reply_pack_model as rpm
from gpu_helpers import to_product_params
from pir_amd import capi
from pir_amd.server import PIRDatabase, PirGpuError
from pir_fixtures import PirSetup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096
INDEX = 5
SEED = b"ct-compact-host"


def test_flag_value_and_its_neighbours():
    header = open(os.path.join(ROOT, "include", "pirgpu.h")).read()
    m = re.search(r"#define PIRGPU_CREATE_CT_COMPACT_REPLY (\d+)u\b", header)
    assert m and int(m.group(1)) == 64 == capi.CREATE_CT_COMPACT_REPLY
    others = [capi.CREATE_STREAMED_DB, capi.CREATE_CT_MULTIPLY, capi.CREATE_CT_DEFERRED, capi.CREATE_PACKED_REPLIES]
    assert others == [1, 4, 8, 16]
    for name, v in zip(("STREAMED_DB", "CT_MULTIPLY", "CT_DEFERRED", "PACKED_REPLIES"), others):
        assert re.search(r"#define PIRGPU_CREATE_%s %du\b" % (name, v), header), name
        assert v & capi.CREATE_CT_COMPACT_REPLY == 0, name
    assert bin(capi.CREATE_CT_COMPACT_REPLY).count("1") == 1


def _create_ex(cp, flags):
    lib = capi.load()
    h = C.c_void_p()
    rc = lib.pirgpu_create_ex(C.byref(cp), flags, C.byref(h))
    msg = lib.pirgpu_create_error().decode()
    if h:
        lib.pirgpu_destroy(h)
    return rc, msg


@pytest.fixture(scope="module")
def world():
    """The 9-item tuple, a product client with result_primes = 1 and one with 0 under the same seed, and the model's
    reply to the first one's query at k primes -- computed once."""
    s = PirSetup(9, 0, 2, N=N, plain_bits=16, bits_per_coeff=10)
    assert list(s.params.dimensions) == [3, 3]
    pp0 = to_product_params(s.params)
    pp0.use_ciphertext_multiplication = True
    pp1 = to_product_params(s.params)
    pp1.use_ciphertext_multiplication = True
    pp1.result_primes = 1
    c1 = pir_amd.PIRClient.Create(pp1, seed=SEED)      # (pirclient_create with the mode and result_primes succeeds)
    c0 = pir_amd.PIRClient.Create(pp0, seed=SEED)
    query = c1.create_query_for(INDEX)
    rc, reply = CM.process_query_ct(s.orc, s.db_ntt, s.params.dimensions, query, c1.galois_keys(), c1.relin_key())
    assert rc == 0 and reply.shape == (1, 2, 2, N)
    q = [int(v) for v in s.orc.moduli[:2]]
    switched = M.switch_residues(reply, q, 1)
    assert c0.noise_budget(reply[0]) > 0 and c0.noise_budget_level(switched[0], 1) > 0
    reply.setflags(write=False)
    switched.setflags(write=False)
    return s, (pp0, c0), (pp1, c1), query, reply, switched, q


def test_refusals_found_before_a_device_is_looked_for(world):
    s, (pp0, _), (pp1, _), *_ = world
    plain = to_product_params(s.params)
    rc, msg = _create_ex(capi.make_params(plain), 64)                       # without the CT flag
    assert rc == capi.INVALID_ARGUMENT and "PIRGPU_CREATE_CT_COMPACT_REPLY" in msg, (rc, msg)
    rc, msg = _create_ex(capi.make_params(pp0), 64 | 16 | 4)                # flag 16 beside the CT flag stays refused
    assert rc == capi.INVALID_ARGUMENT and "PIRGPU_CREATE_PACKED_REPLIES" in msg, (rc, msg)
    rc, msg = _create_ex(capi.make_params(pp1), 4)                          # result_primes without 64 stays refused
    assert rc == capi.INVALID_ARGUMENT and "result_primes" in msg, (rc, msg)
    for flags in (2, 3, 16 | 2, 32 | 16, 64 | 32, 64 | 2):
        rc, msg = _create_ex(capi.make_params(plain), flags)
        assert rc == capi.INVALID_ARGUMENT and "flags" in msg, (flags, rc, msg)
    for kw, word in [(dict(shard=(0, 2)), "row shard"), (dict(slots=(0, 1024)), "slot shard")]:
        rc, msg = _create_ex(capi.make_params(pp1, **kw), 64 | 4)
        assert rc == capi.INVALID_ARGUMENT and word in msg, (kw, rc, msg)
    rc, msg = _create_ex(capi.make_params(pp1), 64 | 4 | 1)
    assert rc == capi.INVALID_ARGUMENT and "STREAMED" in msg, (rc, msg)


class _RecordingLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


def test_python_mirror_passes_the_flag(monkeypatch, world):
    _, (pp0, _), (pp1, _), *_ = world
    lib = _RecordingLib()
    monkeypatch.setattr(capi, "load", lambda: lib)
    for make in (PIRDatabase, PIRDatabase.Create):
        for kw, flag in [(dict(ct_multiplication=True), 4), (dict(ct_multiplication=True, ct_compact_reply=True), 68),
                         (dict(ct_multiplication=True, ct_deferred=True, ct_compact_reply=True), 76),
                         (dict(ct_multiplication=True, ct_compact_reply=False), 4)]:
            del lib.calls[:]
            db = make(pp1, **kw)
            db._h = None
            assert [(n, a[1]) for n, a in lib.calls] == [("pirgpu_create_ex", flag)], kw


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


def test_client_recovers_the_item_from_a_switched_reply_in_both_forms(world):
    s, (pp0, c0), (pp1, c1), query, reply, switched, q = world
    assert c1.reply_k == 1 and c1.reply_ct_count == 1
    # residues, through pirclient_process_reply: decrypted at level 1
    pt = c1.process_reply(switched)
    assert np.array_equal(pt, c1.decrypt_level(switched[0], 1))
    item = s.item(INDEX)
    assert c1.string_decode(pt, len(item), 0) == item
    # the packed response, through pirclient_process_response
    packed = rpm.pack(switched, q)
    assert packed.shape == (1, rpm.ct_words(N, q, 1)) == (1, c1.packed_reply_ct_words)
    blob = _save("pirgpu_wire_save_reply_packed", pp1, packed)
    assert len(blob) < 8 * packed.shape[1] + 256
    assert c1.ProcessResponse([INDEX], blob) == [item]
    assert np.array_equal(c1.LoadResponse(blob)[0], switched)
    assert np.array_equal(c1.unpack_reply(packed), switched)
    # and the same level unpacked on the wire
    assert c1.ProcessResponse([INDEX], _save("pirgpu_wire_save_reply", pp1, switched)) == [item]


def test_the_switched_client_refuses_a_reply_at_k_primes(world):
    s, (pp0, c0), (pp1, c1), query, reply, switched, q = world
    # (the control: this is the client that reads the level-1 reply)
    assert c1.string_decode(c1.process_reply(switched), len(s.item(INDEX)), 0) == s.item(INDEX)
    for blob in (_save("pirgpu_wire_save_reply", pp0, reply), _save("pirgpu_wire_save_reply_packed", pp0, rpm.pack(reply, q))):
        assert c0.ProcessResponse([INDEX], blob) == [s.item(INDEX)]          # what the k-prime client reads
        for call in (lambda: c1.ProcessResponse([INDEX], blob), lambda: c1.LoadResponse(blob)):
            with pytest.raises(PirGpuError) as e:
                call()
            assert e.value.code == capi.INVALID_ARGUMENT
    with pytest.raises(PirGpuError):                                          # and the other way round
        c0.ProcessResponse([INDEX], _save("pirgpu_wire_save_reply_packed", pp1, rpm.pack(switched, q)))


# sha256 of CreateRequest([1, 5]) of the product client with the mode's parameters of the 9-item tuple, result_primes = 0
# and seed SEED, recorded from a build of the commit before this flag existed
REQUEST_SHA256_BEFORE = "0d1d4f15a3783727179f8d6cb3e1eef5310a6ca41e726222fafe34a69fca7ebc"


def test_a_client_without_result_primes_is_the_client_of_before(world):
    s, (pp0, c0), (pp1, c1), query, reply, switched, q = world
    fresh0 = pir_amd.PIRClient.Create(pp0, seed=SEED)
    fresh1 = pir_amd.PIRClient.Create(pp1, seed=SEED)
    request = fresh0.CreateRequest([1, INDEX])
    assert hashlib.sha256(request).hexdigest() == REQUEST_SHA256_BEFORE
    assert request == fresh1.CreateRequest([1, INDEX])      # the request does not depend on the reply's level
    # the k-prime reply: process_reply is the decryption at the full modulus, as before (pirclient_decrypt is untouched)
    pt = c0.process_reply(reply)
    assert np.array_equal(pt, c0.decrypt(reply[0])) and np.array_equal(pt, c0.decrypt_level(reply[0], 2))
    assert c0.string_decode(pt, len(s.item(INDEX)), 0) == s.item(INDEX)
    assert capi.CREATE_CT_COMPACT_REPLY == 64               # (this file's tests all need the feature)
