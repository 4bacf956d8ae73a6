"""Compact queries on the client side (libpirclient.so), no GPU: what pirclient_set_compact_queries
changes about a request -- its size, its form on the wire, that the server-side validation accepts it -- and that the
symmetric query is the same selection as the public-key one, at a noise budget that is not below it.

The expanded query is rebuilt by the independent Python model (tests/query_compact_model.py: c1 from the seed through
hashlib's BLAKE2b) and decrypted by the client's own Decryptor, the one tests/test_client.py pins against the oracle
server: the client library hands out no secret key for the oracle client to decrypt with."""
import ctypes as C
import struct

import numpy as np
import pytest

import pir_amd
import query_compact_model as M
import seal_wire as W
from pir_amd import capi, parameters as P

N = 4096
CT_PREFIX = 16 + 32 + 33 + 16 + 8      # outer header, parms_id, members, array header, count


def make(dbsize=5000, d=2, elem=32, seed=b"compact-client", plain_bits=16):
    enc = P.generate_encryption_params(N, plain_bits)
    pp = P.create_pir_parameters(dbsize, elem, d, enc)
    return pir_amd.PIRClient.Create(pp, seed=seed), pp


def data_moduli(pp):
    return [int(v) for v in pp.encryption_parameters.coeff_modulus[:-1]]


def query_cts(request):
    """[[ciphertext bytes]] per query of a serialized Request."""
    return [[bytes(p) for n2, p in W._parse(bytes(payload)) if n2 == 1] for num, payload in W._parse(request) if num == 1]


def parse_compact_ct(buf, N, q, packed):
    """One compact ciphertext object -> the compact layout [words]; every header field checked on the way."""
    magic, hs, vmaj, _, compr, _, total = struct.unpack_from("<HBBBBHQ", buf, 0)
    assert magic == W.SEAL_MAGIC and hs == 16 and vmaj == 3 and compr == 0 and total == len(buf)
    is_ntt, size, n, nres, scale = struct.unpack_from("<BQQQd", buf, 48)
    assert (is_ntt, size, n, nres, scale) == (0, 2, N, len(q), 1.0)
    off = 48 + 33
    amagic, _, _, _, acompr, _, atotal = struct.unpack_from("<HBBBBHQ", buf, off)
    c0_bytes = M.wire_bytes(N, q, packed) - W.SEED_BYTES
    assert amagic == W.SEAL_MAGIC and acompr == (0x80 if packed else 0) and atotal == 16 + 8 + c0_bytes
    (count,) = struct.unpack_from("<Q", buf, off + 16)
    assert count == len(q) * N                                  # the count is in coefficients, packed or not
    assert len(buf) == off + atotal + W.SEED_BYTES              # the seed follows the array
    return np.frombuffer(buf, dtype="<u8", offset=off + 24).astype(np.uint64)


def validate(pp, request):
    lib = capi.load()                                           # host code of the server library: no device is touched
    lib.pirgpu_wire_validate_request.argtypes = [C.POINTER(capi.Params), C.POINTER(C.c_uint8), C.c_size_t,
                                                 C.POINTER(C.c_uint32)]
    lib.pirgpu_wire_validate_request.restype = C.c_int
    p, n = capi.make_params(pp), C.c_uint32()
    buf = (C.c_uint8 * len(request)).from_buffer_copy(request)
    return lib.pirgpu_wire_validate_request(C.byref(p), buf, len(request), C.byref(n)), n.value


def test_mode_0_is_todays_request_byte_for_byte():
    a, _ = make()
    b, _ = make()
    b.set_compact_queries(0)
    assert a.CreateRequest([1, 4999]) == b.CreateRequest([1, 4999])
    with pytest.raises(pir_amd.PirGpuError) as e:
        b.set_compact_queries(3)
    assert e.value.code == pir_amd.StatusCode.INVALID_ARGUMENT


@pytest.mark.parametrize("mode", [1, 2])
def test_compact_request_size_form_and_validation(mode):
    c, pp = make()
    q = data_moduli(pp)
    packed = mode == 2
    full = c.CreateRequest([1, 4999])
    c.set_compact_queries(mode)
    req = c.CreateRequest([1, 4999])
    assert validate(pp, req) == (0, 2)
    cts, full_cts = query_cts(req), query_cts(full)
    assert len(cts) == 2 and all(len(x) == c.query_ct_count for x in cts)
    words = c.query_compact_words(packed)
    assert words == M.words(N, q, packed)                       # the codec's count == the model's formula
    for query in cts:
        for ct in query:
            assert len(ct) == CT_PREFIX + 8 * words == CT_PREFIX + M.wire_bytes(N, q, packed)
            parse_compact_ct(ct, N, q, packed)
    # the request shrinks by exactly what its query fields shrink by: the key fields are the same bytes
    framed = lambda ql: sum(len(W._field(1, b"".join(W._field(1, x) for x in query))) for query in ql)
    assert len(full) - len(req) == framed(full_cts) - framed(cts)
    assert [p for n, p in W._parse(full) if n != 1] == [p for n, p in W._parse(req) if n != 1]
    if packed:
        assert len(full_cts[0][0]) / len(cts[0][0]) > 3.5


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("index", [0, 4999, 1234])
def test_compact_query_is_the_same_selection_at_no_less_budget(mode, index):
    c, pp = make(seed=b"compact-%d" % mode)
    q = data_moduli(pp)
    packed = mode == 2
    public = c.create_query_for(index)
    c.set_compact_queries(mode)
    (cts,) = query_cts(c.CreateRequest([index]))
    assert len(cts) == public.shape[0]
    for i, ct in enumerate(cts):
        obj = parse_compact_ct(ct, N, q, packed)
        expanded = M.expand(obj, N, q, packed)                  # c1 from the seed, by the Python model
        assert np.array_equal(c.decrypt(expanded), c.decrypt(public[i]))
        assert c.noise_budget(expanded) >= c.noise_budget(public[i])   # one error term against three


def test_residue_level_compact_query_and_save_request():
    c, pp = make(seed=b"compact-abi")
    q = data_moduli(pp)
    twin, _ = make(seed=b"compact-abi")
    for packed in (False, True):
        obj = c.create_query_compact(77, packed)
        assert obj.shape == (c.query_ct_count, M.words(N, q, packed))
        other = twin.create_query_compact(77, packed)           # a twin with the same seed, kept in step: deterministic
        assert np.array_equal(obj, other)
        expanded = M.expand_all(obj, N, q, packed)
        assert np.array_equal(c.decrypt(expanded[0]), c.decrypt(c.create_query_for(77)[0]))
        req = c.SaveRequestCompact([obj], packed)
        assert validate(pp, req) == (0, 1)
        (cts,) = query_cts(req)
        for i, ct in enumerate(cts):
            assert np.array_equal(parse_compact_ct(ct, N, q, packed), obj[i])
        twin.create_query_for(77)


def test_the_packed_byte_on_a_full_size_query_array_is_still_refused():
    """Only the seed-compressed form may be packed; on a full-size array the byte is refused as it was before
    (Unimplemented, like any compression byte: tests/cpp/reply_pack_test.cpp pins that status)."""
    c, pp = make(seed=b"compact-bad")
    req = bytearray(c.CreateRequest([5]))
    (cts,) = query_cts(bytes(req))
    at = bytes(req).index(cts[0]) + 48 + 33 + 5
    assert req[at] == 0
    req[at] = 0x80
    rc, _ = validate(pp, bytes(req))
    assert rc == pir_amd.StatusCode.UNIMPLEMENTED
