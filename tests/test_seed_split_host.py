"""The wire layer's splitting loader (split_kswitch_keys, through its device-free export): what a seed-compressed
GaloisKeys / RelinKeys object is taken apart into for the device's seed expansion -- the c0 halves and the seeds it
was written from --, its verdict on expanded and mixed objects, and its errors against the expanding loader's.
Also: the new C ABI entry points are declared, exported and bound.  No GPU."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import oracle
import seal_wire as W
from pir_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    lib = capi.load()
    lib.pirgpu_wire_split_kswitch_key.argtypes = [C.POINTER(capi.Params), C.POINTER(C.c_uint8), C.c_size_t, C.c_uint64,
                                                  C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint64),
                                                  C.POINTER(C.c_uint8), C.c_char_p, C.c_size_t]
    lib.pirgpu_wire_split_kswitch_key.restype = C.c_int
    lib.pirgpu_wire_load_kswitch_error.argtypes = [C.POINTER(capi.Params), C.POINTER(C.c_uint8), C.c_size_t, C.c_char_p,
                                                   C.c_size_t]
    lib.pirgpu_wire_load_kswitch_error.restype = C.c_int
    return lib


def _params(N, moduli, t):
    p = capi.Params()
    p.poly_modulus_degree, p.num_data_primes = N, len(moduli) - 1
    for i, q in enumerate(moduli[:-1]):
        p.coeff_modulus[i] = q
    p.special_prime, p.plain_modulus = moduli[-1], t
    p.num_dimensions, p.num_pt = 1, 10
    p.dimensions[0] = 10
    return p


def _split(lib, p, blob, index, k, km, N, offset=0):
    raw = (C.c_uint8 * (len(blob) + offset + 1)).from_buffer_copy(bytes(offset) + blob + b"\0")
    buf = C.cast(C.addressof(raw) + offset, C.POINTER(C.c_uint8))
    all_seeded, found = C.c_int(-1), C.c_int(-1)
    c0 = np.zeros((k, km, N), dtype=np.uint64)
    seeds = np.zeros(64 * k, dtype=np.uint8)
    err = C.create_string_buffer(256)
    rc = lib.pirgpu_wire_split_kswitch_key(C.byref(p), buf, len(blob), index, C.byref(all_seeded), C.byref(found),
                                           c0.ctypes.data_as(capi.u64p), seeds.ctypes.data_as(capi.u8p), err, 256)
    return rc, err.value.decode(), all_seeded.value, found.value, c0, seeds.tobytes()


def _load_error(lib, p, blob):
    buf = (C.c_uint8 * max(len(blob), 1)).from_buffer_copy(blob if blob else b"\0")
    err = C.create_string_buffer(256)
    rc = lib.pirgpu_wire_load_kswitch_error(C.byref(p), buf, len(blob), err, 256)
    return rc, err.value.decode()


CHAINS = [(2048, oracle.coeff_modulus_create(2048, [27, 27]), 12289), (4096, oracle.BFV_DEFAULT[4096], 0xFFC001)]


def _keys(N, moduli, elts, rng):
    k, km = len(moduli) - 1, len(moduli)
    keys, seeds = {}, {}
    for g in elts:
        key = np.empty((k, 2, km, N), dtype=np.uint64)
        for i, q in enumerate(moduli):
            key[:, :, i, :] = rng.integers(0, q, size=(k, 2, N), dtype=np.uint64)
        keys[g] = key
        seeds[g] = [rng.integers(0, 256, 64, dtype=np.uint8).tobytes() for _ in range(k)]
    return keys, seeds


@pytest.mark.parametrize("N,moduli,t", CHAINS, ids=["2048-k1", "4096-k2"])
def test_split_gives_back_the_halves_and_seeds(N, moduli, t):
    lib, p = _lib(), _params(N, moduli, t)
    k, km = len(moduli) - 1, len(moduli)
    keys, seeds = _keys(N, moduli, (3, N + 1, N // 2 + 1), np.random.default_rng(N))
    blob = W.save_galois_keys_seeded(keys, seeds, N, W.parms_id(N, moduli, t))
    for g in keys:
        rc, msg, all_seeded, found, c0, sd = _split(lib, p, blob, (g - 1) // 2, k, km, N)
        assert (rc, msg, all_seeded, found) == (0, "", 1, 1)
        assert np.array_equal(c0, keys[g][:, 0])
        assert sd == b"".join(seeds[g])
    rc, _, all_seeded, found, _, _ = _split(lib, p, blob, 2, k, km, N)      # no key at that index
    assert (rc, all_seeded, found) == (0, 1, 0)
    # the bytes of the object at an odd address: the halves lie at any alignment
    rc, _, all_seeded, found, c0, _ = _split(lib, p, blob, 1, k, km, N, offset=3)
    assert found == 1 and np.array_equal(c0, keys[3][:, 0])


@pytest.mark.parametrize("N,moduli,t", CHAINS, ids=["2048-k1", "4096-k2"])
def test_expanded_and_mixed_objects_are_not_all_seeded(N, moduli, t):
    lib, p = _lib(), _params(N, moduli, t)
    k, km = len(moduli) - 1, len(moduli)
    pid = W.parms_id(N, moduli, t)
    keys, seeds = _keys(N, moduli, (3, 5), np.random.default_rng(1))
    expanded = W.save_galois_keys(keys, N, pid)
    rc, _, all_seeded, found, _, _ = _split(lib, p, expanded, 1, k, km, N)
    assert (rc, all_seeded, found) == (0, 0, 0)
    # mixed: entry 1 (element 3) seeded, entry 2 (element 5) expanded
    s3 = W.save_galois_keys_seeded({3: keys[3]}, {3: seeds[3]}, N, pid)
    e5 = W.save_galois_keys({5: keys[5]}, N, pid)
    entry3 = s3[16 + 32 + 8 + 8:]                       # header, parms_id, dim1, the empty entry 0 -> entry 1 on
    entry5 = e5[16 + 32 + 8 + 8 + 8:]                   # ... entries 0 and 1 empty -> entry 2 on
    body = pid + struct.pack("<Q", 3) + struct.pack("<Q", 0) + entry3 + entry5
    mixed = W.header(16 + len(body)) + body
    assert _load_error(lib, p, mixed) == (0, "")
    rc, _, all_seeded, found, _, _ = _split(lib, p, mixed, 1, k, km, N)
    assert (rc, all_seeded, found) == (0, 0, 0)


def test_errors_are_the_expanding_loaders():
    N, moduli, t = CHAINS[0]
    lib, p = _lib(), _params(N, moduli, t)
    k, km = 1, 2
    pid = W.parms_id(N, moduli, t)
    keys, seeds = _keys(N, moduli, (3, 5), np.random.default_rng(2))
    good = W.save_galois_keys_seeded(keys, seeds, N, pid)
    first_word = 16 + 32 + 8 + 8 + 8 + 16 + 16 + 32 + 33 + 16 + 8       # ... of entry 1's c0 (after the empty entry 0)
    assert struct.unpack_from("<Q", good, first_word - 8)[0] == km * N

    def patched(offset, value):
        b = bytearray(good)
        b[offset:offset + 8] = struct.pack("<Q", value)
        return bytes(b)

    def resized(blob):                                   # the outer header's size follows the bytes
        return W.header(len(blob)) + blob[16:]

    cases = {
        "empty": b"",
        "truncated": good[:-9],
        "truncated, outer size adjusted": resized(good[:-9]),
        "seed cut off": resized(good[:-3]),
        "bad magic": b"\x00\x00" + good[2:],
        "wrong parms_id": good[:16] + bytes(32) + good[48:],
        "dim1 too large": patched(48, N + 1),
        "decomposition count": patched(64, k + 1),
        "inner header": good[:72] + b"\xff\xff" + good[74:],
        "inner parms_id": good[:72 + 32] + bytes(32) + good[72 + 64:],
        "coefficient count": patched(first_word - 8, km * N - 1),
        "c0 coefficient equal to its modulus": patched(first_word, moduli[0]),
        "c0 coefficient of the special prime's residue out of range": patched(first_word + 8 * (N + 5), moduli[1]),
        "last c0 coefficient of the second key out of range": patched(len(good) - 64 - 8, moduli[1] + 7),
    }
    for name, blob in cases.items():
        want = _load_error(lib, p, blob)
        assert want[0] != 0 and want[1], name
        rc, msg, all_seeded, found, _, _ = _split(lib, p, blob, 1, k, km, N)
        assert (rc, msg) == want, name
        assert found == 0, name
    rc, msg, _, _, _, _ = _split(lib, p, cases["c0 coefficient equal to its modulus"], 1, k, km, N)
    assert (rc, msg) == (3, "ciphertext data is invalid (coefficient out of range)")


def test_new_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "pirgpu.h")).read()
    whdr = open(os.path.join(ROOT, "pir_amd", "csrc", "wire.h")).read()
    lib = capi.load()
    for name in ("pirgpu_keyset_set_keys_seeded", "pirgpu_expand_seeds", "pirgpu_keyset_seed_stats"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in capi.SIGNATURES, name
    for name in ("pirgpu_wire_split_kswitch_key", "pirgpu_wire_load_kswitch_error"):
        assert re.search(r"\b%s\s*\(" % name, whdr), name
        assert hasattr(lib, name), name
