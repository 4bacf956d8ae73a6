"""Modulus-switched results (pirgpu_params.result_primes) -- the host-side contract, no GPU: the struct field and its
ctypes mirror, the new exports, the CPU client at a prefix level of the modulus chain against the model of
tests/modswitch_model.py (decryption, noise budget, the recursive reply decode, the wire form of a switched reply), and
result_primes = 0 leaving the client as it was."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import modswitch_model as M
import oracle
import pir_amd
import seal_wire
from gpu_helpers import to_product_params
from pir_amd import capi
from pir_amd import parameters as P
from pir_amd.server import PirGpuError
from pir_fixtures import PirSetup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096


def test_struct_layout_and_trailing_field_match_the_header():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.c")
        open(src, "w").write('#include <stdio.h>\n#include "pirgpu.h"\nint main(){printf("%zu %zu %zu", '
                             'sizeof(pirgpu_params), __builtin_offsetof(pirgpu_params, result_primes), '
                             '__builtin_offsetof(pirgpu_params, plaintexts_per_item));return 0;}')
        exe = os.path.join(d, "s")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        size, off_r, off_planes = map(int, subprocess.run([exe], capture_output=True, text=True).stdout.split())
    assert C.sizeof(capi.Params) == size
    assert capi.Params.result_primes.offset == off_r == off_planes + 4
    assert capi.Params._fields_[-1][0] == "result_primes"           # the trailing field
    assert off_r + 4 <= size < off_r + 4 + 8                          # nothing but padding behind it


def test_new_exports_are_declared_bound_and_null_safe():
    header = open(os.path.join(ROOT, "include", "pirgpu.h")).read()
    lib = capi.load()
    for name, sig in [("pirgpu_reply_ct_words", (C.c_uint64, [C.c_void_p])),
                      ("pirgpu_mod_switch", (C.c_int, [C.c_void_p, capi.u64p, C.c_uint64, C.c_uint32, capi.u64p]))]:
        assert name in header and hasattr(lib, name) and capi.SIGNATURES[name] == sig
    assert lib.pirgpu_reply_ct_words(None) == 0
    assert lib.pirgpu_mod_switch(None, None, 0, 1, None) == capi.INVALID_ARGUMENT
    cheader = open(os.path.join(ROOT, "include", "pirclient.h")).read()
    clib = capi.load_client()
    for name in ("pirclient_decrypt_level", "pirclient_noise_budget_level"):
        assert name in cheader and hasattr(clib, name) and name in capi.CLIENT_SIGNATURES
    assert capi.CLIENT_SIGNATURES["pirclient_decrypt_level"] == (C.c_int, [C.c_void_p, capi.u64p, C.c_uint32, capi.u64p])
    assert clib.pirclient_decrypt_level(None, None, 1, None) == capi.INVALID_ARGUMENT


def test_parameters_carry_the_field():
    enc = P.generate_encryption_params(N, 20)
    pp = P.create_pir_parameters(100, 0, 2, enc, result_primes=1)
    assert pp.result_primes == 1 and capi.make_params(pp).result_primes == 1
    assert capi.make_params(P.create_pir_parameters(100, 0, 2, enc)).result_primes == 0
    for bad in (2, 3, -1):
        with pytest.raises(ValueError):
            P.create_pir_parameters(100, 0, 2, enc, result_primes=bad)
    pp.result_primes = 2                                              # r >= k: the client refuses it like the server
    with pytest.raises(PirGpuError) as e:
        pir_amd.PIRClient.Create(pp, seed=b"x")
    assert e.value.code == capi.INVALID_ARGUMENT


@pytest.fixture(scope="module")
def world():
    """10 x 10 plaintexts at N = 4096, [36, 36] + 37, 20-bit t; a model-made switched reply for the oracle client's
    query, and a product client whose ciphertexts the model cannot read (its key never leaves the library): the two sides
    meet on the product client's OWN queries, answered by the model with the product client's Galois keys."""
    s = PirSetup(100, 0, 2, N=N, plain_bits=20)
    pp = to_product_params(s.params)
    pp.result_primes = 1
    client = pir_amd.PIRClient.Create(pp, seed=b"modswitch-api")
    keys = client.galois_keys()
    index = 98
    q = client.create_query_for(index)
    rc, sv = s.orc.oblivious_expansion_multi(q, s.params.dim_sum, keys)
    assert rc == 0
    trace = []
    reply = M.multiply_switched(s.orc, s.db_ntt, s.params.dimensions, sv, 1, trace=trace)
    return s, pp, client, index, reply, trace


def test_client_reply_shape_follows_result_primes(world):
    s, pp, client, index, reply, trace = world
    assert client.reply_ct_count == 4 == reply.shape[0] and client.reply_k == 1
    full = pir_amd.PIRClient.Create(to_product_params(s.params), seed=b"modswitch-api")
    assert full.reply_ct_count == 8 and full.reply_k == 2


def test_process_reply_on_a_model_made_reply_returns_the_item(world):
    s, pp, client, index, reply, trace = world
    pt = client.process_reply(reply)
    assert client.string_decode(pt, pp.bytes_per_item, 0) == s.item(index)
    with pytest.raises(PirGpuError):
        client.process_reply(np.concatenate([reply, reply]))        # 8 ciphertexts: the count of the full modulus


def test_decrypt_level_equals_the_encode_of_the_switched_row(world):
    """The chunks the client decrypts at level 1 are the Encode of the switched level-1 ciphertext of the selected row
    (the model's own statement of what the reply encrypts), and they leave noise budget."""
    s, pp, client, index, reply, trace = world
    row = trace[0][index // 10][0]
    want = M.reencode_level(s.orc, row, 1)
    for i in range(4):
        assert np.array_equal(client.decrypt_level(reply[i], 1), want[i]), i
        assert client.noise_budget_level(reply[i], 1) >= 2
    with pytest.raises(PirGpuError):
        client.decrypt_level(reply[0], 0)
    with pytest.raises(PirGpuError):
        client.decrypt_level(reply[0], 3)


def test_decrypt_level_equals_the_model_on_the_oracle_clients_key():
    """pirclient_decrypt_level against modswitch_model.decrypt_level: a ciphertext of the product client, switched by the
    model, decrypts to the same plaintext at level 1 as at level 2, and level k is pirclient_decrypt itself."""
    enc = P.generate_encryption_params(N, 20)
    pp = P.create_pir_parameters(100, 0, 2, enc, result_primes=1)
    client = pir_amd.PIRClient.Create(pp, seed=b"lvl")
    rng = np.random.default_rng(5)
    pt = rng.integers(0, enc.plain_modulus, size=N, dtype=np.uint64)
    ct = client.encrypt(pt)
    assert np.array_equal(client.decrypt_level(ct, 2), client.decrypt(ct))
    assert client.noise_budget_level(ct, 2) == client.noise_budget(ct)
    low = M.switch_residues(ct, enc.coeff_modulus[:2], 1)
    assert low.shape == (2, 1, N)
    assert np.array_equal(client.decrypt_level(low, 1), pt)
    # a fresh ciphertext's noise is far below one prime: the switch leaves the rounding term, a budget near 36 - 20 bits
    assert 5 <= client.noise_budget_level(low, 1) <= 16


def test_process_response_on_model_made_wire_bytes(world):
    s, pp, client, index, reply, trace = world
    q = [int(x) for x in s.orc.moduli]
    pid1 = seal_wire.parms_id(N, q[:1], s.orc.t)
    response = seal_wire.save_response([reply], pid1)
    assert client.ProcessResponse([index], response) == [s.item(index)]
    assert np.array_equal(client.LoadResponse(response)[0], reply)
    # the same ciphertexts under the full level's parms_id are not a reply of this context
    with pytest.raises(PirGpuError):
        client.ProcessResponse([index], seal_wire.save_response([reply], seal_wire.parms_id(N, q[:2], s.orc.t)))


def test_product_codec_saves_a_level_r_reply_the_independent_codec_loads(world):
    """The server's serialiser (device-free hook) on a switched reply: tests/seal_wire.py loads every ciphertext with
    r residues and the r-prime parms_id; byte for byte what the independent codec writes."""
    s, pp, client, index, reply, trace = world
    lib = capi.load()
    lib.pirgpu_wire_save_reply.argtypes = [C.POINTER(capi.Params), capi.u64p, C.c_uint64, C.POINTER(C.c_void_p),
                                           C.POINTER(C.c_size_t)]
    lib.pirgpu_wire_save_reply.restype = C.c_int
    q = [int(x) for x in s.orc.moduli]
    for r, cts in ((1, reply), (0, np.ascontiguousarray(np.repeat(reply, 2, axis=2)))):   # (r = 0: k = 2 residues)
        p = capi.make_params(pp)
        p.result_primes = r
        out, n = C.c_void_p(), C.c_size_t()
        assert lib.pirgpu_wire_save_reply(C.byref(p), cts.ctypes.data_as(capi.u64p), cts.shape[0], C.byref(out),
                                          C.byref(n)) == 0
        blob = C.string_at(out, n.value)
        lib.pirgpu_free(out)
        pid = seal_wire.parms_id(N, q[:r or 2], s.orc.t)
        assert blob == seal_wire.save_response([cts], pid)
        (loaded,) = seal_wire.load_response(blob)
        assert loaded.shape == (4, 2, r or 2, N) and np.array_equal(loaded, cts)
        inner = seal_wire._parse(seal_wire._parse(blob)[0][1])
        assert all(seal_wire.load_ciphertext(bytes(c))[0] == pid for _, c in inner)


def test_result_primes_zero_leaves_the_client_as_it_was():
    """Same seed, result_primes 0: the same keys, the same request bytes, the full-modulus reply shape."""
    enc = P.generate_encryption_params(N, 20)
    a = pir_amd.PIRClient.Create(P.create_pir_parameters(100, 0, 2, enc), seed=b"same")
    b = pir_amd.PIRClient.Create(P.create_pir_parameters(100, 0, 2, enc, result_primes=1), seed=b"same")
    assert a.reply_ct_count == 8 and a.reply_k == 2 and b.reply_ct_count == 4
    # the request does not depend on the field
    assert a.CreateRequest([5, 77]) == b.CreateRequest([5, 77])
    # the oracle's full-modulus reply goes through the unchanged path
    s = PirSetup(100, 0, 2, N=N, plain_bits=20)
    qa = a.create_query_for(42)
    rc, rep = s.orc.process_query(s.db_ntt, s.params.dimensions, qa, a.galois_keys())
    assert rc == 0
    assert a.string_decode(a.process_reply(rep), s.params.bytes_per_item, 0) == s.item(42)
    response = seal_wire.save_response([rep], seal_wire.parms_id(N, [int(x) for x in s.orc.moduli[:2]], s.orc.t))
    assert a.ProcessResponse([42], response) == [s.item(42)]
