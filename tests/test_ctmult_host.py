"""Host side of the ciphertext-multiplication mode, no GPU: pirgpu_ctmult_plan against the Python
restatement in tests/ctmult_model.py over the supported chains and the chains of the GPU ladder, the bound at its edge
(the largest plain modulus two 30-bit primes take), the refusals that need no device, the new symbols and the flag
value."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ctmult_model as M
import oracle
from pir_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plan(N, q, special, t):
    lib = capi.load()
    qa = (C.c_uint64 * max(len(q), 1))(*q)
    aux = (C.c_uint64 * 16)()
    n = C.c_uint32(99)
    rc = lib.pirgpu_ctmult_plan(N, len(q), qa, special, t, aux, C.byref(n))
    return rc, [int(aux[i]) for i in range(n.value)], lib.pirgpu_create_error().decode()


CHAINS = [(2048, [54], 16), (2048, [27, 27], 16), (4096, [36, 36], 16), (4096, [36, 36], 24), (4096, [36, 36, 37], 20),
          (4096, [60, 60, 60], 20), (4096, [60, 60], 59), (8192, [43, 43, 44, 44], 42), (8192, [50] * 6, 30),
          (16384, [48, 48, 48, 49, 49], 20), (16384, [60] * 6, 59), (8192, [30, 40, 50], 20)]


@pytest.mark.parametrize("N,bits,t_bits", CHAINS + [c[1:] for c in M.LADDER], ids=[None] * len(CHAINS) + [c[0] for c in M.LADDER])
def test_plan_matches_the_restatement(N, bits, t_bits):
    moduli = oracle.coeff_modulus_create(N, bits + [max(bits)])
    q, special = moduli[:-1], moduli[-1]
    t = oracle.plain_modulus_batching(N, t_bits)
    rc, aux, msg = plan(N, q, special, t)
    want, ok = M.plan(N, q, special, t)
    assert ok and rc == 0, msg
    assert aux == want and len(aux) == len(q) + 2
    assert len(set(aux) | set(moduli)) == len(aux) + len(moduli)                 # distinct, from the chain too
    top = max(q).bit_length()
    for b in aux:
        assert oracle.is_prime(b) and b % (2 * N) == 1 and b.bit_length() == top
    Q, B = M.prod(q), M.prod(aux)
    assert Q * B > 2 * (t * N * (Q - 1) ** 2 // 2 + Q) and B > 2 * (t * N * Q + 2)


def test_the_bound_is_tight_for_two_30_bit_primes():
    """(4096, [30, 30]): of the batching primes of 14 ... 60 bits the plan takes every one up to 46 bits and none above,
    in the library and in the restatement alike.  At 46 bits both bounds are within a factor 8 of failing -- Q B over
    t N (Q - 1)^2 + 2 Q is about 2^2, B over 2 (t N Q + 2) about 2^1 -- against 2^43 for the default chain and a 16-bit t:
    the GPU rung "k2-tight" multiplies at this t, where a bound too generous by more than that would give wrong bits."""
    N = 4096
    moduli = oracle.coeff_modulus_create(N, [30, 30, 30])
    q, special = moduli[:-1], moduli[-1]
    verdict = {}
    for t_bits in range(14, 61):
        try:
            t = oracle.plain_modulus_batching(N, t_bits)
        except ValueError:                      # no prime == 1 mod 2N of that size (14 bits)
            continue
        rc, aux, msg = plan(N, q, special, t)
        want, ok = M.plan(N, q, special, t)
        assert (rc == 0) == ok, t_bits
        if ok:
            assert aux == want
        else:
            assert rc == capi.INVALID_ARGUMENT and aux == [] and "auxiliary base" in msg, t_bits
        verdict[t_bits] = ok
    assert len(verdict) >= 40 and 60 in verdict
    assert max(b for b, ok in verdict.items() if ok) == 46
    assert [b for b, ok in verdict.items() if not ok] == [b for b in verdict if b > 46]
    t = oracle.plain_modulus_batching(N, 46)
    Q, B = M.prod(q), M.prod(M.plan(N, q, special, t)[0])
    slack1, slack2 = Q * B / (t * N * (Q - 1) ** 2 + 2 * Q), B / (2 * (t * N * Q + 2))
    print("46-bit t: slack of the two bounds 2^%.2f and 2^%.2f" % (np.log2(slack1), np.log2(slack2)))
    assert 1 < slack1 < 8 and 1 < slack2 < 4


def test_the_special_prime_is_skipped():
    """SEAL hands the largest prime of a size to the special prime: the rule must walk past it."""
    N = 4096
    moduli = oracle.coeff_modulus_create(N, [36, 36, 36])
    rc, aux, _ = plan(N, moduli[:-1], moduli[-1], 65537)
    assert rc == 0 and moduli[-1] not in aux and not set(aux) & set(moduli)
    rc2, aux2, _ = plan(N, moduli[:-1], 0, 65537)
    assert rc2 == 0 and aux2[0] == moduli[-1]              # ... which it would have taken first otherwise


def test_seven_primes_and_a_base_that_is_too_small_are_refused():
    N = 4096
    moduli = oracle.coeff_modulus_create(N, [40] * 8)
    rc, aux, msg = plan(N, moduli[:7], moduli[7], 65537)
    assert rc == capi.INVALID_ARGUMENT and aux == [] and "6 data primes" in msg
    # two extra 30-bit primes hold 2^60, t N is 2^71
    moduli = oracle.coeff_modulus_create(N, [30, 30, 30])
    t = oracle.plain_modulus_batching(N, 59)
    rc, aux, msg = plan(N, moduli[:-1], moduli[-1], t)
    assert rc == capi.INVALID_ARGUMENT and aux == [] and "auxiliary base" in msg
    assert M.plan(N, moduli[:-1], moduli[-1], t)[1] is False
    # the same chain with a small plain modulus is fine
    assert plan(N, moduli[:-1], moduli[-1], 65537)[0] == 0
    assert plan(N, [], 0, 65537)[0] == capi.INVALID_ARGUMENT


def test_symbols_and_flag_value():
    lib = capi.load()
    with open(os.path.join(ROOT, "include", "pirgpu.h")) as f:
        header = f.read()
    for name in ("pirgpu_ctmult_plan", "pirgpu_ct_multiply", "pirgpu_relinearize"):
        assert re.search(r"\bint %s\(" % name, header) and hasattr(lib, name) and name in capi.SIGNATURES
    m = re.search(r"#define PIRGPU_CREATE_CT_MULTIPLY (\d+)u\b", header)
    assert m and int(m.group(1)) == capi.CREATE_CT_MULTIPLY == 4
    assert capi.CREATE_CT_MULTIPLY & capi.CREATE_STREAMED_DB == 0


def test_python_mirror_passes_the_flag():
    import inspect

    import pir_amd
    assert "ct_multiplication" in inspect.signature(pir_amd.PIRDatabase.Create).parameters
    assert hasattr(pir_amd.PIRServer, "set_relin_key")
