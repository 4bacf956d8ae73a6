"""Deferred rounding of the ciphertext-multiplication mode on the CPU (tests/ctmult_deferred_model.py, DESIGN.md section
6.6): the definition -- a row's tensor products summed over the integers, ONE rounding, ONE relinearisation -- recovers
the item on the reference's d = 2 tuples with replies that differ in their bits from the per-child form, is the per-child
form on a row of one child and leaves d = 1 alone; the residue formulation the kernels use (sums mod q_j and mod b_i, then
the scale through the auxiliary base) agrees with the integers; pirgpu_ctmult_plan_terms is pirgpu_ctmult_plan at one
term and refuses exactly the first number of terms the two inequalities refuse; flag, exports and the refusal of the flag
on its own.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ctmult_deferred_model as D
import ctmult_model as M
import oracle
from gpu_helpers import to_product_params
from pir_amd import capi
from pir_fixtures import PirSetup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("N,t_bits,dbsize,bpc,index", [(4096, 16, 9, 10, 5), (4096, 16, 500, 6, 125)])
def test_deferred_query_recovers_the_item(N, t_bits, dbsize, bpc, index):
    s = PirSetup(dbsize, 0, 2, N=N, plain_bits=t_bits, bits_per_coeff=bpc)
    rk = M.relin_key(s.client)
    q = s.client.create_query_for(s.params, index)
    rc, reply = D.process_query_ct_deferred(s.orc, s.db_ntt, s.params.dimensions, q, s.galois_keys, rk)
    assert rc == 0 and reply.shape == (1, 2, s.orc.k, N)
    rc, per_child = M.process_query_ct(s.orc, s.db_ntt, s.params.dimensions, q, s.galois_keys, rk)
    assert rc == 0
    budget, budget_pc = s.client.noise_budget(reply[0]), s.client.noise_budget(per_child[0])
    print("%d items: noise budget of the reply %.2f bits deferred, %.2f bits per child" % (dbsize, budget, budget_pc))
    assert budget > 0 and budget_pc > 0
    assert M.process_response_ct(s.client, s.params, index, reply) == s.item(index)
    assert not np.array_equal(reply, per_child)         # another definition: the same item, other bits


def test_d1_is_the_oracles_process_query():
    s = PirSetup(10, 0, 1, N=4096, plain_bits=24)
    q = s.client.create_query_for(s.params, 3)
    rc, want = s.orc.process_query(s.db_ntt, s.params.dimensions, q, s.galois_keys)
    rc2, got = D.process_query_ct_deferred(s.orc, s.db_ntt, s.params.dimensions, q, s.galois_keys, None)
    assert rc == rc2 == 0 and np.array_equal(got, want)


def test_a_row_of_one_child_is_the_per_child_result():
    """dims [1, P]: the one upper row has one child, so its sum has one term."""
    s = PirSetup(3, 0, 2, N=4096, plain_bits=16)
    dims = [1, s.params.num_pt]
    rk = M.relin_key(s.client)
    q = s.client.create_query_for(s.params, 1)
    rc, sv = s.orc.oblivious_expansion_multi(q, sum(dims), s.galois_keys)
    assert rc == 0
    rc, want = M.levels_ct(s.orc, s.db_ntt, dims, sv, rk)
    rc2, got = D.levels_ct_deferred(s.orc, s.db_ntt, dims, sv, rk)
    assert rc == rc2 == 0 and np.array_equal(got, want)


LADDER = {c[0]: c[1:] for c in M.LADDER}


@pytest.mark.parametrize("N,bits,t_bits", [(4096, [36, 36], 16), LADDER["k3-mixed"], LADDER["k6-int"]],
                         ids=["default", "k3-mixed", "k6-int"])
def test_rns_formulation_of_a_sum_agrees_with_the_integers(N, bits, t_bits):
    """Polynomials of 64 coefficients, three pairs of the hook's family: the tensors summed in residues at Q and at B
    (what the row-sum kernel leaves), scaled by M.rns_scale, against scaled_residues of the integer sum."""
    moduli = oracle.coeff_modulus_create(N, bits + [max(bits)])
    q, t = [int(x) for x in moduli[:-1]], oracle.plain_modulus_batching(N, t_bits)
    aux, ok = D.plan_terms(N, q, moduli[-1], t, 3)
    assert ok and len(aux) == len(q) + 2
    names, A, B = M.hook_inputs(q, t, 64, np.random.default_rng(N), names=["random 0", "all q_j - 1", "full h"])
    xs = [M.tensor(A[i], B[i], q) for i in range(3)]
    want = D.multiply_ct_sum(A, B, q, t)
    assert np.array_equal(want, M.scaled_residues([[sum(v) for v in zip(*(x[m] for x in xs))] for m in range(3)], q, t))
    for m in range(3):
        def summed(base):
            acc = [[0] * 64 for _ in base]
            for x in xs:
                res = M.to_residues(x[m], base).tolist()
                acc = [[(u + v) % p for u, v in zip(ra, rr)] for ra, rr, p in zip(acc, res, base)]
            return np.array(acc, dtype=np.uint64)
        assert np.array_equal(M.rns_scale(summed(q), summed(aux), q, aux, t), want[m]), m


def plan_terms(N, q, special, t, terms):
    lib = capi.load()
    qa = (C.c_uint64 * max(len(q), 1))(*q)
    aux = (C.c_uint64 * 16)()
    n = C.c_uint32(99)
    rc = lib.pirgpu_ctmult_plan_terms(N, len(q), qa, special, t, terms, aux, C.byref(n))
    return rc, [int(aux[i]) for i in range(n.value)], lib.pirgpu_create_error().decode()


@pytest.mark.parametrize("N,bits,t_bits", [c[1:] for c in M.LADDER], ids=[c[0] for c in M.LADDER])
def test_plan_with_one_term_is_the_plan(N, bits, t_bits):
    moduli = oracle.coeff_modulus_create(N, bits + [max(bits)])
    q, special = [int(x) for x in moduli[:-1]], int(moduli[-1])
    t = oracle.plain_modulus_batching(N, t_bits)
    lib = capi.load()
    qa, aux, n = (C.c_uint64 * len(q))(*q), (C.c_uint64 * 16)(), C.c_uint32(0)
    assert lib.pirgpu_ctmult_plan(N, len(q), qa, special, t, aux, C.byref(n)) == 0
    rc, got, msg = plan_terms(N, q, special, t, 1)
    assert rc == 0, msg
    assert got == [int(aux[i]) for i in range(n.value)] == M.plan(N, q, special, t)[0]


def test_plan_refuses_the_first_number_of_terms_the_bounds_refuse():
    """k2-tight, (4096, [30, 30]) with the 46-bit t: the largest number of terms the two inequalities take, found here in
    Python integers, is accepted by the library, and one more is refused."""
    _, N, bits, t_bits = next(c for c in M.LADDER if c[0] == "k2-tight")
    moduli = oracle.coeff_modulus_create(N, bits + [max(bits)])
    q, special = [int(x) for x in moduli[:-1]], int(moduli[-1])
    t = oracle.plain_modulus_batching(N, t_bits)
    aux, ok = M.plan(N, q, special, t)
    assert ok
    Q, Bp = M.prod(q), M.prod(aux)
    terms = 1
    while Q * Bp > t * (terms + 1) * N * (Q - 1) ** 2 + 2 * Q and Bp > 2 * (t * (terms + 1) * N * Q + 2):
        terms += 1
    print("k2-tight: the auxiliary base holds a sum of %d products" % terms)
    assert terms < 64 and D.plan_terms(N, q, special, t, terms)[1] and not D.plan_terms(N, q, special, t, terms + 1)[1]
    rc, got, msg = plan_terms(N, q, special, t, terms)
    assert rc == 0 and got == aux, msg
    rc, got, msg = plan_terms(N, q, special, t, terms + 1)
    assert rc == capi.INVALID_ARGUMENT and got == [] and "auxiliary base" in msg, (rc, msg)


def test_flag_exports_and_python_mirrors():
    import inspect

    import pir_amd
    lib = capi.load()
    with open(os.path.join(ROOT, "include", "pirgpu.h")) as f:
        header = f.read()
    assert re.search(r"#define PIRGPU_CREATE_CT_DEFERRED 8u\b", header)
    assert capi.CREATE_CT_DEFERRED == 8
    assert capi.CREATE_CT_DEFERRED & (capi.CREATE_CT_MULTIPLY | capi.CREATE_STREAMED_DB) == 0
    for name in ("pirgpu_ctmult_plan_terms", "pirgpu_ct_multiply_sum"):
        assert re.search(r"\bint %s\(" % name, header) and hasattr(lib, name) and name in capi.SIGNATURES
    assert "ct_deferred" in inspect.signature(pir_amd.PIRDatabase.Create).parameters
    assert "ct_deferred" in inspect.signature(pir_amd.PIRDatabase.__init__).parameters
    assert hasattr(pir_amd.PIRDatabase, "ct_multiply_sum")
    with open(os.path.join(ROOT, "pir_amd", "csrc", "pir_facade.h")) as f:
        assert "bool ct_deferred = false" in f.read()


def test_the_flag_alone_is_invalid_argument_before_a_device_is_needed():
    lib = capi.load()
    cp = capi.make_params(to_product_params(oracle.create_pir_parameters(300, 288, 2, N=4096, plain_bits=24)))
    h = C.c_void_p()
    rc = lib.pirgpu_create_ex(C.byref(cp), capi.CREATE_CT_DEFERRED, C.byref(h))
    msg = lib.pirgpu_create_error().decode()
    assert not h
    assert rc == capi.INVALID_ARGUMENT and "PIRGPU_CREATE_CT_MULTIPLY" in msg, (rc, msg)
    # ... and with the streamed flag beside it, all the same
    rc = lib.pirgpu_create_ex(C.byref(cp), capi.CREATE_CT_DEFERRED | capi.CREATE_STREAMED_DB, C.byref(h))
    assert rc == capi.INVALID_ARGUMENT and not h
