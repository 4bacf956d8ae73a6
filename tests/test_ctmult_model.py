"""The ciphertext-multiplication mode on the CPU (tests/ctmult_model.py): the definition of the
exact BFV product decrypts to the product of the plaintexts, the RNS / Garner formulation the kernels use agrees with the
big-integer definition on the hook's input family, and the query path recovers the item on the reference's d = 2 tuples
(correctness_test.cpp:99-101).  No GPU."""
import numpy as np
import pytest

import ctmult_model as M
import oracle
from oracle.client import Client
from pir_fixtures import PirSetup


def test_product_decrypts_to_the_product_of_the_plaintexts():
    N = 4096
    t = oracle.plain_modulus_batching(N, 16)
    orc = oracle.Oracle(N, oracle.BFV_DEFAULT[N], t)
    cl = Client(orc, seed=5)
    rng = np.random.default_rng(1)
    m1 = rng.integers(0, t, size=N, dtype=np.uint64)
    m2 = rng.integers(0, t, size=N, dtype=np.uint64)
    ct = M.mul_relin(orc, cl.encrypt(m1), cl.encrypt(m2), M.relin_key(cl))
    want = np.array([x % t for x in M.negacyclic_mul(m1.tolist(), m2.tolist())], dtype=np.uint64)
    budget = cl.noise_budget(ct)
    print("noise budget after one product + relinearisation: %.1f bits" % budget)
    assert budget > 0
    assert np.array_equal(cl.decrypt(ct), want)


@pytest.mark.parametrize("N,bits,t_bits", [(4096, [36, 36], 16), (8192, [43, 43, 44, 44], 42), (4096, [60, 60, 60], 20)] +
                         [c[1:] for c in M.LADDER], ids=[None] * 3 + [c[0] for c in M.LADDER])
def test_rns_formulation_agrees_with_the_integers(N, bits, t_bits):
    """Polynomials of 64 coefficients (the formulation is per coefficient; the bounds of the plan are those of the full
    ring degree, which cover the shorter products), on the chains of the GPU ladder too."""
    moduli = oracle.coeff_modulus_create(N, bits + [max(bits)])
    q, t = moduli[:-1], oracle.plain_modulus_batching(N, t_bits)
    aux, ok = M.plan(N, q, moduli[-1], t)
    assert ok and len(aux) == len(q) + 2
    n = 64
    names, A, B = M.hook_inputs(q, t, n, np.random.default_rng(N))
    M.check_hook_inputs(names, [M.tensor(A[i], B[i], q) for i in range(len(names))], q, t)
    for i, name in enumerate(names):
        for c in range(2):      # the lift alone
            want = M.to_residues(M.crt_lift(A[i, c], q), aux)
            assert np.array_equal(M.rns_lift(A[i, c], q, aux), want), name
        assert np.array_equal(M.rns_multiply_ct(A[i], B[i], q, aux, t), M.multiply_ct(A[i], B[i], q, t)), name


def test_rns_formulation_at_the_full_degree_on_the_tightest_chain():
    """(4096, [30, 30]) with the 46-bit t, the largest the plan takes (tests/test_ctmult_host.py): N = 4096 coefficients at h,
    which 64 coefficients cannot reach -- the top coefficient of x1 is 2 N h^2, the magnitude the bounds are stated for."""
    N = 4096
    moduli = oracle.coeff_modulus_create(N, [30, 30, 30])
    q, t = moduli[:-1], oracle.plain_modulus_batching(N, 46)
    aux, ok = M.plan(N, q, moduli[-1], t)
    assert ok
    names, A, B = M.hook_inputs(q, t, N, np.random.default_rng(N), names=["full h", "full h + 1"])
    assert names == ["full h", "full h + 1"]
    h = (M.prod(q) - 1) // 2
    for i, name in enumerate(names):
        x = M.tensor(A[i], B[i], q)
        assert x[0][N - 1] == N * h * h and x[1][N - 1] == 2 * N * h * h, name
        assert np.array_equal(M.rns_multiply_ct(A[i], B[i], q, aux, t), M.scaled_residues(x, q, t)), name


TUPLES = [(4096, 16, 9, 10, [1, 5]), (4096, 16, 500, 6, [9, 125]), (8192, 42, 87, 0, [5, 33, 86])]


@pytest.mark.parametrize("N,t_bits,dbsize,bpc,indices", TUPLES)
def test_query_recovers_the_item(N, t_bits, dbsize, bpc, indices):
    s = PirSetup(dbsize, 0, 2, N=N, plain_bits=t_bits, bits_per_coeff=bpc)
    rk = M.relin_key(s.client)
    index = indices[-1]
    q = s.client.create_query_for(s.params, index)
    rc, reply = M.process_query_ct(s.orc, s.db_ntt, s.params.dimensions, q, s.galois_keys, rk)
    assert rc == 0 and reply.shape == (1, 2, s.orc.k, N)
    budget = s.client.noise_budget(reply[0])
    print("N = %d, %d items: noise budget of the reply %.1f bits" % (N, dbsize, budget))
    assert budget > 0
    assert M.process_response_ct(s.client, s.params, index, reply) == s.item(index)


def test_d1_is_the_oracles_process_query():
    s = PirSetup(10, 0, 1, N=4096, plain_bits=24)
    q = s.client.create_query_for(s.params, 3)
    rc, want = s.orc.process_query(s.db_ntt, s.params.dimensions, q, s.galois_keys)
    rc2, got = M.process_query_ct(s.orc, s.db_ntt, s.params.dimensions, q, s.galois_keys, None)
    assert rc == rc2 == 0 and np.array_equal(got, want)
