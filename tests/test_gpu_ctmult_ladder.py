"""The hooks of the ciphertext-multiplication mode at every k = 1 ... 6, every transform flavour,
every key-switch width and the ring degrees 2048 ... 16384, each rung bit for bit against the big-integer definition of
tests/ctmult_model.py: pirgpu_ct_multiply on the hook_inputs family (random pairs, q_j - 1 everywhere, the centring
boundary, the magnitude bound N h^2, the three remainders around the rounding step -- check_hook_inputs asserts they are
reached) against scaled_residues(tensor(...)), then pirgpu_relinearize on the results with a random key against
M.relinearize.  The chains are M.LADDER (the same chains go through the RNS restatement on the CPU in
tests/test_ctmult_model.py and through the plan in tests/test_ctmult_host.py):

  id        N      data primes     t    what the rung is there for
  k1        2048   [54]            20   K = 1, three auxiliary primes, the integer flavour chosen by the moduli, N = 2048
  k2-tight  4096   [30, 30]        46   t > q_j (t_q, t_b reduce t); the largest batching t the plan accepts: both bounds
                                        within a factor 8 of failing (test_ctmult_host.py)
  k3-mixed  4096   [30, 36, 40]    20   K = 3; 40-bit auxiliary primes, 40-bit Garner digits reduced into a 30-bit modulus
  k3-wide   4096   [47] x 3        20   the wide fp64 flavour at Q and at B
  k3-pack7  8192   [48] x 3        20   7 packed bytes in the key switch of the relinearisation
  k5        4096   [41] x 5        20   K = 5, seven auxiliary primes, exact fp64 without the lazy inverse, 6 packed bytes
  k6-f64    4096   [40] x 6        20   K = 6, eight auxiliary primes through the fp64 ntt_batch with the lazy inverse
  k6-int    4096   [60] x 6        59   K = 6 at SEAL's largest primes, u64 key-switch words
  n16384    16384  [46, 46]        20   the 14-stage transform at the auxiliary base

Every rung asserts the path it expects to have run -- flavour, lazy inverse, packed width, length and size of the auxiliary
base -- literally, not recomputed from the rules: a changed rule shows up as a failing expectation.  The rungs with k >= 5
or N = 16384 run M.SUB_FAMILY (one random pair, q_j - 1, full h, full h + 1 and the three remainders), the others the
whole family.  The last test is one whole d = 2 reply at K = 3 (selectors, lift indexing and accumulate off the default
chain) against process_query_ct."""
import ctypes as C

import numpy as np
import pytest

import ctmult_model as M
import oracle
import pir_amd
from gpu_helpers import chain, random_key, to_product_params
from pir_amd import parameters as P
from pir_fixtures import PirSetup

pytestmark = pytest.mark.gpu

#      id          flavour  lazy inverse  packed bytes  auxiliary primes  sub-family
PATHS = {
    "k1":        (0, False, 8, 3, False),
    "k2-tight":  (1, True, 5, 4, False),
    "k3-mixed":  (1, True, 6, 5, False),
    "k3-wide":   (2, False, 6, 5, False),
    "k3-pack7":  (2, False, 7, 5, False),
    "k5":        (1, False, 6, 7, True),
    "k6-f64":    (1, True, 6, 8, True),
    "k6-int":    (0, False, 8, 8, True),
    "n16384":    (1, False, 6, 4, True),
}
assert list(PATHS) == [c[0] for c in M.LADDER]

_CASE = {}


def ladder_case(rung):
    """moduli, t, inputs, exact products, key and relinearised products of one rung, computed once."""
    if rung not in _CASE:
        _, N, bits, t_bits = next(c for c in M.LADDER if c[0] == rung)
        moduli = [int(x) for x in chain(N, bits)]
        assert [x.bit_length() for x in moduli] == bits + [max(bits)]
        t = oracle.plain_modulus_batching(N, t_bits)
        assert t.bit_length() == t_bits
        orc = oracle.Oracle(N, moduli, t)
        q = moduli[:-1]
        rng = np.random.default_rng(N + len(q))
        names, A, B = M.hook_inputs(q, t, N, rng, names=M.SUB_FAMILY if PATHS[rung][4] else None)
        xs = [M.tensor(A[i], B[i], q) for i in range(len(names))]
        M.check_hook_inputs(names, xs, q, t)       # the remainders and the magnitude bound are really reached
        want = np.stack([M.scaled_residues(x, q, t) for x in xs])
        rk = random_key(orc, rng)
        relin = np.stack([M.relinearize(orc, want[i], rk) for i in range(len(names))])
        _CASE[rung] = (N, moduli, t, names, A, B, want, rk, relin)
    return _CASE[rung]


@pytest.mark.parametrize("rung", list(PATHS))
def test_rung(rung):
    mode, lazy, pack, n_aux, sub = PATHS[rung]
    N, moduli, t, names, A, B, want, rk, relin = ladder_case(rung)
    assert len(names) == (len(M.SUB_FAMILY) if sub else 11)
    k = len(moduli) - 1
    enc = P.EncryptionParams(N, moduli, t)
    pp = P.create_pir_parameters(4, 0, 1, enc, True)
    db = pir_amd.PIRDatabase.Create(pp, ct_multiplication=True)
    srv = pir_amd.PIRServer(db, pp)
    # the path: flavour, lazy inverse and packed width of the context, the auxiliary base the library planned
    a = srv.arith_info()
    assert db.lib.pirgpu_ntt_mode(db.handle) == mode and a["ntt_mode"] == mode, a
    assert a["f64_lazy_inv"] == lazy and a["pack_bytes"] == pack, a
    qa, aux, n = (C.c_uint64 * k)(*moduli[:k]), (C.c_uint64 * 16)(), C.c_uint32(0)
    assert db.lib.pirgpu_ctmult_plan(N, k, qa, moduli[k], t, aux, C.byref(n)) == 0
    assert n.value == n_aux == k + 2
    assert all(int(aux[i]).bit_length() == max(x.bit_length() for x in moduli[:k]) for i in range(n_aux))
    got = db.ct_multiply(A, B)
    for i, name in enumerate(names):
        bad = np.argwhere(got[i] != want[i])
        assert bad.size == 0, "%s: first mismatch at [component, residue, coefficient] = %s" % (name, bad[:1].tolist())
    srv.set_relin_key(rk)
    out = db.relinearize(got)
    for i, name in enumerate(names):
        assert np.array_equal(out[i], relin[i]), name
    db.close()


def test_whole_reply_at_three_mixed_primes():
    """d = 2, 9 items in 3 x 3 on [30, 36, 40] at N = 4096: the query path -- selectors back in coefficient form, the
    lift's indexing of children and selectors, accumulate -- at K = 3, bits against process_query_ct."""
    N = 4096
    s = PirSetup(9, 0, 2, N=N, plain_bits=20, moduli=[int(x) for x in chain(N, [30, 36, 40])])
    assert s.params.dimensions == [3, 3] and s.orc.k == 3
    rk = M.relin_key(s.client)
    pp = to_product_params(s.params)
    pp.use_ciphertext_multiplication = True
    db = pir_amd.PIRDatabase.Create(pp, ct_multiplication=True)
    db.populate(s.raw)
    srv = pir_amd.PIRServer(db, pp)
    srv.set_galois_keys(s.galois_keys)
    srv.set_relin_key(rk)
    assert srv.ntt_mode() == 1 and srv.arith_info()["pack_bytes"] == 6
    q = s.client.create_query_for(s.params, 5)
    rc, want = M.process_query_ct(s.orc, s.db_ntt, s.params.dimensions, q, s.galois_keys, rk)
    assert rc == 0
    got = srv.process_query(q)
    assert got.shape == want.shape == (1, 2, 3, N)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "first mismatch at [ct, poly, residue, coefficient] = %s" % bad[:1].tolist()
    assert db.get_option("ct_blocks") == 1
    db.close()
