"""The CPU model of modulus-switched results (tests/modswitch_model.py) checked against itself and against the oracle:

  * the drop step on residues equals floor((x + floor(q_m/2)) / q_m) on the CRT integers, on random residues and on the
    boundary inputs the GPU test feeds the kernel;
  * with r = k (no step) the composed multiply is the oracle's own PIRDatabase::multiply -- the composition is right;
  * at the parameters of the GPU round trip the model recovers the item, with at least 2 bits of noise budget left on
    the switched reply (a condition on the choice of those parameters: the numbers are printed), and re-decoding the
    decrypted chunks reproduces the switched level-1 ciphertext exactly."""
import math

import numpy as np
import pytest

import modswitch_model as M
import oracle
from pir_fixtures import PirSetup

CHAINS = [
    (4096, [36, 36]),
    (4096, [60, 60]),
    (8192, [43, 43, 44]),
    (16384, [48, 48, 48, 49]),
    (32768, [49, 49]),
]


@pytest.mark.parametrize("N,bits", CHAINS)
def test_residue_step_equals_the_division_on_crt_integers(N, bits):
    q = [int(x) for x in oracle.coeff_modulus_create(N, bits)]
    k = len(q)
    rng = np.random.default_rng(k * N)
    cts = M.switch_inputs(q, 512, rng)[:, :, :, :]                 # (the step is per coefficient: 512 of them suffice)
    x = np.moveaxis(cts, -2, 0)                                    # [k, 4, 2, n]
    v = M.crt_compose(x, q)
    for r in range(1, k):
        got = np.moveaxis(M.switch_residues(cts, q, r), -2, 0)
        want = M.switch_crt(v, q, r)
        assert all(np.array_equal(got[i].astype(object), want % q[i]) for i in range(r)), (N, r)
    # the listed boundary values really do wrap: Q - 1 gives quotient Q / q_m = 0 mod the smaller modulus
    Q = math.prod(q)
    assert int(M.switch_crt(np.array([Q - 1], dtype=object), q, k - 1)[0]) == 0
    assert int(M.switch_crt(np.array([Q - q[-1] // 2 - 1], dtype=object), q, k - 1)[0]) == Q // q[-1] - 1


@pytest.fixture(scope="module")
def round_trip_setup():
    """The GPU round trip's parameters: N = 4096, [36, 36] + 37, 20-bit t, 10 x 10 plaintexts, r = 1."""
    s = PirSetup(100, 0, 2, N=4096, plain_bits=20)
    assert s.params.dimensions == [10, 10] and s.orc.k == 2
    return s


def test_no_step_is_the_oracles_multiply(round_trip_setup):
    s = round_trip_setup
    q = s.client.create_query_for(s.params, 37)
    rc, want = s.orc.process_query(s.db_ntt, s.params.dimensions, q, s.galois_keys)
    assert rc == 0
    assert np.array_equal(M.process_query_switched(s.orc, s.db_ntt, s.params.dimensions, q, s.galois_keys, s.orc.k), want)
    assert M.expansion_ratio_level(s.orc, s.orc.k) == s.orc.expansion_ratio()


def test_model_recovers_the_item_with_noise_to_spare(round_trip_setup):
    s = round_trip_setup
    p = s.params
    index = 98                                                     # plaintext num_pt - 2
    q = s.client.create_query_for(p, index)
    rc, sv = s.orc.oblivious_expansion_multi(q, p.dim_sum, s.galois_keys)
    assert rc == 0
    trace = []
    reply = M.multiply_switched(s.orc, s.db_ntt, p.dimensions, sv, 1, trace=trace)
    assert reply.shape == (4, 2, 1, 4096)
    rc, full = s.orc.db_multiply(s.db_ntt, p.dimensions, sv.copy())
    budgets = [M.noise_budget_level(s.client, c, 1) for c in reply]
    print("reply noise budget, full modulus: %.1f bits; switched to 1 prime: %.1f bits"
          % (min(s.client.noise_budget(c) for c in full), min(budgets)))
    assert min(budgets) >= 2
    pt = M.process_reply_level(s.client, 2, reply, 1)
    rc, data = oracle.string_decode(pt, p.eff_bits_per_coeff, p.bytes_per_item,
                                    oracle.calculate_item_offset(index, p.items_per_plaintext, p.bytes_per_item))
    assert rc == 0 and data == s.item(index)
    # the client's re-decode of the decrypted chunks is the switched level-1 ciphertext of the selected row, exactly
    row = trace[0][index // 10][0]
    assert np.array_equal(M.redecode_level(s.orc, [M.decrypt_level(s.client, c, 1) for c in reply], 1), row)
    assert np.array_equal(M.reencode_level(s.orc, row, 1), np.stack([M.decrypt_level(s.client, c, 1) for c in reply]))
