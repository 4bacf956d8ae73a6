"""What the comments of the fp64 transforms claim (pir_amd/csrc/ntt_core.h, arith.h, device_params.h), checked on the model
of tests/f64_model.py at the rung moduli of tests/test_gpu_modulus_ladder.py with the structured inputs of
tests/test_gpu_extreme_values.py:

  forward, flavour 1     "|a| grows by at most 0.6 q per stage from < q (<= 9.4 q < 2^53 after 14 stages)"
  inverse, flavour 1     "|values| <= 16 q < 2^50, quotient estimates stay exact to < 0.1" per pass of 4 stages
  inverse, lazy          the sums of a whole transform "stay below 2^52" when bits(q) + log2 N <= 52
  inverse, flavour 2     "|values| <= 0.7 q throughout"
  packed intermediates   "|x| <= q" of what the inverse's last stage leaves (arith.h)

and what happens past the rules.  The model finds one bit of slack behind two of them, which the comments do not claim:
doubles hold integers up to 2^53, not 2^52, so the lazy inverse is still exact at bits + log2 N = 53 (it fails at 54),
and flavour 1 still works at 47 bits although its sums reach 2^51 there.  A cut-off moved by one bit towards the
narrow path would therefore not change a single residue -- which is why the ladder asserts the PATH each rung takes --
and the structured inputs are the ones that reach the bounds: a random input stays a factor two (sums of N terms of one
sign) to sqrt(N) (everything else) inside them.

Every model run is also compared with the CPU oracle's transform: the model computes the same function."""
import numpy as np
import pytest

import oracle
from f64_model import Field, Inexact
from gpu_helpers import structured_patterns


def field(N, bits):
    p, q = oracle.coeff_modulus_create(N, [bits, bits])          # q: the largest prime of that size, the one next to the bound
    orc = oracle.Oracle(N, [q, p], oracle.plain_modulus_batching(N, 20))
    return Field(q, N, orc.psi(0)), orc


def inputs(q, N, every):
    """The structured patterns (all of them, or the ones that attain the extremes at the rungs where all were run: a
    full set costs about 25 s at N = 16384) and one uniformly random input, last."""
    rng = np.random.default_rng(1)
    pats = structured_patterns(q, N, rng)
    if not every:
        top = N.bit_length() - 2
        keep = {"all q-1", "all q/2", "all q/2+1", "%d * delta_1" % (q - 1), "random top", "alternating 0 / q-1",
                "bit 3 set -> q-1", "bit 10 clear -> q-1", "bit %d set -> q-1" % top, "bit %d clear -> q-1" % top}
        pats = [p for p in pats if p[0] in keep]
        assert len(pats) == len(keep)
    return pats + [("random", rng.integers(0, q, size=N, dtype=np.uint64))]


#                  N     bits lazy   all patterns
FLAVOUR_1 = [(4096, 36, True, False), (4096, 40, True, True), (4096, 41, False, True), (2048, 41, True, True),
             (2048, 42, False, True), (16384, 38, True, False), (16384, 39, False, False), (8192, 45, False, False),
             (4096, 46, False, True), (16384, 46, False, False)]


@pytest.mark.parametrize("N,bits,lazy,every", FLAVOUR_1)
def test_flavour_1_stays_inside_its_comments(N, bits, lazy, every):
    assert lazy == (bits + N.bit_length() - 1 <= 52)          # the rule of ctx.hip
    F, orc = field(N, bits)
    logN = N.bit_length() - 1
    for name, v in inputs(F.q, N, every):
        out, st = F.forward(v, 1)
        assert np.array_equal(out, orc.ntt_fwd(0, v)), name
        growth = max(b - a for a, b in zip([1.0] + st.stage_max[:-1], st.stage_max))
        assert growth <= 0.6 and st.max_product <= 0.6, (name, growth, st.max_product)
        assert st.max_abs <= 1 + 0.6 * logN <= 9.4 and st.max_value < 2 ** 53, (name, st.max_abs)
        assert st.max_quotient_error < 0.1, (name, st.max_quotient_error)
        out, st = F.inverse(v, 1, lazy)
        assert np.array_equal(out, orc.ntt_inv(0, v)), name
        if lazy:
            assert st.max_value < 2 ** 52, (name, st.max_value)
        else:
            assert st.max_abs <= 16 and st.max_value < 2 ** 50, (name, st.max_abs)
        assert st.max_quotient_error < 0.1, (name, st.max_quotient_error)
        assert st.max_product <= 0.6 and st.last_product <= 1.0, (name, st.max_product)     # what gets packed: |x| <= q


@pytest.mark.parametrize("N,bits,every", [(4096, 47, True), (8192, 48, False), (8192, 49, False), (16384, 47, False)])
def test_flavour_2_stays_inside_its_comments(N, bits, every):
    F, orc = field(N, bits)
    logN = N.bit_length() - 1
    for name, v in inputs(F.q, N, every):
        out, st = F.forward(v, 2)
        assert np.array_equal(out, orc.ntt_fwd(0, v)), name
        growth = max(b - a for a, b in zip([1.0] + st.stage_max[:-1], st.stage_max))
        assert growth <= 0.6 and st.max_abs <= 1 + 0.6 * logN and st.max_value < 2 ** 53, (name, growth, st.max_abs)
        out, st = F.inverse(v, 2)
        assert np.array_equal(out, orc.ntt_inv(0, v)), name
        assert max(st.max_norm, st.max_product) <= 0.7 and st.last_product <= 1.0, (name, st.max_norm, st.max_product)
        assert st.max_abs <= 2.0, (name, st.max_abs)             # a sum of two kept values, before it is normalised
        assert st.max_quotient_error < 0.1, (name, st.max_quotient_error)


def test_the_structured_inputs_reach_the_lazy_bound_and_a_random_one_does_not():
    """bits + log2 N = 52: the all-(q - 1) vector drives a sum to N (q - 1), a factor 1 - 2^-22.8 below 2^52, and "index bit 11 set"
    takes a quotient estimate off by one -- the product leaves at 0.53 q instead of 0.5 q, still the right residue."""
    F, orc = field(4096, 40)
    pats = dict(inputs(F.q, 4096, False))
    _, st = F.inverse(pats["all q-1"], 1, True)
    assert st.max_value == 4096 * (F.q - 1) and 2 ** 52 * (1 - 2.0 ** -22) < st.max_value < 2 ** 52
    _, st = F.inverse(pats["bit 11 set -> q-1"], 1, True)
    assert st.wrong_quotients >= 1 and 0.53 < st.last_product < 0.54 and st.max_quotient_error > 0.03
    _, st = F.inverse(pats["random"], 1, True)
    assert st.max_value < 2 ** 51.01 and st.last_product < 0.51 and st.max_quotient_error < 0.005


def test_one_bit_past_the_lazy_rule_only_structured_inputs_leave_the_claimed_range():
    """41 bits at N = 4096 with the lazy form forced on (bits + log2 N = 53): the all-(q - 1) family reaches 2^53 -- twice
    the 2^52 the comment allows -- where a random input reaches 2^52.  The results are still exact (the slack the
    comment does not claim).  One more bit and "q - 1 - (small random)" is not: its sums pass 2^53 and are odd.  (The
    all-(q - 1) vector survives even that: its sums are (q - 1) 2^s, representable at any size.)"""
    F, orc = field(4096, 41)
    pats = dict(inputs(F.q, 4096, False))
    for name in ("all q-1", "random top"):
        out, st = F.inverse(pats[name], 1, True)
        assert 2 ** 52.99 < st.max_value < 2 ** 53, name
        assert np.array_equal(out, orc.ntt_inv(0, pats[name]))
    out, st = F.inverse(pats["random"], 1, True)
    assert st.max_value < 2 ** 52.01
    assert np.array_equal(out, orc.ntt_inv(0, pats["random"]))
    F, orc = field(4096, 42)
    pats = dict(inputs(F.q, 4096, False))
    with pytest.raises(Inexact):
        F.inverse(pats["random top"], 1, True)


def test_one_bit_past_the_flavour_1_cut_off_the_pass_sums_leave_the_claimed_range():
    """47 bits in flavour 1 (the rule hands them to flavour 2): the all-(q - 1) vector takes the sums of a pass to
    16 q = 2^51, past the "< 2^50" of the comment; a random input reaches about 11 q.  Quotient estimates and products keep
    their bounds and the residues are right: again one bit of slack."""
    F, orc = field(4096, 47)
    pats = dict(inputs(F.q, 4096, False))
    out, st = F.inverse(pats["all q-1"], 1)
    assert st.max_abs == 16 * (F.q - 1) / F.q and 2 ** 50 < st.max_value < 2 ** 51
    assert np.array_equal(out, orc.ntt_inv(0, pats["all q-1"]))
    out, st = F.inverse(pats["random"], 1)
    assert st.max_abs < 12 and st.max_quotient_error < 0.1 and st.last_product <= 1.0
    assert np.array_equal(out, orc.ntt_inv(0, pats["random"]))
