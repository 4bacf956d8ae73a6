"""What the comments of the scan's fold claim (pir_amd/csrc/scan_mfma.hip: `kBiasBits`, the F64F paragraph), asserted on
the model of tests/scan_fold_model.py at the operands that reach the bounds.

For every kernel variant launch_scan_mfma_groups instantiates -- (L, KS, NW) x top-digit form x fold; the arithmetic
depends on NW only through KS -- and for the smallest and the largest NTT-friendly prime (N = 4096: == 1 mod 8192) of
every bit size the digit count serves, the sign-coherent family is searched: both operands with low digits all -128 or
all +127 and the top digit at either end of what the centring leaves, in all 64 KS columns of a chunk.  Asserted:

  int32 diagonals    sum of |terms| <= (L - 1) 2^14 * 64 KS < 2^25.2 (so no order of accumulation leaves int32)
  integer fold       |group| < 2^57.2; 0 < group + bias < 2^59.4 without int64 overflow; reduce128's input < 2^99.5;
                     the residue is cols * x_db * x_sel mod q
  fp64 fold          every double is the integer it stands for (f64_model.Inexact otherwise); |C| < 2^49.01; the sum of
                     the chunks' residues < 2^53; quotient estimates off by < 0.1; the same residue

What the model found: with the bias one bit lower (2^57 <= bias < 2^58, as the fold was first written) group 0 of SIX
digits over SEVEN k-steps reaches -2^57.13 and `group + bias` goes negative for the smallest prime of every size from
41 to 47 bits (40 in the nibble form) -- any q < 1.097 * 2^(bits - 1) -- in both top-digit forms; from 412 columns on at
47 bits.  No other variant and no largest prime is affected (L = 7 over 6 k-steps stays at 2^56.92, L = 5 at 2^56.81), and the fp64 fold
is inside its bounds everywhere.  test_the_lower_bias_fails_exactly_there pins that map."""
import math

import numpy as np
import pytest

import oracle
import scan_fold_model as M
from gpu_helpers import smallest_primes
from test_scan_digit_model import to_digits_top4, vmax

N = 4096
MAX_BITS = {5: 39, 6: 47, 7: 55}                       # mfma_geometry: L digits up to that many bits of the data moduli
# launch_scan_mfma_groups: 8-wave kernels of 1..3 (L = 7: 1..2) k-steps, 4-wave kernels of 3..7 (L = 7: 3..6)
DISPATCH = [(5, 1, 8), (5, 2, 8), (5, 3, 8), (6, 1, 8), (6, 2, 8), (6, 3, 8), (7, 1, 8), (7, 2, 8),
            (5, 3, 4), (5, 4, 4), (5, 5, 4), (5, 6, 4), (5, 7, 4), (6, 3, 4), (6, 4, 4), (6, 5, 4), (6, 6, 4), (6, 7, 4),
            (7, 3, 4), (7, 4, 4), (7, 5, 4), (7, 6, 4)]
log2 = lambda v: math.log2(v) if v else float("-inf")


def primes_of(bits):
    """(smallest, largest) NTT-friendly prime of that size, or None where the size has fewer than two."""
    try:
        lo = smallest_primes(N, bits, 1)[0]
        hi = oracle.coeff_modulus_create(N, [bits])[0]
    except ValueError:
        return None
    return (lo, hi) if lo != hi else None


def sizes(L):
    out = [(b, primes_of(b)) for b in range(14, MAX_BITS[L] + 1)]
    return [(b, p) for b, p in out if p]


def ksteps(L):
    return sorted({ks for l, ks, _ in DISPATCH if l == L})


def forms(L, bits):
    """Top-digit forms instantiated for L that a modulus of that size can take (nibble: L <= 6, bits <= 8 (L - 1) + 4)."""
    return ([True] if L <= 6 and bits <= 8 * (L - 1) + 4 else []) + [False]


def pair_products(q, L, top4):
    """[(db name, sel name, x_db, x_sel, P[s], A[s])] over the family: the diagonals of ONE column and their sums of |terms|."""
    fam = M.family(q, L, top4)
    out = []
    for na, va in fam:
        for nb, vb in fam:
            da, db = M.to_digits(va % q, q, L, top4)[0], M.to_digits(vb % q, q, L, top4)[0]
            P, _ = M.diagonals([da], [db])
            A = [sum(abs(da[a] * db[s - a]) for a in range(L) if 0 <= s - a < L) for s in range(2 * L - 1)]
            out.append((na, nb, va, vb, P, A))
    return out


def test_the_dispatch_table_and_the_bias_are_the_ones_modelled():
    assert M.variants_in_source() == DISPATCH
    assert M.bias_bits_in_source() == 59
    for L in (5, 6, 7):
        assert M.top4_vmax(L) == vmax(L)


def test_the_model_computes_the_function():
    """Digits reconstruct the residue in both centrings, reduce128 reduces any 128-bit value, and both folds return
    sum_s T[s] 2^(8 s) mod q on the diagonals of random operands."""
    rng = np.random.default_rng(5)
    for L, bits, top4 in [(5, 36, True), (5, 39, False), (6, 44, True), (6, 47, False), (7, 50, False), (7, 55, False)]:
        for q in primes_of(bits):
            xs = [int(v) for v in rng.integers(0, q, size=300)] + [0, 1, q - 1, q >> 1, (q >> 1) + 1, vmax(L) % q, (vmax(L) + 1) % q]
            for x in xs:
                d, lost = M.to_digits(x, q, L, top4)
                assert lost == 0 and all(-128 <= b <= 127 for b in d) and (not top4 or -8 <= d[-1] <= 7), (x, q, d)
                assert (sum(b * 256 ** a for a, b in enumerate(d)) - x) % q == 0
            if top4:
                ref = to_digits_top4(np.array(xs, dtype=np.uint64), q, L)
                assert [[int(ref[a][i]) for a in range(L)] for i in range(len(xs))] == [M.to_digits(x, q, L, True)[0] for x in xs]
            for _ in range(200):
                v = int(rng.integers(0, 1 << 62)) << 66 | int(rng.integers(0, 1 << 62)) << 4 | int(rng.integers(0, 16))
                assert M.reduce128(v & M.M64, v >> 64, q) == v % q
            cols = 100
            A = [M.to_digits(int(v), q, L, top4)[0] for v in rng.integers(0, q, size=cols)]
            B = [M.to_digits(int(v), q, L, top4)[0] for v in rng.integers(0, q, size=cols)]
            T, _ = M.diagonals(A, B)
            want = sum(t << (8 * s) for s, t in enumerate(T)) % q
            assert M.int_fold(T, q, 59)[0] == want
            if q < 2 ** 50:
                assert M.f64_fold(np.array(T, dtype=object).reshape(-1, 1), q)[0] == [want]


@pytest.mark.parametrize("L", [5, 6, 7])
def test_every_variant_stays_inside_its_types_and_comments(L):
    bias_bits = M.bias_bits_in_source()
    worst = dict(T=0, group=0, biased=0, v=0, chunk=0.0, acc=0.0, qerr=0.0)
    for bits, pair in sizes(L):
        for q in pair:
            for top4 in forms(L, bits):
                prods = pair_products(q, L, top4)
                for KS in ksteps(L):
                    cols = 64 * KS
                    where = (L, KS, top4, bits, hex(q))
                    Ts = []
                    for na, nb, va, vb, P, A in prods:
                        T = [cols * p for p in P]
                        Ts.append(T)
                        bound = cols * max(A)
                        assert bound <= (L - 1) * 2 ** 14 * cols < 2 ** 25.2 and bound < 2 ** 31, (where, na, nb)
                        worst["T"] = max(worst["T"], bound)
                        r, st = M.int_fold(T, q, bias_bits)
                        assert not st.int64_overflow, (where, na, nb)
                        assert st.max_group < 2 ** 57.2, (where, na, nb, log2(st.max_group))
                        assert 0 < st.min_biased, ("group + bias is negative: the cast wraps", where, na, nb, st.min_biased)
                        assert r == cols * va * vb % q, (where, na, nb)
                        assert 2 ** (bias_bits - 1) <= q << (bias_bits - bits) < 2 ** bias_bits, where
                        assert st.max_v < 2 ** 99.5, (where, log2(st.max_v))
                        worst["group"] = max(worst["group"], st.max_group)
                        worst["biased"] = max(worst["biased"], st.max_biased)
                        worst["v"] = max(worst["v"], st.max_v)
                    if q < 2 ** 50:                         # ctx.hip: the fp64 fold needs every data modulus below 2^50
                        r, st = M.f64_fold(np.array(Ts, dtype=object).T, q)
                        assert r == [cols * va * vb % q for _, _, va, vb, _, _ in prods], where
                        assert st.max_chunk < 2 ** 49.01 and st.max_acc < 2 ** 53 and st.max_value < 2 ** 53, (where, st.max_chunk)
                        assert st.max_quotient_error < 0.1 and st.wrong_quotients == 0, (where, st.max_quotient_error)
                        assert st.max_product <= 0.6 and st.max_norm <= 0.5, (where, st.max_product, st.max_norm)
                        worst["chunk"] = max(worst["chunk"], st.max_chunk)
                        worst["acc"] = max(worst["acc"], st.max_acc)
                        worst["qerr"] = max(worst["qerr"], st.max_quotient_error)
    print("L = %d:" % L, {k: round(log2(v), 3) if k != "qerr" else v for k, v in worst.items()})
    # the bounds are reached, not merely respected: the widest variant sits on them
    KS = max(ksteps(L))
    assert worst["T"] == (L - 1) * 2 ** 14 * 64 * KS
    assert worst["biased"] < 2 ** 59.4
    assert log2(worst["group"]) > {5: 56.8, 6: 57.13, 7: 56.9}[L]
    assert log2(worst["chunk"]) > 48.5


def lower_bias_failures(L):
    """{(KS, top4, bits, 'smallest' | 'largest')} where the fold with 2^57 <= bias < 2^58 returns a wrong residue."""
    bad = set()
    for bits, pair in sizes(L):
        for which, q in zip(("smallest", "largest"), pair):
            for top4 in forms(L, bits):
                for na, nb, va, vb, P, A in pair_products(q, L, top4):
                    for KS in ksteps(L):
                        cols = 64 * KS
                        r, st = M.int_fold([cols * p for p in P], q, 58)
                        if r != cols * va * vb % q:
                            assert st.min_biased < 0           # the only way it goes wrong
                            bad.add((KS, top4, bits, which))
                        else:
                            assert st.min_biased >= 0
    return bad


def test_the_lower_bias_fails_exactly_there():
    assert lower_bias_failures(5) == set() and lower_bias_failures(7) == set()
    # from 41 bits on the five low digits of both operands are free, and diagonal 4 -- the top of group 0 -- holds five
    # products of -128 * 127
    want = {(7, top4, bits, "smallest") for bits in range(41, 48) for top4 in forms(6, bits)}
    # ... and at 40 bits in the nibble form, which leaves so small a residue uncentred (q - 1 <= vmax): digit 4 then
    # takes the whole byte range
    want.add((7, True, 40, "smallest"))
    assert lower_bias_failures(6) == want and (7, True, 44, "smallest") in want and (7, False, 47, "smallest") in want
    # 47 bits, q = 0x400000008001: 411 columns of (-128 .., +127 ..) are still folded right, 412 are not
    q = smallest_primes(N, 47, 1)[0]
    assert q == 0x400000008001
    fam = dict(M.family(q, 6, False))
    va = next(v for n, v in fam.items() if n.startswith("low -128"))
    vb = next(v for n, v in fam.items() if n.startswith("low 127"))
    da, db = M.to_digits(va % q, q, 6, False)[0], M.to_digits(vb % q, q, 6, False)[0]
    for cols, ok in ((410, True), (411, True), (412, False), (416, False), (448, False)):
        T, _ = M.diagonals([da] * cols, [db] * cols)
        assert (M.int_fold(T, q, 58)[0] == cols * va * vb % q) == ok, cols
        assert M.int_fold(T, q, 59)[0] == cols * va * vb % q


# ---------------------------------------------------------------- AccLimb / AccWide (kernels.hip)

def test_limb_accumulators_hold_their_interval_at_the_largest_limbs():
    """AccLimb's comment: exact for kLimbLazy = 128 terms of a modulus below 2^50 -- s00 < 128 * 2^56 + q (the sum is
    carried as a residue from one interval to the next), s01 < 128 * 2^51, s11 < 128 * 2^44 -- at the residue whose two
    28-bit limbs are both largest and at q - 1, on both sides, in every term; the interval could not be doubled."""
    lazy = M.limb_lazy_in_source()
    assert lazy == 128
    for bits in (36, 49, 50):
        for q in primes_of(bits):
            assert q < 2 ** 50
            for a in (q - 1, M.limb_max(q)):
                for b in (q - 1, M.limb_max(q)):
                    for n in (lazy - 1, lazy, lazy + 1, 3 * lazy + 1):
                        acc = M.AccLimb(q)
                        assert M.lazy_scan(acc, [(a, b)] * n, lazy) == n * a * b % q, (q, a, b, n)
                        assert not acc.wrapped
                        assert acc.max[0] < lazy * 2 ** 56 + q and acc.max[1] < lazy * 2 ** 51 and acc.max[2] < lazy * 2 ** 44
            a, n = M.limb_max(q), 2 * lazy + 2
            acc = M.AccLimb(q)
            assert M.lazy_scan(acc, [(a, a)] * n, n) != n * a * a % q and acc.wrapped          # no fold in between
    q = primes_of(50)[1]
    acc = M.AccLimb(q)
    M.lazy_scan(acc, [(M.limb_max(q), M.limb_max(q))] * (2 * lazy), lazy)
    assert acc.max[0] > lazy * 2 ** 56 - 2 ** 37                     # the bound of s00 is reached to within 2^-26


def test_wide_accumulators_hold_lazy_limit_terms_of_q_minus_one():
    """AccWide: `lazy_limit` = 2^(128 - 2 bits) products of residues of a `bits`-bit modulus fit 128 bits together with
    the carried residue; one interval more does not at 61 bits (64 terms of (q - 1)^2 are 2^128 - ...)."""
    assert [M.lazy_limit(b) for b in (48, 49, 50, 55, 60, 61)] == [1 << 30, 1 << 30, 1 << 28, 1 << 18, 1 << 8, 1 << 6]
    for bits in (60, 61):
        lazy = M.lazy_limit(bits)
        for q in primes_of(bits):
            for n in (lazy - 1, lazy, lazy + 1, 2 * lazy + 1):
                acc = M.AccWide(q)
                assert M.lazy_scan(acc, [(q - 1, q - 1)] * n, lazy) == n * (q - 1) ** 2 % q
                assert not acc.wrapped
        q = primes_of(bits)[1]                                         # the largest prime: 2 lazy_limit terms wrap
        acc = M.AccWide(q)
        M.lazy_scan(acc, [(q - 1, q - 1)] * (2 * lazy), 2 * lazy)
        assert acc.wrapped
    # larger intervals cannot be run term by term; the bound is lazy_limit * (q - 1)^2 + q < 2^128 for every size
    for bits in range(14, 62):
        assert M.lazy_limit(bits) * (2 ** bits - 2) ** 2 + 2 ** bits < 2 ** 128
