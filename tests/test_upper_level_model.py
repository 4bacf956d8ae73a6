"""The accumulators of the upper recursion level on the CPU model of tests/upper_level_model.py, at the operands
tests/test_gpu_upper_worst_case.py sends through the kernels.

fp64 (upper_fused_kernel's comment "|term| <= 0.7 q, renormalised every 8 terms"; upper_mac_kernel's sums carried as
doubles from block to block): a pseudo-random chunk, its transform x as the kernel holds it, and the selector
w = r0 x^-1 with r0 = 0.45 q, so that every child adds the same residue in every slot.  At the largest and the smallest
NTT-friendly primes of 46 bits (flavour 1) and of 47 and 49 bits (flavour 2): no term above 0.7 q, every sum the exact
integer, and the running sum reaches 8 x 0.45 q = 3.6 q -- the eight coherent terms between two normalisations, against
the random walk of random selectors (0.8 q rms; 2.9 q in the worst of 4096 slots, never in all of them).  The largest
double kept is 3.8 q < 2^51 at 49 bits: the comment's bound holds with two bits to spare, nothing to correct.

integer (128-bit sums folded every lazy_limit children): children x = q - (t - 2^b + 1), selectors q - 1.  The folded
schedule gives n x w mod q just below, at and above the interval and past two of them; without the fold, or with the fold
one child late, the residue is a different one for every n above the interval: the operands tell the schedules apart."""
import numpy as np
import pytest

import oracle
import upper_level_model as U
from f64_model import Field, floats
from gpu_helpers import chain, chain_low

N = 4096
T_BITS = 20


def fp64_operands(N, bits, low_end, seed=5):
    """(Field, x of chunk 0 as the kernel holds it, the coherent selector, r0) for one pseudo-random ciphertext."""
    moduli = (chain_low if low_end else chain)(N, [bits])
    q = int(moduli[0])
    t = oracle.plain_modulus_batching(N, T_BITS)
    orc = oracle.Oracle(N, moduli, t)
    F = Field(q, N, orc.psi(0))
    b = t.bit_length() - 1
    assert b <= 31 and t < q                                    # the kernels' fast lift: chunk -> signed double
    mode = 1 if bits <= 46 else 2
    rng = np.random.default_rng(seed + bits)
    chunk = rng.integers(0, 1 << b, size=N)
    lifted = [U.lift(int(v), t) for v in chunk]
    x, st = F.forward(lifted, mode, canonical=False)
    assert st.max_norm <= 0.5 + 1e-9
    # the model computes the oracle's transform of the lifted plaintext
    want = orc.ntt_fwd(0, np.array([v % q for v in lifted], dtype=np.uint64))
    assert [int(v) % q for v in x.tolist()] == [int(v) for v in want]
    r0 = U.target(q)
    return F, x, U.coherent_selector(F, x, r0), r0


# (bits, smallest prime of the size)
FP64 = [(46, False), (46, True), (47, False), (47, True), (49, False), (49, True)]


@pytest.mark.parametrize("bits,low_end", FP64)
@pytest.mark.parametrize("blocks", [[25], [10, 10, 5], [5] * 5, [9, 8], [8], [9], [24]], ids=lambda b: "+".join(map(str, b)))
def test_fp64_sums_of_coherent_terms_stay_exact(bits, low_end, blocks):
    F, x, w, r0 = fp64_operands(N, bits, low_end)
    n = sum(blocks)
    for target, sign in ((r0, 1), (F.q - r0, -1)):
        ws = w if sign > 0 else floats(np.array([(F.q - int(v)) % F.q for v in w.tolist()], dtype=object))
        out, st = U.fp64_schedule(F, [x] * n, [ws] * n, blocks)            # raises Inexact if a double is not its integer
        assert set(out) == {n * target % F.q}
        print("%d bits %s prime, blocks %s, target %+d: max |term| %.3f q, max |sum| %.3f q = 2^%.2f, %d of %d terms "
              "changed sign, quotient estimates off by at most %.3f" % (
                  bits, "smallest" if low_end else "largest", blocks, sign, st.max_term, st.max_acc,
                  np.log2(st.max_acc_value), st.flipped, n * N, st.max_quotient_error))
        assert st.max_term <= 0.7
        assert st.max_acc_value < 2 ** 53
        # 8 x 0.45 q: eight coherent terms between two normalisations (a block shorter than eight children ends first and
        # the count restarts: such a split reaches its own length and the carry, 5 x 0.45 q + 0.25 q)
        assert st.max_acc >= (3.6 if max(blocks) >= 8 else 0.45 * max(blocks))
        assert st.max_acc <= 8 * 0.7 + 0.5 + 1e-9                           # what the comment implies: 8 terms + a carry


def test_random_selectors_stay_below_the_coherent_sum():
    """The same children with uniformly random selectors, what every other GPU test of the upper level sees: eight terms
    uniform in (-q / 2, q / 2) add to 0.82 q rms, and 3.6 q is 4.4 standard deviations -- not reached in any of the 4096
    slots, where the coherent selectors reach it in every one."""
    F, x, _, _ = fp64_operands(N, 49, False)
    rng = np.random.default_rng(9)
    ws = [floats(np.array([int(v) for v in rng.integers(0, F.q, size=N)], dtype=object)) for _ in range(8)]
    out, st = U.fp64_schedule(F, [x] * 8, ws, [8])
    X = [int(v) % F.q for v in x.tolist()]
    assert out == [sum(X[s] * int(w[s]) for w in ws) % F.q for s in range(N)]
    print("random selectors: max |sum| %.3f q" % st.max_acc)
    assert st.max_acc < 3.6


def int_operands(N, bits):
    q = int(chain(N, [bits])[0])
    t = oracle.plain_modulus_batching(N, T_BITS)
    b = t.bit_length() - 1
    x = U.lift((1 << b) - 1, t, q)
    assert x == q - (t - (1 << b) + 1)
    return q, x, q - 1, U.lazy_limit(q)


@pytest.mark.parametrize("N,bits,limit", [(4096, 61, 64), (2048, 60, 256), (32768, 61, 64)])
def test_integer_fold_around_its_interval(N, bits, limit):
    q, x, w, lim = int_operands(N, bits)
    assert lim == limit
    assert limit * x * w + q < 2 ** 128 <= (limit + 1) * x * w            # one interval fits, one more child does not
    for n in (limit - 1, limit, limit + 1, 2 * limit + 2):
        want = n * x * w % q
        shapes = [[n]] + ([[limit - 1] * (n // (limit - 1)) + [n % (limit - 1)]] if n > limit else [])
        for blocks in shapes:                                              # one launch; blocks shorter than the interval
            assert U.int_schedule(q, [x] * n, [w] * n, limit, blocks) == want, (n, blocks)
        for variant in ("no fold", "late"):
            got = U.int_schedule(q, [x] * n, [w] * n, limit, [n], variant)
            assert (got == want) == (n <= limit), (n, variant)


def test_chunk_layout_and_all_ones_value():
    q = int(chain(4096, [61])[0])
    assert U.chunk_layout([q], 19) == [(p, 0, s) for p in (0, 1) for s in (0, 19, 38, 57)]
    v = U.all_ones_value(q, 19)
    assert v < q and [(v >> s) & (2 ** 19 - 1) for s in (0, 19, 38)] == [2 ** 19 - 1] * 3 and v >> 57 == (q >> 57) - 1
