"""The packed-reply model (tests/reply_pack_model.py) against a naive per-bit restatement of DESIGN.md section 6.8."""
import numpy as np
import pytest

import reply_pack_model as rpm


def naive_pack_poly(x, w):
    """Bit b of coefficient i is stream bit i * w + b; stream bit s is bit s % 64 of word s // 64 -- in Python integers."""
    stream = 0
    for i, v in enumerate(int(v) for v in x):
        assert v >> w == 0
        for b in range(w):
            stream |= ((v >> b) & 1) << (i * w + b)
    n_words = len(x) * w // 64
    return np.array([(stream >> (64 * i)) & (2**64 - 1) for i in range(n_words)], dtype=np.uint64)


def naive_unpack_poly(words, N, w):
    stream = 0
    for i, v in enumerate(int(v) for v in words):
        stream |= v << (64 * i)
    return np.array([(stream >> (i * w)) & ((1 << w) - 1) for i in range(N)], dtype=np.uint64)


WIDTHS = [1, 2, 3, 30, 36, 37, 43, 49, 60, 61, 63, 64]


@pytest.mark.parametrize("w", WIDTHS)
def test_pack_poly_is_the_bit_stream(w):
    rng = np.random.default_rng(w)
    N = 128
    top = (1 << w) - 1
    for x in (rng.integers(0, top, size=N, dtype=np.uint64, endpoint=True),
              np.full(N, top, dtype=np.uint64),
              np.array([0, top] * (N // 2), dtype=np.uint64),
              np.array([0] * (N - 1) + [1], dtype=np.uint64)):
        got = rpm.pack_poly(x, w)
        assert got.shape == (N * w // 64,)
        assert np.array_equal(got, naive_pack_poly(x, w))
        assert np.array_equal(rpm.unpack_poly(got, N, w), x)
        assert np.array_equal(naive_unpack_poly(got, N, w), x)


def test_width_is_the_bit_length_of_q_minus_one():
    assert rpm.width(3) == 2 and rpm.width(5) == 3 and rpm.width(2**36 + 1) == 37 and rpm.width(2**36) == 36
    assert rpm.width(68719403009) == 36           # a 36-bit prime of the headline chain's size
    assert rpm.width((1 << 61) - 1) == 61


def test_ciphertext_layout_and_sizes():
    q = [1073479681, 68719403009, 1099511590913]    # 30, 36, 40 bits
    N = 64
    assert rpm.widths(q) == [30, 36, 40]
    assert rpm.ct_words(N, q) == 2 * (30 + 36 + 40)
    assert rpm.ct_words(N, q, 1) == 2 * 30
    assert rpm.ct_words(4096, [68719403009, 68719230977]) * 8 == 73728       # the headline reply: 8 x this = 589 824 B
    rng = np.random.default_rng(5)
    for r in (1, 2, 3):
        cts = np.stack([rng.integers(0, q[j], size=(3, 2, N), dtype=np.uint64) for j in range(r)], axis=2)
        p = rpm.pack(cts, q)
        assert p.shape == (3, rpm.ct_words(N, q, r))
        at = 0
        for c in range(2):        # the polynomials in the order (c, j)
            for j in range(r):
                pw = N * rpm.width(q[j]) // 64
                assert np.array_equal(p[1, at:at + pw], naive_pack_poly(cts[1, c, j], rpm.width(q[j])))
                at += pw
        assert np.array_equal(rpm.unpack(p, q, r, N), cts)


def test_extreme_residues_round_trip():
    q = [(1 << 61) - 1, 3, 2**36 + 1]     # widths 61, 2, 37 (the model does not need primes)
    N = 64
    cts = np.empty((2, 2, 3, N), dtype=np.uint64)
    for j, qj in enumerate(q):
        cts[0, :, j] = qj - 1
        cts[1, :, j] = np.array([0, qj - 1] * (N // 2), dtype=np.uint64)
    assert np.array_equal(rpm.unpack(rpm.pack(cts, q), q, 3, N), cts)


def test_unpack_rejects_a_coefficient_at_or_above_its_modulus():
    q = [5]           # width 3: 5, 6, 7 fit the width and are out of range
    N = 64
    x = np.zeros((2, 1, N), dtype=np.uint64)
    p = rpm.pack(x, q)
    p[..., 0] |= np.uint64(5 << 3)      # coefficient 1 of polynomial (0, 0) = 5
    with pytest.raises(ValueError):
        rpm.unpack(p, q, 1, N)
    with pytest.raises(AssertionError):
        rpm.pack(np.full((2, 1, N), 5, dtype=np.uint64), q)
