"""The compact-query model (tests/query_compact_model.py) against its parts: layout and sizes in
Python integers, unpacking through tests/reply_pack_model.py, c1 through tests/seal_wire.py's sampler over the data
moduli.  The host's range check rpk::check_poly (pir_amd/csrc/reply_pack.h) is restated here step for step and compared
with unpack_poly; the C++ itself runs in tests/cpp/query_compact_test.cpp.

Widths: 36, 37, 49 and 60 bits.  A width of 64 needs a modulus above 2^63, which no chain allows (SEAL bounds a
coefficient modulus by 61 bits, the sampler by 2^63): the plain form is what stands for "64 bits a coefficient"."""
import numpy as np
import pytest

import oracle
import query_compact_model as M
import reply_pack_model as rpm
import seal_wire as W
from gpu_helpers import chain

N = 2048
SEED = bytes(range(64))


def _prime(bits):
    return int(oracle.coeff_modulus_create(N, [bits])[0])


def check_poly(words, N, w, q):
    """rpk::check_poly restated: streams like unpack_poly, stores nothing."""
    mask = (1 << w) - 1
    acc = have = 0
    bad = False
    it = iter(int(v) for v in words)
    for _ in range(N):
        if have >= w:
            v = acc & mask
            acc >>= w
            have -= w
        else:
            nxt = next(it)
            v = (acc | (nxt << have)) & mask
            took = w - have
            acc = nxt >> took
            have = 64 - took
        bad |= v >= q
    return not bad


def test_headline_sizes():
    q = [int(v) for v in oracle.BFV_DEFAULT[4096][:2]]
    assert [rpm.width(v) for v in q] == [36, 36]
    assert M.words(4096, q, False) == 2 * 4096 + 8
    assert M.words(4096, q, True) == 2 * 4096 * 36 // 64 + 8
    assert M.wire_bytes(4096, q, True) == 2 * 4096 * 36 // 8 + 64 == 36928
    assert 2 * 2 * 4096 * 8 == 131072                         # the expanded ciphertext the issue starts from
    assert 131072 / 36928 > 3.5


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("bits", [[36], [36, 37], [49, 60, 36]], ids=lambda b: "-".join(map(str, b)))
def test_layout_round_trip_and_expansion(bits, packed):
    q = [_prime(b) for b in bits]
    rng = np.random.default_rng(sum(bits))
    c0 = np.stack([rng.integers(0, v, N, dtype=np.uint64) for v in q])
    c0[:, 0] = [v - 1 for v in q]                             # the largest residue, first and last
    c0[:, -1] = [v - 1 for v in q]
    obj = M.compact(c0, SEED, q, packed)
    assert obj.shape == (sum(N * (b if packed else 64) // 64 for b in bits) + 8,)
    back, seed = M.split(obj, N, q, packed)
    assert np.array_equal(back, c0) and seed == SEED
    assert M.check(obj, N, q, packed)
    ct = M.expand(obj, N, q, packed)
    assert ct.shape == (2, len(q), N) and np.array_equal(ct[0], c0)
    assert np.array_equal(ct[1], W.sample_poly_uniform(SEED, q, N))
    # the walk over the data moduli is a prefix of the key-level walk
    special = int(oracle.coeff_modulus_create(N, [max(bits)])[0])
    assert np.array_equal(ct[1], W.sample_poly_uniform(SEED, q + [special], N)[:len(q)])
    if not packed:
        assert np.array_equal(obj[:-8], c0.reshape(-1))       # plain: the words themselves


@pytest.mark.parametrize("bits", [36, 37, 49, 60])
def test_check_poly_against_unpack_poly(bits):
    q = _prime(bits)
    w = rpm.width(q)
    assert w == bits
    # a coefficient that straddles two words: the first i with (i w) % 64 + w > 64
    straddle = next(i for i in range(1, N) if (i * w) % 64 + w > 64)
    rng = np.random.default_rng(bits)
    base = rng.integers(0, q, N, dtype=np.uint64)
    for pos in (0, N - 1, straddle):
        for value, ok in ((q - 1, True), (q, False), ((1 << w) - 1, False)):
            x = base.copy()
            x[pos] = value
            words = rpm.pack_poly(x, w)
            got = rpm.unpack_poly(words, N, w)
            assert np.array_equal(got, x)
            assert bool(np.all(got < np.uint64(q))) == ok
            assert check_poly(words, N, w, q) == ok, (bits, pos, value)


def test_expand_refuses_a_coefficient_equal_to_its_modulus():
    q = [_prime(36), _prime(37)]
    c0 = np.zeros((2, N), dtype=np.uint64)
    for packed in (False, True):
        obj = M.compact(c0, SEED, q, packed)
        bad = obj.copy()
        if packed:
            bad[:N * 36 // 64] = rpm.pack_poly(np.where(np.arange(N) == N - 1, q[0], 0).astype(np.uint64), 36)
        else:
            bad[N - 1] = q[0]
        assert not M.check(bad, N, q, packed)
        with pytest.raises(ValueError):
            M.expand(bad, N, q, packed)
        assert M.expand(obj, N, q, packed).shape == (2, 2, N)


def test_width_64_is_the_plain_form():
    """A context accepts coefficient moduli below 2^61 only (pirgpu_create), so no chain packs at 64 bits; at w = 64 the
    stream is the words themselves, which is the plain form."""
    assert rpm.width(int(chain(N, 61)[0])) == 61
    x = np.random.default_rng(64).integers(0, 1 << 63, N, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    assert np.array_equal(rpm.pack_poly(x, 64), x) and np.array_equal(rpm.unpack_poly(x, N, 64), x)
    assert check_poly(x, N, 64, (1 << 64) - 1 + 1) and not check_poly(x, N, 64, int(x.max()))
