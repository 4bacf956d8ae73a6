"""CPU model of packed replies (PIRGPU_CREATE_PACKED_REPLIES), in numpy integers.

A reply ciphertext is [2][r][N] canonical residues (r = result_primes or k).  For modulus q_j the width is
w_j = bit length of q_j - 1.  Polynomial (c, j) becomes a little-endian bit stream of N * w_j bits -- bit b of
coefficient i is stream bit i * w_j + b -- stored as N * w_j / 64 little-endian u64 words (whole words: N is a multiple
of 64).  A packed ciphertext is its 2 r polynomials in the order (c, j): 2 * sum_j N * w_j / 64 words.  Nothing else
changes: ciphertext count, order and plane-major layout stay.  unpack(pack(x)) == x for every canonical x."""
import numpy as np


def width(q):
    """Bits a canonical residue of q needs: the bit length of q - 1."""
    return (int(q) - 1).bit_length()


def widths(q, r=None):
    q = [int(v) for v in q]
    return [width(v) for v in (q if r is None else q[:r])]


def poly_words(N, w):
    assert N % 64 == 0
    return N * w // 64


def ct_words(N, q, r=None):
    """Words of one packed ciphertext over the first r moduli of q."""
    return 2 * sum(poly_words(N, w) for w in widths(q, r))


def pack_poly(x, w):
    """x: [N] uint64, every value < 2^w -> [N w / 64] uint64."""
    x = np.ascontiguousarray(x, dtype=np.uint64)
    assert x.ndim == 1 and 1 <= w <= 64
    if w < 64:
        assert not np.any(x >> np.uint64(w)), "value does not fit its width"
    # bit b of coefficient i -> stream bit i * w + b; numpy's little bit order is exactly "bit s of the stream is bit
    # s % 8 of byte s // 8", and little-endian u64 words over those bytes put stream bit s at bit s % 64 of word s // 64
    bits = np.unpackbits(x.view(np.uint8).reshape(-1, 8), axis=1, bitorder="little")[:, :w]
    return np.packbits(bits.reshape(-1), bitorder="little").view("<u8").astype(np.uint64)


def unpack_poly(words, N, w):
    """[N w / 64] uint64 -> [N] uint64."""
    words = np.ascontiguousarray(words, dtype="<u8")
    assert words.shape == (poly_words(N, w),)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little").reshape(N, w)
    full = np.zeros((N, 64), dtype=np.uint8)
    full[:, :w] = bits
    return np.packbits(full, axis=1, bitorder="little").reshape(-1).view("<u8").astype(np.uint64)


def pack(cts, q):
    """cts [..., 2, r, N] uint64 canonical residues of q[0..r-1] -> [..., ct_words] uint64."""
    cts = np.asarray(cts, dtype=np.uint64)
    r, N = cts.shape[-2], cts.shape[-1]
    assert cts.shape[-3] == 2 and r <= len(q)
    ws = widths(q, r)
    flat = cts.reshape(-1, 2, r, N)
    out = np.empty((flat.shape[0], ct_words(N, q, r)), dtype=np.uint64)
    for n in range(flat.shape[0]):
        at = 0
        for c in range(2):
            for j in range(r):
                assert not np.any(flat[n, c, j] >= np.uint64(int(q[j]))), "residue is not canonical"
                pw = poly_words(N, ws[j])
                out[n, at:at + pw] = pack_poly(flat[n, c, j], ws[j])
                at += pw
    return out.reshape(cts.shape[:-3] + (out.shape[1],))


def unpack(packed, q, r, N):
    """[..., ct_words] uint64 -> [..., 2, r, N] uint64; raises ValueError on a coefficient >= q_j."""
    packed = np.asarray(packed, dtype=np.uint64)
    ws = widths(q, r)
    assert packed.shape[-1] == ct_words(N, q, r)
    flat = packed.reshape(-1, packed.shape[-1])
    out = np.empty((flat.shape[0], 2, r, N), dtype=np.uint64)
    for n in range(flat.shape[0]):
        at = 0
        for c in range(2):
            for j in range(r):
                pw = poly_words(N, ws[j])
                out[n, c, j] = unpack_poly(flat[n, at:at + pw], N, ws[j])
                at += pw
                if np.any(out[n, c, j] >= np.uint64(int(q[j]))):
                    raise ValueError("packed coefficient out of range")
    return out.reshape(packed.shape[:-1] + (2, r, N))
