"""CPU model of compact queries, in numpy integers.

A compact query ciphertext is c0 -- [k][N] canonical residues of the data moduli q_0 .. q_{k-1}, coefficient form --
plus a 64-byte public seed; c1 = sample_poly_uniform(BlakePRNG(seed), q_0 .. q_{k-1}) (tests/seal_wire.py).  c0 comes
plain (k N little-endian u64 words) or packed (polynomial j as the stream tests/reply_pack_model.py's pack_poly writes at
width(q_j) bits a coefficient); the 8 words of the seed follow c0 in both.  Expanded it is an ordinary [2][k][N]
ciphertext."""
import numpy as np

import reply_pack_model as rpm
import seal_wire

SEED_WORDS = seal_wire.SEED_BYTES // 8


def widths(q, packed):
    return [rpm.width(v) if packed else 64 for v in q]


def words(N, q, packed):
    """Words of one compact ciphertext over the data moduli q: k N + 8, or sum_j N w_j / 64 + 8."""
    return sum(rpm.poly_words(N, w) for w in widths(q, packed)) + SEED_WORDS


def wire_bytes(N, q, packed):
    """Bytes of c0 and the seed alone (the issue's figure: 2 * 4096 * 36 / 8 + 64 = 36 928 at the headline shape)."""
    return words(N, q, packed) * 8


def compact(c0, seed, q, packed):
    """c0 [k, N] canonical residues + seed (64 bytes) -> [words] uint64."""
    c0 = np.asarray(c0, dtype=np.uint64)
    k, N = c0.shape
    assert k == len(q) and len(seed) == seal_wire.SEED_BYTES
    parts = []
    for j, w in enumerate(widths(q, packed)):
        assert not np.any(c0[j] >= np.uint64(int(q[j]))), "residue is not canonical"
        parts.append(rpm.pack_poly(c0[j], w))
    parts.append(np.frombuffer(seed, dtype="<u8").astype(np.uint64))
    out = np.concatenate(parts)
    assert out.shape == (words(N, q, packed),)
    return out


def split(obj, N, q, packed):
    """[words] uint64 -> (c0 [k, N] as the words say it, without a range check, seed bytes)."""
    obj = np.ascontiguousarray(obj, dtype=np.uint64)
    assert obj.shape == (words(N, q, packed),)
    c0 = np.empty((len(q), N), dtype=np.uint64)
    at = 0
    for j, w in enumerate(widths(q, packed)):
        pw = rpm.poly_words(N, w)
        c0[j] = rpm.unpack_poly(obj[at:at + pw], N, w)
        at += pw
    return c0, obj[at:].astype("<u8").tobytes()


def check(obj, N, q, packed):
    """The host's verdict: every c0 coefficient below its modulus."""
    c0, _ = split(obj, N, q, packed)
    return all(not np.any(c0[j] >= np.uint64(int(q[j]))) for j in range(len(q)))


def expand(obj, N, q, packed):
    """[words] uint64 -> [2, k, N] uint64; raises ValueError on a c0 coefficient >= q_j."""
    if not check(obj, N, q, packed):
        raise ValueError("ciphertext data is invalid (coefficient out of range)")
    c0, seed = split(obj, N, q, packed)
    return np.stack([c0, seal_wire.sample_poly_uniform(seed, [int(v) for v in q], N)])


def expand_all(objs, N, q, packed):
    """[..., words] -> [..., 2, k, N]."""
    objs = np.asarray(objs, dtype=np.uint64)
    flat = objs.reshape(-1, objs.shape[-1])
    out = np.stack([expand(o, N, q, packed) for o in flat])
    return out.reshape(objs.shape[:-1] + out.shape[1:])
