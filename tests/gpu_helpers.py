"""Helpers shared by the GPU parity tests: oracle PirParams <-> product PIRParameters."""
import numpy as np

import oracle
import pir_amd
from pir_amd.parameters import EncryptionParams, PIRParameters


def to_product_params(p: "oracle.PirParams") -> PIRParameters:
    enc = EncryptionParams(p.N, list(p.moduli), p.t)
    return PIRParameters(num_items=p.num_items, num_pt=p.num_pt, dimensions=list(p.dimensions),
                         encryption_parameters=enc, bytes_per_item=p.bytes_per_item,
                         items_per_plaintext=p.items_per_plaintext, bits_per_coeff=p.bits_per_coeff,
                         use_ciphertext_multiplication=p.use_ciphertext_multiplication)


def random_ct(orc, rng, n=1):
    out = np.empty((n, 2, orc.k, orc.N), dtype=np.uint64)
    for j in range(orc.k):
        out[:, :, j, :] = rng.integers(0, orc.moduli[j], size=(n, 2, orc.N), dtype=np.uint64)
    return out


def random_key(orc, rng):
    key = np.empty((orc.k, 2, orc.k + 1, orc.N), dtype=np.uint64)
    for i in range(orc.k + 1):
        key[:, :, i, :] = rng.integers(0, orc.moduli[i], size=(orc.k, 2, orc.N), dtype=np.uint64)
    return key


def chain(N, data_bits, special_bits=None):
    """Coefficient modulus chain with data primes of `data_bits` bits each (an int = two of that size, or a list) and
    a special prime of `special_bits` (default: the largest data size), found the way SEAL's CoeffModulus::Create does."""
    data = [data_bits, data_bits] if isinstance(data_bits, int) else list(data_bits)
    return oracle.coeff_modulus_create(N, data + [max(data) if special_bits is None else special_bits])


def smallest_primes(N, bits, count):
    """The `count` smallest NTT-friendly primes (== 1 mod 2N) of exactly `bits` bits, ascending: the ones just above
    2^(bits - 1), where a constant derived from the bit count alone (a shift of q up to a fixed size) is smallest."""
    found, v = [], (1 << (bits - 1)) + 1
    while len(found) < count and v < (1 << bits):
        if oracle.is_prime(v):
            found.append(v)
        v += 2 * N
    if len(found) < count:
        raise ValueError("not enough primes")
    return found


def chain_low(N, data_bits, special_bits=None):
    """chain()'s counterpart at the other end of every size: the SMALLEST NTT-friendly primes of `data_bits` bits (an int =
    two of that size, or a list), the special prime -- the largest of its size -- after them."""
    data = [data_bits, data_bits] if isinstance(data_bits, int) else list(data_bits)
    need = {}
    for b in data:
        need[b] = need.get(b, 0) + 1
    table = {b: smallest_primes(N, b, cnt) for b, cnt in need.items()}
    special = oracle.coeff_modulus_create(N, [max(data) if special_bits is None else special_bits])
    return [table[b].pop(0) for b in data] + special


def structured_patterns(q, N, rng):
    """Deterministic worst-case residue vectors of one modulus: [(name, uint64[N])].  Random inputs stay a factor
    sqrt(N) inside the worst-case bounds of the transforms; these sit on them."""
    q = int(q)
    pos = np.arange(N)
    full = lambda v: np.full(N, v, dtype=np.uint64)
    out = [("all 0", full(0)), ("all q-1", full(q - 1)), ("all q/2", full(q // 2)), ("all q/2+1", full(q // 2 + 1))]
    for i in (0, 1, N // 2, N - 1):
        for c in (1, q - 1):
            v = full(0)
            v[i] = c
            out.append(("%d * delta_%d" % (c, i), v))
    for b in range(N.bit_length() - 1):
        m = ((pos >> b) & 1).astype(bool)
        out.append(("bit %d set -> q-1" % b, np.where(m, q - 1, 0).astype(np.uint64)))
        out.append(("bit %d clear -> q-1" % b, np.where(m, 0, q - 1).astype(np.uint64)))
    out.append(("random top", (q - 1 - rng.integers(0, 1000, size=N)).astype(np.uint64)))
    out.append(("alternating 0 / q-1", np.where(pos & 1, q - 1, 0).astype(np.uint64)))
    return out


def device_to_seal_order(a):
    """NTT-domain polynomials in device order (last axis; slot e * N/16 + tid holds SEAL position 16 * tid + e,
    pir_amd/csrc/ntt_core.h) -> SEAL's order."""
    a = np.asarray(a)
    N = a.shape[-1]
    return np.ascontiguousarray(a.reshape(a.shape[:-1] + (16, N // 16)).swapaxes(-1, -2).reshape(a.shape))


def seal_to_device_order(a):
    """The inverse of device_to_seal_order.  N = 32768 keeps SEAL's order on the device (ntt_ring32k.hip)."""
    a = np.asarray(a)
    N = a.shape[-1]
    if N >= 32768:
        return np.ascontiguousarray(a)
    return np.ascontiguousarray(a.reshape(a.shape[:-1] + (N // 16, 16)).swapaxes(-1, -2).reshape(a.shape))


def all_to_all_in_process(recvs, sends, recv_splits, send_splits):
    """What torch.distributed.all_to_all_single does, between in-process 'ranks' (1-D tensors, element splits)."""
    G = len(sends)
    for dst in range(G):
        ro = 0
        for src in range(G):
            so = sum(send_splits[src][:dst])
            n = send_splits[src][dst]
            assert n == recv_splits[dst][src]
            recvs[dst][ro:ro + n].copy_(sends[src][so:so + n])
            ro += n
    # the copies run on torch's current stream, the library's kernels on its own non-blocking streams: nothing orders the
    # two but the host (a product caller uses Comm, which waits, or the entry points' after / then streams)
    if recvs and recvs[0].is_cuda:
        import torch
        torch.cuda.synchronize()
