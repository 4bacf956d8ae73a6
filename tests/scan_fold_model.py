"""The fold of the int8-MFMA scan (pir_amd/csrc/scan_mfma.hip) restated on the CPU -- TEST INFRASTRUCTURE.

`to_digits` in both centrings, the digit diagonals T[a + b], and the two folds of value = sum_s T[s] 2^(8 s) mod q:

  integer fold   int64 groups of five diagonals, each made non-negative with `bias` (a multiple of q), the cast to
                 uint64_t, the `<< 40` into 128 bits and reduce128 (SEAL's barrett_reduce_128, arith.h)
  fp64 fold      chunks of four diagonals in one double, f64_norm / f64_mulmod with the centred 2^(32 c) mod q of
                 ctx.hip (`fold_w`), one rounding per operation (the helpers of f64_model.py)

Both compute WHAT THE KERNEL COMPUTES, wrap-around included (a group below -bias comes out of the cast as a huge
unsigned number, as on the GPU), and record how large every intermediate became; the callers decide what to assert.
Everything is Python integers; doubles appear only where the kernel has one.

The worst case of the accumulators is the sign-coherent family (`family`): every column holds the same pair of
operands, whose low digits are all -128 or all +127 and whose top digit is at one end of what the centring leaves --
every term of a digit pair then has the same sign and the sums grow linearly with the columns, not like a random walk.
tests/test_scan_fold_model.py searches it for every instantiated kernel variant; tests/test_gpu_scan_worst_case.py
feeds the same operands to the kernels and uses this model only to prove that its inputs are that hard.  GPU results
are never compared with the model: those are compared with the oracle."""
import os
import re

import numpy as np

from f64_model import Field, Inexact, Stats, floats, ints, _require_exact

SCAN_SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pir_amd", "csrc", "scan_mfma.hip")
M64 = (1 << 64) - 1


def bias_bits_in_source():
    """kBiasBits of scan_mfma.hip: the integer fold's bias is q shifted up to exactly that many bits."""
    with open(SCAN_SOURCE) as f:
        m = re.search(r"constexpr int kBiasBits = (\d+);", f.read())
    assert m, "scan_mfma.hip no longer defines kBiasBits"
    return int(m.group(1))


def variants_in_source():
    """(L, KS, NW) of every PIRGPU_MFMA_CASE of launch_scan_mfma_groups' dispatch."""
    with open(SCAN_SOURCE) as f:
        return [tuple(int(v) for v in m) for m in re.findall(r"PIRGPU_MFMA_CASE\((\d), (\d), (\d)\)", f.read())]


# ---------------------------------------------------------------- operands

def top4_vmax(L):
    p = 256 ** (L - 1)
    return 7 * p + 127 * ((p - 1) // 255)


def centre(x, q, L, top4):
    """The signed value to_digits decomposes: asymmetric (top digit in [-8, 7]) or symmetric about 0."""
    if top4:
        return x - q if x > top4_vmax(L) else x
    return x - q if x > (q >> 1) else x


def int8(v):
    b = v & 0xFF
    return b - 256 if b >= 128 else b


def to_digits(x, q, L, top4):
    """The L signed bytes the kernel stores for residue x (the top one through its nibble in the TOP4 form), and what
    is lost of the value: non-zero when the residue does not fit them."""
    v0 = v = centre(x, q, L, top4)
    d = []
    for _ in range(L):
        b = int8(v)
        d.append(b)
        v = (v - b) >> 8
    if top4:
        n = d[-1] & 0xF                                   # pack_top4 keeps four bits, expand_top4 sign-extends them
        d[-1] = n - 16 if n >= 8 else n
    return d, v0 - sum(b * 256 ** a for a, b in enumerate(d))


def from_digits(low, top, m):
    """The value of m digits whose low ones are all `low` and whose top one is `top`."""
    return top * 256 ** (m - 1) + low * ((256 ** (m - 1) - 1) // 255)


def centred_range(q, L, top4):
    """[lo, hi] of centre(x) over all residues x of q."""
    if top4:
        return (top4_vmax(L) + 1 - q if q - 1 > top4_vmax(L) else 0), min(top4_vmax(L), q - 1)
    return (q >> 1) + 1 - q, q >> 1


def top_ends(low, q, L, top4):
    """(m, smallest top, largest top): the most digits m <= L a residue of q can have with m - 1 low digits all `low`
    (a modulus much smaller than 256^(L - 1) leaves the upper digits zero), and the ends of digit m - 1 then."""
    lo, hi = centred_range(q, L, top4)
    for m in range(L, 0, -1):
        p, base = 256 ** (m - 1), from_digits(low, 0, m)
        dmin, dmax = (-8, 7) if top4 and m == L else (-128, 127)
        tmin, tmax = max(-((base - lo) // p), dmin), min((hi - base) // p, dmax)
        if tmin <= tmax and (m == 1 or (tmin, tmax) != (0, 0)):
            return m, tmin, tmax
    raise ValueError("no residue")


def family(q, L, top4):
    """[(name, value)]: low digits all -128 or all +127, top digit at either end -- centred values of residues of q."""
    out = []
    for low in (-128, 127):
        m, tmin, tmax = top_ends(low, q, L, top4)
        for top in (tmin, tmax):
            v = from_digits(low, top, m)
            d, lost = to_digits(v % q, q, L, top4)
            assert lost == 0 and d == [low] * (m - 1) + [top] + [0] * (L - m), (q, L, top4, low, top, d)
            out.append(("low %d top %d" % (low, top) + (" (%d digits)" % m if m < L else ""), v))
    return out


# ---------------------------------------------------------------- diagonals

def diagonals(db_digits, sel_digits):
    """T[s] = sum over columns of sum_{a + b = s} A[col][a] B[col][b], and the largest sum of |terms| of one diagonal
    (what no order of accumulation can exceed).  db_digits, sel_digits: [cols][L]."""
    L = len(db_digits[0])
    T, A = [0] * (2 * L - 1), [0] * (2 * L - 1)
    for da, db in zip(db_digits, sel_digits):
        for a in range(L):
            for b in range(L):
                T[a + b] += da[a] * db[b]
                A[a + b] += abs(da[a] * db[b])
    return T, max(A)


# ---------------------------------------------------------------- the integer fold

def reduce128(lo, hi, q):
    """arith.h reduce128 with its 64-bit wrap-around."""
    ratio = (1 << 128) // q
    br_lo, br_hi = ratio & M64, ratio >> 64
    carry = (lo * br_lo) >> 64
    t2lo, t2hi = (lo * br_hi) & M64, (lo * br_hi) >> 64
    t1 = (t2lo + carry) & M64
    t3 = (t2hi + (t1 < t2lo)) & M64
    t2lo, t2hi = (hi * br_lo) & M64, (hi * br_lo) >> 64
    t1b = (t1 + t2lo) & M64
    carry = (t2hi + (t1b < t1)) & M64
    qhat = (hi * br_hi + t3 + carry) & M64
    r = (lo - qhat * q) & M64
    return r - q if r >= q else r


class IntFoldStats:
    def __init__(self):
        self.max_group = 0          # largest |G| of a group of five diagonals
        self.min_biased = None      # smallest G + bias (negative: the cast wraps)
        self.max_biased = 0         # largest G + bias
        self.max_v = 0              # largest value handed to reduce128
        self.int64_overflow = False


def int_fold(T, q, bias_bits, st=None):
    """The F64F = false branch for one lane value: T[0 .. 2L-2] -> canonical residue (as the kernel computes it)."""
    st = st or IntFoldStats()
    NS = len(T)
    NG = (NS + 4) // 5
    bias = q << (bias_bits - q.bit_length())
    r = 0
    for gq in range(NG - 1, -1, -1):
        G = sum(T[s] << (8 * (s - gq * 5)) for s in range(gq * 5, min(gq * 5 + 5, NS)))
        biased = G + bias
        if not (-(1 << 63) <= G < (1 << 63) and -(1 << 63) <= biased < (1 << 63)):
            st.int64_overflow = True
        st.max_group = max(st.max_group, abs(G))
        st.min_biased = biased if st.min_biased is None else min(st.min_biased, biased)
        st.max_biased = max(st.max_biased, biased)
        u = biased & M64                                  # (uint64_t)(G + (int64_t)bias)
        if gq == NG - 1 and NG > 1:
            r = u
        else:
            v = ((r << 40) + u) & ((1 << 128) - 1)
            st.max_v = max(st.max_v, (r << 40) + u)
            r = reduce128(v & M64, v >> 64, q)
    return r, st


# ---------------------------------------------------------------- the fp64 fold

class FoldField(Field):
    """f64_model.Field's mulmod / norm / add for one modulus, without the transform's tables."""

    def __init__(self, q):
        self.q = int(q)
        self.qd = np.float64(self.q)
        self.qinv = np.float64(1.0) / self.qd
        w, acc, self.fold_w = (1 << 32) % self.q, (1 << 32) % self.q, []
        for _ in range(3):                                # ctx.hip: 2^(32 (e + 1)) mod q, centred
            self.fold_w.append(np.float64(-(self.q - acc) if acc > self.q // 2 else acc))
            acc = acc * w % self.q


class F64FoldStats(Stats):
    def __init__(self):
        super().__init__()
        self.max_chunk = 0.0        # largest |C| of a chunk of four diagonals
        self.max_acc = 0.0          # largest |acc| of the sum of the chunks' residues


def f64_fold(T, q, st=None):
    """The F64F = true branch for M lane values at once: T = object array [2L-1, M] -> [M] canonical residues.
    Raises f64_model.Inexact where a double the kernel keeps is not the integer it stands for."""
    st = st or F64FoldStats()
    F = FoldField(q)
    T = np.asarray(T, dtype=object)
    NS, M = T.shape
    NC = (NS + 3) // 4
    acc = np.zeros(M)
    for c in range(NC - 1, -1, -1):
        C = np.zeros(M)
        for s in range(min(4 * c + 3, NS - 1), 4 * c - 1, -1):
            E = ints(C) * 256 + T[s]                       # fma(C, 256, (double)T[s]): one rounding
            C = floats(E)
            _require_exact(C, E, "chunk of four diagonals")
        st.max_chunk = max(st.max_chunk, float(np.abs(C).max()))
        term = F.norm(C, st) if c == 0 else F.mulmod(C, F.fold_w[c - 1], st)
        acc = F.add(acc, term, st)
        st.max_acc = max(st.max_acc, float(np.abs(acc).max()))
    r = F.norm(acc, st)
    r = np.where(r < 0, r + F.qd, r)
    return [int(v) for v in F._canonical(r)], st


# ---------------------------------------------------------------- the 64-bit scans' lazy accumulators (kernels.hip)

KERNELS_SOURCE = os.path.join(os.path.dirname(SCAN_SOURCE), "kernels.hip")
LIMB = (1 << 28) - 1


def limb_lazy_in_source():
    with open(KERNELS_SOURCE) as f:
        m = re.search(r"constexpr uint32_t kLimbLazy = (\d+);", f.read())
    assert m, "kernels.hip no longer defines kLimbLazy"
    return int(m.group(1))


def lazy_limit(bits):
    """ctx.hip: terms an AccWide sum takes between folds, from the size of the largest modulus."""
    return 1 << min(30, max(0, 128 - 2 * bits))


def limb_max(q):
    """The residue of q whose two 28-bit limbs are both as large as a residue's can be."""
    hi = (q - 1) >> 28
    r = (hi << 28) | LIMB
    return r if r < q else ((hi - 1) << 28) | LIMB


class AccLimb:
    """Three 64-bit sums of 28-bit limb products, with the wrap-around of uint64_t; `wrapped` records one."""

    def __init__(self, q):
        self.q, self.s00, self.s01, self.s11, self.wrapped = q, 0, 0, 0, False
        self.max = [0, 0, 0]

    def _add(self, s, v):
        s += v
        if s > M64:
            self.wrapped = True
        return s & M64

    def mac(self, a, b):
        a0, a1, b0, b1 = a & LIMB, a >> 28, b & LIMB, b >> 28
        self.s00 = self._add(self.s00, a0 * b0)
        self.s01 = self._add(self._add(self.s01, a0 * b1), a1 * b0)
        self.s11 = self._add(self.s11, a1 * b1)
        self.max = [max(m, s) for m, s in zip(self.max, (self.s00, self.s01, self.s11))]

    def fold(self):
        t = (self.s00 + (self.s01 << 28) + (self.s11 << 56)) & ((1 << 128) - 1)
        return reduce128(t & M64, t >> 64, self.q)

    def set(self, r):
        self.s00, self.s01, self.s11 = r, 0, 0


class AccWide:
    """One 128-bit sum of whole products."""

    def __init__(self, q):
        self.q, self.v, self.wrapped, self.max = q, 0, False, 0

    def mac(self, a, b):
        self.v += a * b
        if self.v >> 128:
            self.wrapped = True
        self.v &= (1 << 128) - 1
        self.max = max(self.max, self.v)

    def fold(self):
        return reduce128(self.v & M64, self.v >> 64, self.q)

    def set(self, r):
        self.v = r


def lazy_scan(acc, pairs, interval):
    """scan_kernel's schedule: `interval` products, then the sum is folded and carried as a residue while columns remain."""
    for n, (a, b) in enumerate(pairs):
        acc.mac(a, b)
        if (n + 1) % interval == 0 and n + 1 < len(pairs):
            acc.set(acc.fold())
    return acc.fold()
