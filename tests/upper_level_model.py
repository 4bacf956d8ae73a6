"""The two accumulation schedules of the upper recursion level restated on the CPU -- TEST INFRASTRUCTURE, next to
f64_model.py (whose mulmod / norm / add check that every double the kernel keeps IS the integer it stands for).

  fp64      upper_fused_kernel<kNttF64 / kNttF64Wide> (ntt_kernels.hip) and upper_mac_kernel (kernels.hip): per child
            acc += f64_mulmod(x, w), f64_norm after every 8th child of the launch; at the end of a block of children the
            sum carried from the block before is added, f64_norm, and the next block restarts its count; the last block's
            sum is made canonical.  The fused kernel is the one-block case.
  integer   upper_fused_kernel<kNttInt> and upper_mac_int_kernel (ntt_ring32k.hip): a 128-bit sum of 64 x 64-bit products,
            folded (reduce128) after every `lazy_limit` children of the launch and at the end of a block, the residue of the
            block before added with add_mod.  Sums are masked to 128 bits, as the hardware's would wrap.  Two WRONG
            variants exist so that a test can show its operands tell them apart: "no fold" (never folded before the end of
            the block) and "late" (folded one child too late).

The operands of tests/test_gpu_upper_worst_case.py are built here as well (chunk values, their plain lift, the selector
that puts every child's product on one residue), so that the model test and the GPU test speak about the same numbers.
GPU results are never compared with this model: those are compared with the oracle and with closed forms."""
import numpy as np

from f64_model import Stats, floats, ints

MASK128 = (1 << 128) - 1


class UpperStats(Stats):
    def __init__(self):
        super().__init__()
        self.max_term = 0.0      # largest |f64_mulmod result| / q over all children and slots
        self.max_acc = 0.0       # largest |running sum| / q, before a normalisation takes it down
        self.max_acc_value = 0.0  # ... as an absolute number (an exact integer below 2^53)
        self.flipped = 0         # terms whose sign differs from the first child's in that slot


def lazy_limit(q):
    """device_params / ctx.hip: 128-bit products summed before a reduction, 2^(128 - 2 bits), at most 2^30."""
    return min(1 << 30, 1 << (128 - 2 * int(q).bit_length()))


def lift(v, t, q=None):
    """Plain lift of a chunk value v < t: the signed representative the fp64 kernels start from (v - t above the
    threshold), or with `q` the canonical residue of the integer kernels."""
    x = v - t if v >= (t + 1) >> 1 else v
    return x if q is None else x % q


def fp64_schedule(F, xs, ws, blocks):
    """xs[i], ws[i]: float64 arrays over the slots (signed transformed plaintext, canonical selector residue) of child i;
    blocks: children per launch, in order.  -> (canonical residues as Python ints, UpperStats)."""
    assert sum(blocks) == len(xs) == len(ws)
    st = UpperStats()
    carried, i, first_sign = None, 0, None

    def seen(a):
        m = float(np.abs(a).max())
        st.max_acc = max(st.max_acc, m / float(F.qd))
        st.max_acc_value = max(st.max_acc_value, m)

    for n_here in blocks:
        acc = np.zeros_like(xs[0])
        since = 0
        for _ in range(n_here):
            term = F.mulmod(xs[i], ws[i], st)
            st.max_term = max(st.max_term, float(np.abs(term).max() / F.qd))
            if first_sign is None:
                first_sign = np.sign(term)
            st.flipped += int(np.count_nonzero(np.sign(term) != first_sign))
            acc = F.add(acc, term, st)
            seen(acc)
            i += 1
            since += 1
            if since == 8:
                since = 0
                acc = F.norm(acc, st)
        if carried is not None:
            acc = F.add(acc, carried, st)
            seen(acc)
        carried = F.norm(acc, st)
    r = np.where(carried < 0, carried + F.qd, carried)
    out = [int(v) for v in r.tolist()]
    assert all(0 <= v < F.q for v in out)
    return out, st


def reduce128(v, q):
    assert 0 <= v <= MASK128
    return v % q


def int_schedule(q, xs, ws, limit, blocks, variant="folded"):
    """xs[i], ws[i]: canonical residues (Python ints) of child i in one slot.  -> the residue the schedule leaves."""
    assert sum(blocks) == len(xs) == len(ws) and variant in ("folded", "no fold", "late")
    fold_at = {"folded": limit, "no fold": None, "late": limit + 1}[variant]
    carried, i = None, 0
    for n_here in blocks:
        a, since = 0, 0
        for _ in range(n_here):
            a = (a + xs[i] * ws[i]) & MASK128
            i += 1
            since += 1
            if since == fold_at:
                since = 0
                a = reduce128(a, q)
        s = reduce128(a, q)
        if carried is not None:
            s = s + carried - q if s + carried >= q else s + carried          # add_mod
        carried = s
    return carried


# ---------------------------------------------------------------- operands

def chunk_layout(qs, b):
    """CiphertextReencoder::Encode order: [(polynomial, source residue, shift)] -- b-bit fields of every residue."""
    out = []
    for poly in range(2):
        for j, q in enumerate(qs):
            for i in range(-(-int(q).bit_length() // b)):
                out.append((poly, j, i * b))
    return out


def all_ones_value(q, b):
    """The residue < q whose b-bit chunks are all ones except the top one, which is as large as q allows less one (and
    at least 1: a zero chunk lifts to a zero plaintext, and the reference refuses its product as transparent)."""
    top_shift = (-(-int(q).bit_length() // b) - 1) * b
    top = (q >> top_shift) - 1
    assert top >= 1, (q, b)
    v = (top << top_shift) | ((1 << top_shift) - 1)
    assert v < q
    return v


def coherent_selector(F, x_signed, r0):
    """w with x * w == r0 (mod q) in every slot: float64 array of canonical residues."""
    q = F.q
    X = [int(v) % q for v in x_signed.tolist()]
    assert all(X), "a transformed chunk with a zero slot has no inverse there"
    return floats(np.array([r0 * pow(v, -1, q) % q for v in X], dtype=object))


def target(q):
    """0.45 q rounded up, so that eight terms are 3.6 q or more in integers: far enough from q / 2 that the quotient
    estimate of a 49-bit product (error up to ~0.04) does not flip the sign, as it does for some terms at 0.49."""
    return (45 * q + 99) // 100
