"""The upper recursion level (d >= 2: re-encode, plain lift, forward NTT, multiply-accumulate with the selectors over the
children of a row) at COHERENT worst-case operands: every child of a row adds a term of the same sign and of (nearly) the
largest size, so that the fp64 sums of upper_fused_kernel / upper_mac_kernel reach the eight terms of 0.45 q between two
normalisations their comments budget for, and the 128-bit sums of upper_fused_kernel<kNttInt> / upper_mac_int_kernel
cross the lazy_limit children after which they must be folded -- instead of the random walk (0.8 q rms) and the 2^126
that random operands leave (tests/upper_level_model.py, tests/test_upper_level_model.py: the same operands on a CPU model
of both schedules, where removing the fold or folding one child late changes the residue).

How the operands get there through the public interface (d = 2, dims [n, 2], all n x 2 plaintexts the constant 1):

  children   a constant-1 plaintext lifts to 1 in every NTT slot, so a row sum is the sum of the two scan selectors.  With
             Y0 random and Y1 = NTT(y) - Y0, EVERY child of the upper level is the ciphertext y, chosen freely in
             coefficient form; neither scan selector is zero, which keeps the reference's "transparent ciphertext"
             refusal away.
  "delta"    y = the residue whose b-bit chunks are all ones (the top chunk as large as q allows) in coefficient 0 and
             zero elsewhere: chunk e lifts to x_e * delta_0, x_e = q - (t - 2^b + 1) for the full chunks, whose transform
             is the constant x_e.  Upper selectors all q - 1: every term is x_e (q - 1), and the reply is the closed form
             n x_e (q - 1) mod q in coefficient 0 and zero elsewhere -- a reference that involves neither the oracle nor a
             transform.
  "coherent" y pseudo-random; the transform X of one chunk is known on the CPU (the oracle's plain lift + NTT) and the
             selector is w = r0 X^-1 with r0 = 0.45 q, per slot: every child adds the residue r0 in every slot of that
             chunk's output (component 0 aims at chunk 0, component 1 at the first chunk of the second polynomial), with
             products |x| w of full size in the quotient estimates.

Every case runs as a group of 3 through stage_batch + batch_run_selectors (member 0 as constructed, member 1 with the
negated target -- q - r0, resp. selectors 1 --, member 2 random selectors; with the int8-MFMA scan, i.e. moduli below
2^55, the three share every launch of the upper level, with the 64-bit scans each member gets launches of its own at the
batch pipeline's chunk count, and UPPER_PARTS counts three times a member's parts) and member by member as a lone vector through
PIRDatabase.multiply (the upper selectors as their inverse transforms).  Every reply is compared bit for bit with the
oracle's db_multiply, the delta replies with the closed form as well.  Before anything runs on the GPU the case asserts on
the CPU that its operands are worst case (the 2^128 wrap inequality in Python integers, or the model's 3.6 q); the path
is asserted through arith_info / scan_info, and the counter option UPPER_PARTS tells how the children of a row were cut
into chunks (fused) or blocks (split), so that a case cannot pass without a launch crossing the interval.

Out of scope: double-form selectors (SELF64) are written by a batch lane's own expansion on the device and cannot be
injected -- encrypted selectors are pseudo-random by nature; d = 3 at worst case -- level 0's children are level 1's
output, which this construction does not control: d = 3 stays with the random tests."""
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import oracle
import pir_amd
import upper_level_model as U
from f64_model import Field, floats
from gpu_helpers import chain, chain_low, device_to_seal_order, seal_to_device_order, to_product_params

pytestmark = pytest.mark.gpu


class Case:
    """Parameters, oracle, operands and expected replies of one (ring, data primes, end of the size, children, kind)."""

    def __init__(self, N, bits, low_end, n, t_bits, kind):
        t0 = time.time()
        self.N, self.n, self.kind = N, n, kind
        moduli = (chain_low if low_end else chain)(N, list(bits))
        self.qs = [int(q) for q in moduli[:-1]]
        self.k = k = len(self.qs)
        self.t = t = oracle.plain_modulus_batching(N, t_bits)
        self.b = b = t.bit_length() - 1
        p = oracle.create_pir_parameters(2 * n, 0, 2, N=N, moduli=moduli, t=t)
        assert p.num_pt == 2 * n
        p.dimensions = [n, 2]
        self.params = p
        self.orc = orc = oracle.Oracle.from_params(p)
        self.layout = U.chunk_layout(self.qs, b)
        self.E = len(self.layout)
        assert self.E == 2 * orc.expansion_ratio()
        rng = np.random.default_rng(1000 * bits[0] + n + 7 * low_end + N)
        # the database: every plaintext the constant 1, which lifts to 1 in every slot
        self.coeff_rows = [np.array([1], dtype=np.uint64)] * (2 * n)
        self.db_ntt = np.ones((2 * n, k, N), dtype=np.uint64)
        assert np.array_equal(orc.db_from_coeffs(self.coeff_rows[:1])[0], self.db_ntt[0])
        # the child every row sum is
        y = np.zeros((2, k, N), dtype=np.uint64)
        for j, q in enumerate(self.qs):
            if kind == "delta":
                y[:, j, 0] = U.all_ones_value(q, b)
            else:
                y[:, j, :] = rng.integers(0, q, size=(2, N), dtype=np.uint64)
        self.y = y
        Y = orc.ct_ntt_fwd(y)
        self.scan = np.empty((2, 2, k, N), dtype=np.uint64)           # SEAL order
        for j, q in enumerate(self.qs):
            self.scan[0, :, j] = rng.integers(1, q, size=(2, N), dtype=np.uint64)
            self.scan[1, :, j] = (Y[:, j].astype(object) - self.scan[0, :, j].astype(object)) % q
        assert self.scan.all()
        self.scan_coeff = np.stack([orc.ct_ntt_inv(self.scan[c]) for c in range(2)])
        # chunk values of y and their lifts: x[e][jt] as canonical residues over the coefficients
        self.chunks = [(y[poly, j] >> np.uint64(sh)) & np.uint64((1 << b) - 1) for poly, j, sh in self.layout]
        assert np.array_equal(np.stack(self.chunks), orc.reencode(y))
        # upper selectors of the three members, SEAL order, one ciphertext per member for 0 and 1 (the same for every child)
        one = np.empty((2, 2, k, N), dtype=np.uint64)
        if kind == "delta":
            for j, q in enumerate(self.qs):
                one[0, :, j], one[1, :, j] = q - 1, 1
        else:
            self.aim = (0, self.E // 2)
            for j, q in enumerate(self.qs):
                r0 = U.target(q)
                for comp, e in enumerate(self.aim):
                    lifted = np.array([U.lift(int(v), t, q) for v in self.chunks[e]], dtype=np.uint64)
                    X = [int(v) for v in orc.ntt_fwd(j, lifted)]
                    assert all(X)
                    inv = [pow(v, -1, q) for v in X]
                    one[0, comp, j] = np.array([r0 * v % q for v in inv], dtype=np.uint64)
                    one[1, comp, j] = np.array([(q - r0) * v % q for v in inv], dtype=np.uint64)
        self.upper = [np.broadcast_to(one[0], (n, 2, k, N)), np.broadcast_to(one[1], (n, 2, k, N))]
        rnd = np.empty((n, 2, k, N), dtype=np.uint64)
        for j, q in enumerate(self.qs):
            rnd[:, :, j] = rng.integers(0, q, size=(n, 2, N), dtype=np.uint64)
        self.upper.append(rnd)
        self.upper_coeff = [np.broadcast_to(orc.ct_ntt_inv(one[0]), (n, 2, k, N)),
                            np.broadcast_to(orc.ct_ntt_inv(one[1]), (n, 2, k, N)),
                            np.stack([orc.ct_ntt_inv(rnd[i]) for i in range(n)])]
        self.expected = []
        for m in range(3):
            seal = np.ascontiguousarray(np.concatenate([self.upper[m], self.scan]))
            rc, exp = orc.db_multiply(self.db_ntt, p.dimensions, seal, sv_is_ntt=np.ones(n + 2, np.uint8))
            assert rc == 0 and exp.shape[0] == self.E and exp.any()
            self.expected.append(exp)
        if kind == "delta":
            for m, s in ((0, None), (1, 1)):
                for e in range(self.E):
                    for jt, q in enumerate(self.qs):
                        x = U.lift(int(self.chunks[e][0]), t, q)
                        want = n * x * (q - 1 if s is None else s) % q
                        got = self.expected[m][e, :, jt]
                        assert (got[:, 0] == want).all() and not got[:, 1:].any(), (m, e, jt)
        else:
            for m in (0, 1):          # the aimed chunk's output is the constant n r0 (n (q - r0)) in NTT form: n r0 delta_0
                for comp, e in enumerate(self.aim):
                    for jt, q in enumerate(self.qs):
                        r = U.target(q) if m == 0 else q - U.target(q)
                        got = self.expected[m][e, comp, jt]
                        assert got[0] == n * r % q and not got[1:].any(), (m, comp, e, jt)
        self.sv_dev = np.stack([np.concatenate([seal_to_device_order(self.upper[m]), seal_to_device_order(self.scan)])
                                for m in range(3)])
        assert np.array_equal(device_to_seal_order(self.sv_dev[2, :n]), rnd) or N >= 32768
        self.cpu_seconds = time.time() - t0

    def coeff_sv(self, m):
        """Selection vector m in coefficient form (what PIRDatabase.multiply takes)."""
        return np.ascontiguousarray(np.concatenate([self.upper_coeff[m], self.scan_coeff]))

    # ---- how hard the operands are, asserted before anything runs on the GPU
    def assert_integer_sums_wrap(self, limit, longest):
        """`longest` children in one launch are more than one interval, and their products, unfolded, pass 2^128 -- while
        one interval's do not (the kernels' contract)."""
        assert self.kind == "delta" and longest > limit
        for jt, q in enumerate(self.qs):
            assert U.lazy_limit(q) == limit
            full = [e for e, (_, j, sh) in enumerate(self.layout) if int(self.chunks[e][0]) == (1 << self.b) - 1]
            assert len(full) >= 2 * (self.k if self.k > 1 else 1)
            for e in full:
                x = U.lift(int(self.chunks[e][0]), self.t, q)
                assert x == q - (self.t - (1 << self.b) + 1)
                assert limit * x * (q - 1) + q < 2 ** 128 <= (limit + 1) * x * (q - 1), (jt, e)
                want = longest * x * (q - 1) % q
                for variant in ("no fold", "late"):
                    assert U.int_schedule(q, [x] * longest, [q - 1] * longest, limit, [longest], variant) != want

    def assert_fp64_sums_are_coherent(self, mode, blocks):
        """The model's running sum over `blocks` (children per launch) reaches 8 x 0.45 q on the aimed chunk, exactly."""
        assert self.kind == "coherent" and self.k == 1 and max(blocks) >= 8 and sum(blocks) == self.n
        q = self.qs[0]
        assert self.b <= 31 and self.t < q                          # the kernels' fast lift
        F = Field(q, self.N, self.orc.psi(0))
        lifted = [U.lift(int(v), self.t) for v in self.chunks[0]]
        x, _ = F.forward(lifted, mode, canonical=False)
        w = floats(np.array([int(v) for v in self.upper[0][0, 0, 0]], dtype=object))
        out, st = U.fp64_schedule(F, [x] * self.n, [w] * self.n, blocks)
        assert set(out) == {self.n * U.target(q) % q}
        print("model, %d-bit q, blocks %s: max |term| %.3f q, max |sum| %.3f q" % (q.bit_length(), blocks, st.max_term,
                                                                                 st.max_acc))
        assert st.max_term <= 0.7 and st.max_acc >= 3.6 and st.max_acc_value < 2 ** 53


@functools.lru_cache(maxsize=2)
def case_of(N, bits, low_end, n, t_bits, kind):
    return Case(N, bits, low_end, n, t_bits, kind)


def run(case, options, expect_arith, expect_scan, lone_parts, group_parts):
    """One context with `options`: its path, the parts its upper level is cut into, its replies."""
    import torch
    t0 = time.time()
    pp = to_product_params(case.params)
    db = pir_amd.PIRDatabase.Create(pp)
    for name, value in options.items():
        db.set_option(name, value)
    db.populate_coeffs(case.coeff_rows)
    srv = pir_amd.PIRServer(db, pp)
    arith, scan = srv.arith_info(), srv.scan_info()
    print("arith_info", arith, "scan_info", scan)
    for key, value in expect_arith.items():
        assert arith[key] == value, (key, arith)
    for key, value in dict(expect_scan, rows=case.n, cols=2).items():
        assert scan[key] == value, (key, scan)
    sv_dev = torch.from_numpy(case.sv_dev.view(np.int64)).cuda()
    srv.set_concurrency(4)
    srv.stage_batch(np.zeros((3, 1, 2, case.k, case.N), dtype=np.uint64))     # sizes the reply buffers
    db.set_option("upper_parts", 0)
    srv.batch_run_selectors(sv_dev.data_ptr(), 3)
    group = srv.fetch_batch()
    parts = db.get_option("upper_parts")
    print("UPPER_PARTS of the group:", parts)
    assert parts == group_parts
    lone = []
    for m in range(3):
        db.set_option("upper_parts", 0)
        lone.append(db.multiply(case.coeff_sv(m)))
        parts = db.get_option("upper_parts")
        if m == 0:
            print("UPPER_PARTS of a lone vector:", parts)
        assert parts == lone_parts
    db.close()
    for m in range(3):
        assert np.array_equal(group[m], case.expected[m]), ("group", m)
        assert np.array_equal(lone[m], case.expected[m]), ("lone", m)
    print("operands and oracle %.2f s, GPU side %.2f s" % (case.cpu_seconds, time.time() - t0))


INT = dict(ntt_mode=0, f64_lazy_inv=False, pack_bytes=8)
NO_MFMA = dict(mfma=False, digits=0)                       # moduli of 2^55 and more: the 64-bit scans
MFMA_6 = dict(mfma=True, digits=6, chunks=1, single_query_mfma=True)       # 46 / 47 bits: the int8-MFMA scan, 6 digits
MFMA_7 = dict(mfma=True, digits=7, chunks=1, single_query_mfma=True)       # 49 bits


# ---------------------------------------------------------------- the fused integer kernel

@pytest.mark.parametrize("n", [63, 64, 65, 130])
def test_fused_integer_sums_around_the_fold_interval_61_bits(n):
    """int-61: N = 4096, one 61-bit prime, UPPER_BLOCKS = 1 so that one chunk holds the whole row: just below, at and
    above lazy_limit = 64 children, and past two intervals."""
    case = case_of(4096, (61,), False, n, 20, "delta")
    if n > 64:
        case.assert_integer_sums_wrap(64, n)
    run(case, dict(upper_blocks=1), dict(INT, lazy_limit=64), NO_MFMA, 1, 3)


def test_fused_integer_sums_above_the_fold_interval_60_bits():
    """int-60: N = 2048, one 60-bit prime, lazy_limit = 256: 258 children in one chunk (257 products already wrap)."""
    case = case_of(2048, (60,), False, 258, 20, "delta")
    case.assert_integer_sums_wrap(256, 258)
    run(case, dict(upper_blocks=1), dict(INT, lazy_limit=256), NO_MFMA, 1, 3)


def test_fused_integer_chunk_sums_meet_in_reduce_splits():
    """int-61-chunks: the default UPPER_BLOCKS cuts the 130 children into chunks far shorter than the interval (44 chunks
    of 3 for a lone vector: 512 workgroups over 8 chunk slots; 8 chunks of 17 per member of a batch: 64 over 8); the chunk sums,
    each n_c x_e (q - 1) mod q, meet in reduce_splits_kernel.  Same reply bits as int-61."""
    case = case_of(4096, (61,), False, 130, 20, "delta")
    assert case.E == 8
    run(case, {}, dict(INT, lazy_limit=64), NO_MFMA, 44, 3 * 8)


def test_fused_integer_sums_with_two_primes():
    """int-2: k = 2, 65 children in one chunk: chunks of residue 1 are lifted and multiplied under modulus 0 and the
    reverse (enc_res != jt), each of the four (source residue, target modulus) pairs past the interval."""
    case = case_of(4096, (61, 61), False, 65, 20, "delta")
    assert {(j, jt) for _, j, _ in case.layout for jt in range(2)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    case.assert_integer_sums_wrap(64, 65)
    run(case, dict(upper_blocks=1), dict(INT, lazy_limit=64), NO_MFMA, 1, 3)


# ---------------------------------------------------------------- the fused fp64 kernels

F64_46 = dict(ntt_mode=1, f64_lazy_inv=False, lazy_limit=2 ** 30)
F64_WIDE = dict(ntt_mode=2, f64_lazy_inv=False, lazy_limit=2 ** 30)


def fused_fp64(N, bits, low_end, n, kind, arith, scan, mode):
    case = case_of(N, (bits,), low_end, n, 20, kind)
    if kind == "coherent" and n >= 8:
        case.assert_fp64_sums_are_coherent(mode, [n])
    run(case, dict(upper_blocks=1), arith, scan, 1, 1)


@pytest.mark.parametrize("kind", ["coherent", "delta"])
@pytest.mark.parametrize("n", [8, 9, 24, 25])
@pytest.mark.parametrize("low_end", [False, True], ids=["largest prime", "smallest prime"])
def test_fused_fp64_sums_flavour_1(low_end, n, kind):
    """f64-46: N = 4096, one 46-bit prime, upper_fused_kernel<kNttF64> in its default plain-prefetch form, one chunk:
    exactly one normalisation interval, one child more, three intervals (the running sum is largest after the third:
    3.8 q) and one child more."""
    fused_fp64(4096, 46, low_end, n, kind, dict(F64_46, pack_bytes=6), MFMA_6, 1)


@pytest.mark.parametrize("kind", ["coherent", "delta"])
@pytest.mark.parametrize("n", [24, 25])
@pytest.mark.parametrize("bits,low_end", [(49, False), (49, True), (47, False)],
                         ids=["49 bits largest", "49 bits smallest", "47 bits largest"])
def test_fused_fp64_sums_flavour_2(bits, low_end, n, kind):
    """f64-49: N = 8192, one prime at both ends of 49 bits and at the top of 47, upper_fused_kernel<kNttF64Wide>: 3.8 q
    is 2^50.9 here, next to the 2^53 a double holds exactly."""
    fused_fp64(8192, bits, low_end, n, kind, dict(F64_WIDE, pack_bytes=7 if bits == 49 else 6),
               MFMA_7 if bits == 49 else MFMA_6, 2)


def test_fused_fp64_sums_lds_twiddle_form():
    """lds-tw: PIRGPU_UPPER_LDS_TW = 1 is read once per process, so the f64-46 cases with 25 children run again in one
    fresh child process with the LDS-twiddle form of upper_fused_kernel selected."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PIRGPU_UPPER_LDS_TW="1", PIRGPU_ALLOW_ENV="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-k",
                        "test_fused_fp64_sums_flavour_1 and largest and 25"], env=env, capture_output=True, text=True,
                       timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "2 passed" in r.stdout, r.stdout[-2000:]


# ---------------------------------------------------------------- the split form: upper_ntt_kernel + upper_mac_kernel

def blocks_of(n, blk):
    return [blk] * (n // blk) + ([n % blk] if n % blk else [])


@pytest.mark.parametrize("kind", ["coherent", "delta"])
@pytest.mark.parametrize("mb,lone_blk,group_blk", [(3072, 25, 25), (2, 10, 3), (6, 25, 10), (1, 5, 1)],
                         ids=["scratch holds the row", "2 MB", "6 MB", "1 MB"])
def test_split_fp64_sums_carried_between_blocks(mb, lone_blk, group_blk, kind):
    """f64-split: N = 4096, one 46-bit prime, SPLIT_UPPER = 1, 25 children.  A child is 6 chunks x 4096 doubles = 192 KB of
    scratch per query, so SPLIT_UPPER_MB = 2 gives a lone vector blocks of 10 (10 + 10 + 5: not a multiple of the 8 after
    which the sums are normalised, so the count restarts in the middle of an interval and the carry meets a sum of two
    terms) and 6 MB gives a group of 3 the same; 1 MB gives blocks of 5 (of 1 for the group): five carries, though a
    block shorter than 8 children cannot hold eight coherent terms -- the model's 3.6 q is asserted for the blocks of 10
    and of 25."""
    case = case_of(4096, (46,), False, 25, 20, kind)
    assert case.E == 6
    if kind == "coherent":
        for blk in {lone_blk, group_blk}:
            if blk >= 8:
                case.assert_fp64_sums_are_coherent(1, blocks_of(25, blk))
    run(case, dict(split_upper=1, split_upper_mb=mb), dict(F64_46, pack_bytes=6), MFMA_6,
        len(blocks_of(25, lone_blk)), len(blocks_of(25, group_blk)))


@pytest.mark.parametrize("kind", ["coherent", "delta"])
def test_split_fp64_sums_at_16384(kind):
    """f64-split-16k: N = 16384 takes the split form by default; 17 children, 768 KB of scratch each per query: 7 MB
    holds 9 of a lone vector's (two blocks, 9 + 8) and 3 of a group's (six blocks); 21 MB holds 9 of a group's."""
    case = case_of(16384, (46,), False, 17, 20, kind)
    assert case.E == 6
    if kind == "coherent":
        case.assert_fp64_sums_are_coherent(1, [9, 8])
    run(case, dict(split_upper_mb=7), dict(F64_46, pack_bytes=6), MFMA_6, 2, 6)
    run(case, dict(split_upper_mb=21), dict(F64_46, pack_bytes=6), MFMA_6, 1, 2)


# ---------------------------------------------------------------- N = 32768: upper_lift_kernel + upper_mac_int_kernel

@pytest.mark.parametrize("n", [65, 130])
def test_ring32k_integer_sums_above_the_fold_interval(n):
    """ring32k: N = 32768, one 61-bit prime (k = 1 and a 22-bit t: 6 chunks, 1.5 MB of scratch per child and query), once
    with the whole row in one block -- the fold inside upper_mac_int_kernel -- and once with SPLIT_UPPER_MB = 48: blocks of
    32 children, every block's residue carried into the next through add_mod."""
    case = case_of(32768, (61,), False, n, 22, "delta")
    assert case.E == 6
    case.assert_integer_sums_wrap(64, n)
    run(case, {}, dict(INT, lazy_limit=64), NO_MFMA, 1, 3)
    run(case, dict(split_upper_mb=48), dict(INT, lazy_limit=64), NO_MFMA, len(blocks_of(n, 32)), 3 * len(blocks_of(n, 32)))
