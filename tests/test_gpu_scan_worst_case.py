"""The database scan at COHERENT worst-case operands: every digit product of a row sum has the same sign, so the int32
diagonals, the 40-bit groups and the fp64 chunks of scan_mfma.hip -- and the lazy 64-bit sums of kernels.hip -- reach the
budgets their comments state instead of the square root of them that random data leaves (tests/scan_fold_model.py,
tests/test_scan_fold_model.py: the same operands on a CPU model of the fold).

How the operands get there through the public interface:

  database   a constant plaintext c = x mod t with |x| < t / 2 lifts to the centred residue x in every NTT slot of every
             data prime (t is taken one bit above the primes: the create call wants t < 2^60, not t < q), loaded with
             populate_coeffs; one tile of the operand layout is read back and compared digit by digit
  selectors  NTT-form residues handed to batch_run_selectors (groups of 3) and, as the constant polynomials they are
             the transform of, to PIRDatabase.multiply (a lone selection vector)

N = 4096, d = 2, 9 rows x one chunk at the kernel's widest (448 columns, 384 at L = 7), two data primes of one size: the
smallest and the largest NTT-friendly primes of 36 / 39 / 44 / 47 / 50 / 55 bits.  Rows 0-3 hold the four members of the
family (low digits all -128 or all +127, top digit at either end of the centring) in every column, rows 4-8 mix members
column by column so that the sign of the product with the mixed selectors 4 and 5 is still the same in every column;
selectors 0-3 are the four members, 4 and 5 the mixed ones.  Before anything runs on the GPU the diagonals T of every
coherent (row, selector) pair are computed from the operands and required to be at least 0.99 of the model's maximum
over the family for that kernel variant and that pairing of signs (a pair of +127 digits cannot give more than
127^2 / 128^2 = 0.984 of what a pair of -128 gives, so the maximum is taken per pairing; the launch as a whole
reaches the variant's overall maximum).

Every reply is compared with the oracle's db_multiply and with the 64-bit scan's (SCAN_MFMA = 0); the path taken is
asserted through arith_info and scan_info."""
import functools

import numpy as np
import pytest

import oracle
import pir_amd
import scan_fold_model as M
from gpu_helpers import chain, chain_low, device_to_seal_order, to_product_params

pytestmark = pytest.mark.gpu

N = 4096
ROWS = 9
NSEL = 6
# (bits, digits, nibble top digit by default)
SIZES = [(36, 5, True), (39, 5, False), (44, 6, True), (47, 6, False), (50, 7, False), (55, 7, False)]
WIDEST = {5: 7, 6: 7, 7: 6}          # k-steps of the widest chunk (4-wave kernel)
NARROW = {5: 3, 6: 3, 7: 2}          # ... of the 8-wave kernel


def sigma(c):
    """The sign pattern of the mixed operands over the columns: + + + - - -.  Half the products of a positive row sum are
    then 127 * 127 and half 128 * 128 (0.992 of the all -128 maximum), and no prefix of the columns holds -128 and +127
    digits in the ratio 127 : 128 at which a sum of members can vanish (255 columns: 129 against 126) -- the reference
    refuses a running sum that is identically zero ("result ciphertext is transparent"), and so does the oracle."""
    return 1 if c % 6 < 3 else -1


class Case:
    """Parameters, oracle, operands and expected replies of one (modulus size, end of the size, top-digit form, columns)."""

    def __init__(self, bits, L, low_end, top4, cols):
        self.bits, self.L, self.top4, self.cols = bits, L, top4, cols
        moduli = (chain_low if low_end else chain)(N, bits)
        self.qs = [int(q) for q in moduli[:2]]
        t = oracle.plain_modulus_batching(N, bits + 1)
        p = oracle.create_pir_parameters(ROWS * cols, 0, 2, N=N, moduli=moduli, t=t)
        assert p.num_pt == ROWS * cols
        p.dimensions = [ROWS, cols]
        self.params, self.t = p, t
        self.orc = oracle.Oracle.from_params(p)
        # the family of the smaller prime: its centred range lies inside the other's, so both primes see the same digits
        fam = M.family(min(self.qs), L, top4)
        self.members = [v for _, v in fam]                      # (low -128, top min), (-128, max), (+127, min), (+127, max)
        for v in self.members:
            assert 2 * abs(v) < t
            d = [M.to_digits(v % q, q, L, top4) for q in self.qs]
            assert d[0] == d[1] and d[0][1] == 0, (v, d)
        # member index = 2 * (low digits +127) + (top digit at its upper end); database [row][col], selectors [query][col]
        pick = lambda sign, c: (0 if sign < 0 else 2) + (c & 1)
        self.Xi = [[r] * cols for r in range(4)]
        for r in range(4, ROWS):
            rho = 1 if r & 1 else -1
            self.Xi.append([pick(rho * sigma(c), c + r) for c in range(cols)])
        self.Si = [[i] * cols for i in range(4)]
        self.Si.append([pick(sigma(c), c) for c in range(cols)])
        self.Si.append([pick(-sigma(c), c + 1) for c in range(cols)])
        self.X = [[self.members[m] for m in row] for row in self.Xi]       # centred values
        self.S = [[self.members[m] for m in row] for row in self.Si]
        self.coherent = [(r, i) for r in range(4) for i in range(4)] + [(r, i) for r in range(4, ROWS) for i in (4, 5)]
        # what the database load and the oracle are given
        self.coeff_rows = [np.array([x % t], dtype=np.uint64) for row in self.X for x in row]
        k = 2
        self.db_ntt = np.empty((ROWS * cols, k, N), dtype=np.uint64)
        flat = [x for row in self.X for x in row]
        for j, q in enumerate(self.qs):
            self.db_ntt[:, j, :] = np.array([x % q for x in flat], dtype=np.uint64)[:, None]
        for v in self.members:                                   # the lift really gives the constant x mod q_j
            lifted = self.orc.db_from_coeffs([np.array([v % t], dtype=np.uint64)])[0]
            for j, q in enumerate(self.qs):
                assert (lifted[j] == v % q).all(), (v, j)
        # selection vectors, NTT form, device order: random upper-level selectors (every row sum reaches the reply), the
        # scan selectors constant over the slots
        rng = np.random.default_rng(bits * 1000 + cols + low_end)
        self.sv = np.empty((NSEL, ROWS + cols, 2, k, N), dtype=np.uint64)
        for j, q in enumerate(self.qs):
            self.sv[:, :ROWS, :, j, :] = rng.integers(0, q, size=(NSEL, ROWS, 2, N), dtype=np.uint64)
            for i in range(NSEL):
                self.sv[i, ROWS:, :, j, :] = np.array([s % q for s in self.S[i]], dtype=np.uint64)[:, None, None]
        self.upper_coeff, self.expected = [], []
        for i in range(NSEL):
            seal = self.sv[i].copy()
            seal[:ROWS] = device_to_seal_order(self.sv[i, :ROWS])
            self.upper_coeff.append(np.stack([self.orc.ct_ntt_inv(seal[r]) for r in range(ROWS)]))
            rc, exp = self.orc.db_multiply(self.db_ntt, p.dimensions, seal, sv_is_ntt=np.ones(ROWS + cols, np.uint8))
            assert rc == 0 and exp.any()
            self.expected.append(exp)
        self.valu = None                                         # replies of the 64-bit scan, once

    def coeff_sv(self, i):
        """Selection vector i in coefficient form (what PIRDatabase.multiply takes)."""
        sv = np.zeros((ROWS + self.cols, 2, 2, N), dtype=np.uint64)
        sv[:ROWS] = self.upper_coeff[i]
        for j, q in enumerate(self.qs):
            sv[ROWS:, :, j, 0] = np.array([s % q for s in self.S[i]], dtype=np.uint64)[:, None]
        return sv

    # ---- the model's side: how hard the operands are
    def diagonals(self, r, i, c0, c1):
        """max_s |T[s]| of row r with selector i over the columns [c0, c1) (one chunk)."""
        q, L = min(self.qs), self.L
        count = {}
        for c in range(c0, c1):
            count[(self.X[r][c], self.S[i][c])] = count.get((self.X[r][c], self.S[i][c]), 0) + 1
        T = [0] * (2 * L - 1)
        for (x, s), n in count.items():
            P, _ = M.diagonals([M.to_digits(x % q, q, L, self.top4)[0]], [M.to_digits(s % q, q, L, self.top4)[0]])
            T = [a + n * b for a, b in zip(T, P)]
        return max(abs(v) for v in T)

    def family_maximum(self, ncols):
        """{(sign of the database's low digits, of the selector's): max |T|} over the family, `ncols` columns."""
        q, L = min(self.qs), self.L
        out = {}
        for a, x in enumerate(self.members):
            for b, s in enumerate(self.members):
                P, _ = M.diagonals([M.to_digits(x % q, q, L, self.top4)[0]], [M.to_digits(s % q, q, L, self.top4)[0]])
                key = (a >> 1, b >> 1)
                out[key] = max(out.get(key, 0), ncols * max(abs(v) for v in P))
        return out

    def assert_operands_are_worst_case(self, chunks):
        per_chunk = self.cols // chunks
        ref = self.family_maximum(per_chunk)
        overall = 0
        for ch in range(chunks):
            for r, i in self.coherent:
                got = self.diagonals(r, i, ch * per_chunk, (ch + 1) * per_chunk)
                if r < 4:
                    want = ref[(r >> 1, i >> 1)]
                else:   # mixed: the sign of the product is fixed, the pairing alternates between the two with that sign
                    same = (self.Xi[r][0] >> 1) == (self.Si[i][0] >> 1)
                    want = max(ref[(0, 0)], ref[(1, 1)]) if same else max(ref[(0, 1)], ref[(1, 0)])
                assert got >= 0.99 * want, (r, i, ch, got, want)
                overall = max(overall, got)
        assert overall >= 0.99 * max(ref.values()) and max(ref.values()) >= 0.99 * (self.L - 1) * 2 ** 14 * per_chunk

    def assert_stored_digits(self, db, nibble, info):
        """Tile (row tile 0, column group 0) of slot 0 of each prime in the operand layout holds the intended digits."""
        L = self.L
        TB = (L - 1) * 256 + 128 if nibble else L * 256
        KG = (self.cols + 15) // 16
        for j in (0, N):
            tile = db.read_operand(j * KG * TB, TB)
            for r in range(16):
                for c in range(16):
                    d = [int(tile[a * 256 + r * 16 + c].view(np.int8)) for a in range(L - 1 if nibble else L)]
                    if nibble:
                        byte = int(tile[(L - 1) * 256 + r * 8 + (c >> 3) * 4 + (c & 3)])
                        nib = byte >> 4 if c & 4 else byte & 0xF
                        d.append(nib - 16 if nib >= 8 else nib)
                    want = M.to_digits(self.X[r][c] % self.qs[0], self.qs[0], L, nibble)[0] if r < ROWS else [0] * L
                    assert d == want, (j, r, c, d, want)


@functools.lru_cache(maxsize=1)
def case_of(bits, L, low_end, top4, cols):
    return Case(bits, L, low_end, top4, cols)


def context(case, **options):
    pp = to_product_params(case.params)
    db = pir_amd.PIRDatabase.Create(pp)
    for name, value in options.items():
        db.set_option(name, value)
    db.populate_coeffs(case.coeff_rows)
    return db, pir_amd.PIRServer(db, pp)


def replies_of(case, db, srv, sv_dev):
    """[NSEL] replies from two group launches of 3 and [NSEL] from lone selection vectors."""
    srv.set_concurrency(8)
    groups = []
    for g in range(NSEL // 3):
        srv.stage_batch(np.zeros((3, 1, 2, 2, N), dtype=np.uint64))     # sizes the reply buffers
        srv.batch_run_selectors(sv_dev[3 * g:3 * g + 3].data_ptr(), 3)
        groups.extend(srv.fetch_batch())
    lone = [db.multiply(case.coeff_sv(i)) for i in range(NSEL)]
    return groups, lone


def device_selectors(case):
    import torch
    return torch.from_numpy(case.sv.view(np.int64)).cuda()


def valu_replies(case, sv_dev):
    if case.valu is None:
        db, srv = context(case, scan_mfma=0)
        assert not srv.scan_info()["mfma"]
        case.valu = replies_of(case, db, srv, sv_dev)
        db.close()
    return case.valu


def check(case, options, chunks, ksteps, folds):
    """One context with `options`: its path, its stored digits, its replies."""
    allow = all(q < 2 ** 50 for q in case.qs)
    nibble = case.top4
    case.assert_operands_are_worst_case(chunks)
    sv_dev = device_selectors(case)
    db, srv = context(case, scan_mfma_top4=1 if nibble else 0, **options)
    info, a = srv.scan_info(), srv.arith_info()
    assert info["mfma"] and info["digits"] == case.L and info["chunks"] == chunks and info["ksteps"] == ksteps, info
    assert info["top_digit_nibble"] == nibble and info["single_query_mfma"] and info["rows"] == ROWS, info
    if folds is None:      # the defaults: the lone vector folds in fp64 from 6 digits, a group whenever the moduli allow
        folds = (1 if case.L >= 6 else 0, 1)
    assert a["scan_f64_fold"] == bool(folds[0] and allow) and a["scan_f64_fold_batch"] == bool(folds[1] and allow), a
    db.finalize()
    case.assert_stored_digits(db, nibble, info)
    groups, lone = replies_of(case, db, srv, sv_dev)
    db.close()
    valu = valu_replies(case, sv_dev)
    for i in range(NSEL):
        assert np.array_equal(groups[i], case.expected[i]), ("group", i)
        assert np.array_equal(lone[i], case.expected[i]), ("lone", i)
        assert np.array_equal(valu[0][i], case.expected[i]) and np.array_equal(valu[1][i], case.expected[i]), ("64-bit", i)


def _cases(eight_wave):
    out = []
    for bits, L, nibble in SIZES:
        for low_end in (True, False):
            # the byte form forced on moduli that take the nibble by default: the widest chunk only (it is the 39- / 47-bit
            # rung's kernel at a smaller top digit)
            for top4 in ([True] + ([] if eight_wave else [False]) if nibble else [False]):
                allow = bits <= 50
                if eight_wave:
                    fold_sets = [(0, 0), (1, 1)] if allow else [(0, 0)]
                else:
                    fold_sets = [None, (0, 0), (0, 1), (1, 0), (1, 1)] if allow else [None, (1, 1)]
                for folds in fold_sets:
                    name = "%d bits %s primes, %s top digit, %s" % (
                        bits, "smallest" if low_end else "largest", "nibble" if top4 else "byte",
                        "default folds" if folds is None else "fold %d batch %d" % folds)
                    out.append(pytest.param(bits, L, low_end, top4, folds, id=name))
    return out


@pytest.mark.parametrize("bits,L,low_end,top4,folds", _cases(False))
def test_widest_chunk_at_coherent_extremes(bits, L, low_end, top4, folds):
    """The 4-wave kernel over its widest chunk.  The lone vector runs the fold SCAN_F64_FOLD names, the groups the fp64
    fold when either option is on (scan_group_mfma); the integer fold of 6 digits over 7 k-steps with the smallest
    primes is the case that returned wrong residues while the bias was 2^57 <= bias < 2^58."""
    case = case_of(bits, L, low_end, top4, 64 * WIDEST[L])
    options = {} if folds is None else dict(scan_f64_fold=folds[0], scan_f64_fold_batch=folds[1])
    check(case, options, 1, WIDEST[L], folds)


@pytest.mark.parametrize("bits,L,low_end,top4,folds", _cases(True))
def test_two_chunks_of_the_eight_wave_kernel_at_coherent_extremes(bits, L, low_end, top4, folds):
    """The 8-wave kernel forced, two column chunks of its widest: reduce_splits_kernel adds two partial sums that are
    each at their extreme."""
    case = case_of(bits, L, low_end, top4, 2 * 64 * NARROW[L])
    check(case, dict(scan_mfma_wide=0, scan_mfma_single=1, scan_f64_fold=folds[0], scan_f64_fold_batch=folds[1]), 2,
          NARROW[L], folds)


# ---------------------------------------------------------------- the 64-bit scans (kernels.hip: AccLimb, AccWide)

def limb_case(bits, low_end, dims):
    """One data prime; every plaintext the constant residue `a`, every scan selector (b0, b1) constant over the slots."""
    moduli = (chain_low if low_end else chain)(N, [bits])
    q = int(moduli[0])
    t = oracle.plain_modulus_batching(N, 32)
    p = oracle.create_pir_parameters(int(np.prod(dims)), 0, len(dims), N=N, moduli=moduli, t=t)
    p.dimensions = list(dims)
    return p, oracle.Oracle.from_params(p), q, t


def run_64bit(bits, low_end, dims, options, expect_limb, counts):
    """Database residues and selectors from {q - 1, the residue with both 28-bit limbs largest}, in every column; single
    selection vectors and groups; against the oracle and, at d = 1, against cols * a * b mod q."""
    import torch
    p, orc, q, t = limb_case(bits, low_end, dims)
    cols, rows = dims[-1], int(np.prod(dims[:-1]))
    upper = sum(dims[:-1])
    extremes = [q - 1, M.limb_max(q)]
    rng = np.random.default_rng(bits + cols)
    for a in extremes:
        x = a - q                                                  # centred: |x| < 2^29 < t / 2
        assert 2 * abs(x) < t
        coeff = [np.array([x % t], dtype=np.uint64)] * (rows * cols)
        db_ntt = np.full((rows * cols, 1, N), a, dtype=np.uint64)
        assert np.array_equal(orc.db_from_coeffs(coeff[:1])[0], db_ntt[0])
        nsel = max(counts)
        sv = np.empty((nsel, upper + cols, 2, 1, N), dtype=np.uint64)
        sv[:, :upper] = rng.integers(0, q, size=(nsel, upper, 2, 1, N), dtype=np.uint64)
        pairs = [(extremes[i & 1], extremes[(i >> 1) & 1]) for i in range(nsel)]
        if len(dims) > 1 and a == q - 1:
            # (q - 1)^2 * cols = cols: the upper half of so small a row sum re-encodes to a zero plaintext, which the
            # reference refuses as transparent; q - 1 meets q - 1 at d = 1
            pairs = [(extremes[1], extremes[1])] * nsel
        for i, (b0, b1) in enumerate(pairs):
            sv[i, upper:, 0], sv[i, upper:, 1] = b0, b1
        expected = []
        for i in range(nsel):
            seal = sv[i].copy()
            seal[:upper] = device_to_seal_order(sv[i, :upper])
            rc, exp = orc.db_multiply(db_ntt, p.dimensions, seal, sv_is_ntt=np.ones(upper + cols, np.uint8))
            assert rc == 0
            if len(dims) == 1:                                     # the reply is the row sum in coefficient form: a constant
                for comp in range(2):
                    assert exp[0, comp, 0, 0] == cols * a * pairs[i][comp] % q and not exp[0, comp, 0, 1:].any()
            expected.append(exp)
        pp = to_product_params(p)
        db = pir_amd.PIRDatabase.Create(pp)
        for name, value in options.items():
            db.set_option(name, value)
        db.populate_coeffs(coeff)
        srv = pir_amd.PIRServer(db, pp)
        info, arith = srv.scan_info(), srv.arith_info()
        assert not info["mfma"] and info["rows"] == rows and info["cols"] == cols, info
        assert arith["scan_limb"] == expect_limb and arith["lazy_limit"] == M.lazy_limit(bits), arith
        sv_dev = torch.from_numpy(sv.view(np.int64)).cuda()
        srv.set_concurrency(4)
        for count in counts:
            srv.stage_batch(np.zeros((count, 1, 2, 1, N), dtype=np.uint64))
            srv.batch_run_selectors(sv_dev.data_ptr(), count)
            got = srv.fetch_batch()
            for i in range(count):
                assert np.array_equal(got[i], expected[i]), (a, cols, count, i)
        # a lone selection vector, in coefficient form: the scan selectors are constant polynomials
        for i in (0, nsel - 1):
            c = np.zeros((upper + cols, 2, 1, N), dtype=np.uint64)
            seal = device_to_seal_order(sv[i, :upper])
            for r in range(upper):
                c[r] = orc.ct_ntt_inv(seal[r])
            c[upper:, 0, 0, 0], c[upper:, 1, 0, 0] = pairs[i]
            assert np.array_equal(db.multiply(c), expected[i]), (a, cols, "lone", i)
        db.close()


# (bits, limb accumulators, fold interval): 28-bit limbs below 2^50 (kLimbLazy = 128 terms), 128-bit sums from 2^50 on
# (lazy_limit = 2^(128 - 2 bits) terms: 64 at 61 bits; at 51 bits the interval is out of reach and only the choice is pinned)
LIMB_RUNGS = [(50, True, 128), (51, False, None), (61, False, 64)]


@pytest.mark.parametrize("low_end", [True, False], ids=["smallest prime", "largest prime"])
@pytest.mark.parametrize("bits,limb,interval", LIMB_RUNGS)
@pytest.mark.parametrize("kernel", ["scan_kernel", "scan_mq_kernel"])
def test_64bit_scan_at_d1_around_the_fold_interval(kernel, bits, limb, interval, low_end):
    """d = 1, all columns in one split (SCAN_NSPLIT = 1), just below, at and above the interval after which the lazy sums
    are folded, and past two intervals.  A lone selection vector and a batch of one take scan_kernel (SCAN_MQ_SINGLE = 0)
    or scan_mq_kernel with 128-bit sums; batches of 3 and 4 share passes of scan_mq_kernel (groups of 2 and 4) with the
    accumulators the moduli select."""
    options = dict(scan_nsplit=1, scan_mq_single=0 if kernel == "scan_kernel" else 1)
    for cols in ([interval - 1, interval, interval + 1, 2 * interval + 1] if interval else [129]):
        run_64bit(bits, low_end, [cols], options, limb, [1, 3, 4])


@pytest.mark.parametrize("bits,limb,interval", LIMB_RUNGS)
def test_64bit_scan_with_few_rows_at_d2(bits, limb, interval):
    """d = 2 with 4 rows (fewer than the 8 the MFMA scan wants): scan_mq_kernel over whole rows."""
    for cols in ([interval, interval + 1] if interval else [129]):
        run_64bit(bits, False, [4, cols], dict(scan_nsplit=1), limb, [1, 4])
