"""The shared-selector path of the ciphertext-multiplication mode (option CT_SHARED_SEL, pir_amd/csrc/ctmult_shared.hip,
DESIGN.md section 6.6) driven with chosen operands: on a context whose option is 1 the hooks pirgpu_ct_multiply and
pirgpu_ct_multiply_sum lift and transform the selectors b once -- at B through ctm_lift_polys_kernel<K> and the forward
transform, at Q through the forward transform alone -- and run ctm_tensor_sel_kernel / ctm_tensor_rowsum_sel_kernel.
Whole replies (tests/test_gpu_ctmult_wide.py) reach these kernels at k = 2 and k = 4 with uniform residues and rows of
2 - 4 children only.  Here, bit for bit against the big-integer models of tests/ctmult_model.py and
tests/ctmult_deferred_model.py (every comparison is exact equality of uint64 arrays):

  a. pirgpu_ct_multiply on every rung of M.LADDER -- k = 1, 2, 3, 5, 6, the three transform flavours, N = 2048 ... 16384
     -- on the rung's hook_inputs family: the centring boundary on both sides in the ciphertext half and in the selector
     half of ctm_lift_polys_kernel<K>, all q_j - 1 through ctm_tensor_sel_kernel at both bases; the ladder has no rung at
     k = 4, where the 8192-k4 case of tests/test_gpu_ctmult.py is run instead (whole family, and a row of seven);
  b. pirgpu_ct_multiply_sum on the five rungs of the deferred file, and with n = 1 against pirgpu_ct_multiply;
  c. the lazy fold of ctm_tensor_rowsum_sel_kernel at its limit on 60-bit primes, with distinct selectors (b1 independent
     of b0) on both sides of the first fold and in the remainder segment: one thread per word, split over workgroups, blocks of eight -- and
     once more with operands that would wrap at one modulus alone, which is what makes a late fold visible (on this
     kernel and on its four-polynomial twin);
  d. option 1 against option 0 on mixed prime sizes: the same bits from both hooks;
  e. the option off: four lifts per pair, the ladder's values.

The expected values are the cached cases of tests/test_gpu_ctmult.py, _ladder.py and _deferred.py: in one
session nothing is computed twice.  Every context is a one-dimensional hook context with ct_shared_sel = 1 set before its
first use, and every test reads the option back.

CT_LIFTS round a hook call: 4 per pair in the four-polynomial form, 2 per pair + 2 per selector lifted in the shared
form.  A hook call lifts one selector per pair, so BOTH FORMS COUNT 4 n ON n PAIRS.  The tests assert 4 n (hook_lifts):
that fails a hook that does not count, but NOTHING IN THIS FILE PROVES WHICH PATH RAN -- the bits of the two paths are
equal by construction (test d).  A hook that ignores the option passes this file, which is then a second run of the
sibling files' cases; a counting rule that differs between the forms is needed to close that.  As it stands, what fails it is an error in the shared kernels, their tables or the
hooks' selector plumbing (DESIGN.md section 6.6 lists the mutations tried)."""
import numpy as np
import pytest

import ctmult_deferred_model as D
import ctmult_model as M
import pir_amd
import test_gpu_ctmult as T
import test_gpu_ctmult_deferred as TD
import test_gpu_ctmult_ladder as TL

pytestmark = pytest.mark.gpu

RUNGS = [c[0] for c in M.LADDER]


def hook_lifts(n):
    """CT_LIFTS round a hook call on n pairs.  Four-polynomial form: 4 per pair.  Shared form: the ciphertext half of
    every pair and every selector once, 2 n + 2 n.  The same number: it shows that the hook counted, not which path ran."""
    return 4 * n


def hook_db(N, moduli, t, shared=1, **options):
    """A create_pir_parameters(4, 0, 1, ...) hook context; ct_shared_sel is set before the first use, or left alone."""
    if shared is not None:
        options = dict(options, ct_shared_sel=shared)
    return TD.hook_db(N, moduli, t, **options)


def first_bad(got, want):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    return bad[:1].tolist()


def check_pairs(db, names, A, B, want, lifts):
    """ct_multiply(A, B) == want, pair by pair, with the lifts it must have counted."""
    db.set_option("ct_lifts", 0)
    got = db.ct_multiply(A, B)
    assert db.get_option("ct_lifts") == lifts
    assert got.dtype == want.dtype == np.uint64 and got.shape == want.shape
    for i, name in enumerate(names):
        assert np.array_equal(got[i], want[i]), "%s: first mismatch at [component, residue, coefficient] = %s" % (
            name, first_bad(got[i], want[i]))
    return got


def check_sum(db, A, B, want, lifts, what=""):
    db.set_option("ct_lifts", 0)
    got = db.ct_multiply_sum(A, B)
    assert db.get_option("ct_lifts") == lifts
    assert got.dtype == want.dtype == np.uint64 and got.shape == want.shape
    assert np.array_equal(got, want), "%sfirst mismatch at [component, residue, coefficient] = %s" % (what, first_bad(got, want))
    return got


# ------------------------------------------------------------------------------------------------ a. the ladder, per child

@pytest.mark.parametrize("rung", RUNGS)
def test_rung_per_child(rung):
    """The family of the four-polynomial sibling on every rung (the sub-family where that file runs it: k >= 5 and
    N = 16384), against the same `want`."""
    N, moduli, t, names, A, B, want = TL.ladder_case(rung)[:7]
    assert len(names) == (len(M.SUB_FAMILY) if TL.PATHS[rung][4] else 11)
    assert {"all q_j - 1", "full h", "full h + 1"} <= set(names)
    db, _ = hook_db(N, moduli, t)
    try:
        assert db.get_option("ct_shared_sel") == 1
        assert db.lib.pirgpu_ntt_mode(db.handle) == TL.PATHS[rung][0]
        n = len(names)
        check_pairs(db, names, A, B, want, hook_lifts(n))
        assert db.get_option("ct_shared_sel") == 1
    finally:
        db.close()


# ------------------------------------------------------------------------------------------------ a'. k = 4

_K4 = {}
K4_ROW = ["random 1", "all q_j - 1", "full h", "full h + 1", "delta -1", "delta 0", "delta 1"]


def k4_case():
    """The ladder has no rung at k = 4: the four-polynomial path is pinned there by the 8192-k4 case of
    tests/test_gpu_ctmult.py (N = 8192, [43, 43, 44, 44]-bit data primes, 42-bit t, the whole family), whose cached inputs
    and products are taken as they are.  The row: the pairs K4_ROW of that family, summed (pairs with b1 = b0 or constant
    operands: few big products in the model)."""
    if not _K4:
        N, moduli = 8192, [int(x) for x in T.CHAIN_8192]
        t, names, A, B, want = T.hook_case(N, moduli, 42)[:5]
        q = moduli[:-1]
        assert len(q) == 4 and len(names) == 11
        idx = [names.index(x) for x in K4_ROW]
        assert D.plan_terms(N, q, moduli[-1], t, len(idx))[1]
        row = D.multiply_ct_sum(A[idx], B[idx], q, t)
        row.setflags(write=False)
        _K4["case"] = (N, moduli, t, names, A, B, want, idx, row)
    return _K4["case"]


def test_k4_per_child_and_deferred():
    """ctm_lift_polys_kernel<4> on the centring boundary in both halves, the tensor kernels at k = 4 / kb = 6, the 13-stage
    transform: ct_multiply on the whole family, ct_multiply_sum on a row of seven and on rows of one."""
    N, moduli, t, names, A, B, want, idx, row = k4_case()
    assert {"all q_j - 1", "full h", "full h + 1"} <= set(names)
    db, _ = hook_db(N, moduli, t)
    try:
        assert db.get_option("ct_shared_sel") == 1
        got = check_pairs(db, names, A, B, want, hook_lifts(len(names)))
        check_sum(db, A[idx], B[idx], row, hook_lifts(len(idx)), "the row: ")
        for i in (names.index("random 0"), names.index("full h + 1")):
            check_sum(db, A[i:i + 1], B[i:i + 1], got[i], hook_lifts(1), names[i] + ": ")
    finally:
        db.close()


# ------------------------------------------------------------------------------------------------ b. the ladder, deferred

@pytest.mark.parametrize("rung", TD.SUM_RUNGS)
def test_rung_deferred(rung):
    N, moduli, t, names, A, B, want = TD.sum_case(rung)
    n = A.shape[0]
    db, _ = hook_db(N, moduli, t)
    try:
        assert db.get_option("ct_shared_sel") == 1
        check_sum(db, A, B, want, hook_lifts(n))
        for i in (0, names.index("full h")):                            # a row of one child: the per-child product
            one = db.ct_multiply(A[i:i + 1], B[i:i + 1])[0]
            check_sum(db, A[i:i + 1], B[i:i + 1], one, hook_lifts(1), names[i] + ": ")
    finally:
        db.close()


# ------------------------------------------------------------------------------------------------ c. the lazy fold

_FOLD = {}
FOLD_CONFIGS = pytest.mark.parametrize("options", [{"ct_scratch_mb": 1024, "ct_rowsum_splits": 1}, {}, {"ct_scratch_mb": 1}],
                                       ids=["one-thread-per-word", "split-over-workgroups", "blocks-of-eight"])


def independent_pair(q, N, rng):
    """TD.random_pair with b0 and b1 drawn independently: the two selector polynomials swapped, or one of them read at a
    wrong offset, changes the tensor."""
    A, B = TD.random_pair(q, N, rng)
    for j, qj in enumerate(q):
        B[1, j, :] = rng.integers(0, qj, size=N, dtype=np.uint64)
    return A, B


def fold_case(kind):
    """k6-int.  lazy / 2 + 2 children are one constant pair c (all four polynomials the same constant); four distinct
    random pairs (b1 independent of b0) sit at the children 0, lazy / 2 - 1, lazy / 2 and the last: with a fold every lazy / 2 children, one on
    each side of the first fold and one in the remainder segment, so that a selector read at a wrong offset after a fold
    changes the sum.  X = n_const tensor(c, c) + the tensors of the four (computed once for both kinds).

    "all":  c = -1, residue q_j - 1 at every prime.  Its NTT form is q - 1 in every slot at Q and b_i - 1 at B: every dyadic
            product is the maximal (q - 1)^2, x1 takes two per child, and tensor(c, c) = (1, 2, 1).
    "one":  c = the constant with residue q_0 - 1 at the first prime and 1 at the others.  Maximal products at q_0 alone."""
    if kind not in _FOLD:
        N, moduli, t = TD.rung_chain("k6-int")
        q = moduli[:-1]
        lazy = 1 << (128 - 2 * 60)
        n_const = lazy // 2 + 2
        n = n_const + 4
        at = [0, lazy // 2 - 1, lazy // 2, n - 1]
        assert (lazy + 4) * (min(q) - 1) ** 2 >= 1 << 128          # x1 of the constant children alone wraps unfolded
        assert D.plan_terms(N, q, moduli[-1], t, n)[1]
        if "four" not in _FOLD:
            rng = np.random.default_rng(6060)
            four = [independent_pair(q, N, rng) for _ in at]
            Af, Bf = np.stack([f[0] for f in four]), np.stack([f[1] for f in four])
            assert len({b.tobytes() for b in Bf}) == 4 and not any(np.array_equal(b[0], b[1]) for b in Bf)
            _FOLD["four"] = (Af, Bf, D.tensor_sum(Af, Bf, q))
        Af, Bf, Xf = _FOLD["four"]
        c = np.zeros((2, len(q), N), dtype=np.uint64)
        for j, qj in enumerate(q):
            c[:, j, 0] = qj - 1 if kind == "all" or j == 0 else 1
        xc = M.tensor(c, c, q)
        assert not any(any(x[1:]) for x in xc)                      # constants
        if kind == "all":
            assert [x[0] for x in xc] == [1, 2, 1]
        A, B = np.stack([c] * n), np.stack([c] * n)
        for i, j in enumerate(at):
            A[j], B[j] = Af[i], Bf[i]
        assert sum(np.array_equal(B[j], c) for j in range(n)) == n_const
        X = [list(x) for x in Xf]
        for m in range(3):
            X[m][0] += n_const * xc[m][0]
        want = M.scaled_residues(X, q, t)
        for x in (A, B, want):
            x.setflags(write=False)
        _FOLD[kind] = (N, moduli, t, lazy, A, B, want)
    return _FOLD[kind]


def run_fold(kind, options, shared=1):
    N, moduli, t, lazy, A, B, want = fold_case(kind)
    db, pp = hook_db(N, moduli, t, shared=shared, **options)
    try:
        assert db.get_option("ct_shared_sel") == shared
        assert pir_amd.PIRServer(db, pp).arith_info()["lazy_limit"] == lazy == 256
        n = A.shape[0]
        assert n == lazy // 2 + 6
        check_sum(db, A, B, want, hook_lifts(n), "%s: " % (options,))
    finally:
        db.close()


@FOLD_CONFIGS
def test_lazy_fold_of_the_shared_row_sum_at_its_limit(options):
    """134 children at N = 4096, k = 6, the constant -1 ("all").  One thread per word: the row in one block, a fold inside
    the loop and the selector pointer recomputed behind it.  The defaults: three blocks, the children of each shared out
    over workgroups.  ct_scratch_mb = 1: blocks of eight with the accumulator carried, where the selector offset
    lo - first differs from the block offset lo - j0 in every block after the first.

    What these operands do NOT show is a fold that comes too late.  An unfolded x1 wraps at EVERY modulus of Q and of B
    alike, each losing 2^128 once: the residues then are those of the integer X1 - 2^128, which the 14 moduli hold
    exactly, and t 2^128 / Q is about 2^-173 at six 60-bit primes -- the rounded result keeps its bits (seen on an
    MI355X with `per` taken as lazy_limit: this test passed).  The next test is there for that."""
    run_fold("all", options)


@pytest.mark.parametrize("shared", [1, 0], ids=["shared", "four-polynomial"])
def test_lazy_fold_when_one_modulus_alone_would_wrap(shared):
    """The same row with the constant that is -1 at the first prime and 1 at the others ("one"): an unfolded x1 wraps at
    q_0 -- (lazy + 4)(q_0 - 1)^2 >= 2^128, asserted with the case -- and at no other prime of Q, where the 268 products of
    the constant children are 1 and the rest below 2^120 each.  The residues of a late fold are then those of no integer
    near X1, and the result differs.  One thread per word, on the shared-selector kernel and on its twin
    ctm_tensor_rowsum_kernel (the four-polynomial path), whose own test uses the operands of "all"."""
    run_fold("one", {"ct_scratch_mb": 1024, "ct_rowsum_splits": 1}, shared)


# ------------------------------------------------------------------------------------------------ d. both paths, same bits

def test_both_paths_give_the_same_bits_on_mixed_primes():
    """k3-mixed ([30, 36, 40]-bit primes, 40-bit auxiliary primes): the whole family on a context with the option 0 and on
    one with the option 1, as pairs and as one row."""
    N, moduli, t, names, A, B, want = TL.ladder_case("k3-mixed")[:7]
    n = len(names)
    assert D.plan_terms(N, moduli[:-1], moduli[-1], t, n)[1]
    out = {}
    for shared in (0, 1):
        db, _ = hook_db(N, moduli, t, shared=shared)
        try:
            assert db.get_option("ct_shared_sel") == shared
            db.set_option("ct_lifts", 0)
            pairs = db.ct_multiply(A, B)
            assert db.get_option("ct_lifts") == (hook_lifts(n))
            db.set_option("ct_lifts", 0)
            row = db.ct_multiply_sum(A, B)
            assert db.get_option("ct_lifts") == (hook_lifts(n))
            out[shared] = (pairs, row)
        finally:
            db.close()
    assert out[0][0].dtype == out[0][1].dtype == np.uint64
    for i, name in enumerate(names):
        assert np.array_equal(out[1][0][i], out[0][0][i]), "%s: first mismatch at %s" % (name, first_bad(out[1][0][i], out[0][0][i]))
    assert np.array_equal(out[1][1], out[0][1]), "the row: first mismatch at %s" % first_bad(out[1][1], out[0][1])
    assert np.array_equal(out[1][0], want)


# ------------------------------------------------------------------------------------------------ e. the option off

def test_option_off_is_untouched():
    """A default hook context: the option reads 0, every pair lifts its four polynomials, the products are the ladder's
    and the row the deferred file's."""
    N, moduli, t, names, A, B, want = TL.ladder_case("k3-mixed")[:7]
    db, _ = hook_db(N, moduli, t, shared=None)
    try:
        assert db.get_option("ct_shared_sel") == 0
        check_pairs(db, names, A, B, want, hook_lifts(len(names)))
        _, _, _, _, As, Bs, row = TD.sum_case("k3-mixed")
        check_sum(db, As, Bs, row, hook_lifts(As.shape[0]))
        assert db.get_option("ct_shared_sel") == 0
    finally:
        db.close()
