"""CPU model of the deferred rounding of the ciphertext-multiplication mode (PIRGPU_CREATE_CT_DEFERRED, DESIGN.md section
6.6) -- TEST INFRASTRUCTURE ONLY.  Everything that is not restated here is tests/ctmult_model.py.

For a row of an upper level whose existing children are i in C, with (x0, x1, x2)_i = M.tensor(child_i, sel_i, q):

    X_m = sum over i in C of x_m,i          over the integers
    D_m = floor((t X_m + h) / Q)            M.scaled_residues: ONE rounding per row
    row = M.relinearize(orc, D, rk)         ONE key switch per row

against one rounding and one key switch per child in M.levels_ct.  Row sums (scan + inverse transform), d = 1, the
transparent-ciphertext rule and process_response_ct are those of ctmult_model.  `plan_terms` restates
pirgpu_ctmult_plan_terms: a sum of n products has to fit the auxiliary base."""
import numpy as np

import ctmult_model as M


def tensor_sum(As, Bs, q):
    """As, Bs [n][2][k][N] -> (X0, X1, X2): the sum of the n tensor products, integer lists."""
    X = None
    for A, B in zip(As, Bs):
        x = M.tensor(A, B, q)
        X = x if X is None else tuple([u + v for u, v in zip(Xm, xm)] for Xm, xm in zip(X, x))
    return X


def multiply_ct_sum(As, Bs, q, t):
    """pirgpu_ct_multiply_sum: [n][2][k][N] x [n][2][k][N] -> [3][k][N] canonical residues of (D0, D1, D2) of the sum."""
    return M.scaled_residues(tensor_sum(As, Bs, q), q, t)


def bounds_hold(N, q, aux, t, terms):
    """The two inequalities of the plan for a sum of up to `terms` products, in Python integers."""
    Q, Bp = M.prod(q), M.prod(aux)
    return Q * Bp > t * terms * N * (Q - 1) ** 2 + 2 * Q and Bp > 2 * (t * terms * N * Q + 2)


def plan_terms(N, q, special, t, terms):
    """pirgpu_ctmult_plan_terms restated: (aux primes, ok)."""
    aux, _ = M.plan(N, q, special, t)
    return aux, len(aux) == len(q) + 2 and bounds_hold(N, q, aux, t, terms)


def levels_ct_deferred(orc, db_ntt, dims, sv, rk):
    """M.levels_ct with the rounding deferred across the children of a row -> (rc, [2][k][N] or None)."""
    dims = list(dims)
    d = len(dims)
    off = [sum(dims[:l]) for l in range(d)]
    cols = dims[-1]
    P = db_ntt.shape[0]
    q = orc.moduli[:orc.k]
    lower = []
    for r in range((P + cols - 1) // cols):
        part = np.ascontiguousarray(db_ntt[r * cols:(r + 1) * cols])
        sel = np.ascontiguousarray(sv[off[-1]:off[-1] + part.shape[0]]).copy()
        rc, out = orc.db_multiply(part, [part.shape[0]], sel)
        if rc != 0:
            return rc, None
        lower.append(out[0])
    for l in range(d - 2, -1, -1):
        upper = []
        for r in range((len(lower) + dims[l] - 1) // dims[l]):
            kids = lower[r * dims[l]:(r + 1) * dims[l]]
            D = multiply_ct_sum(kids, [sv[off[l] + i] for i in range(len(kids))], q, orc.t)
            upper.append(M.relinearize(orc, D, rk))
        lower = upper
    assert len(lower) == 1
    return 0, lower[0]


def process_query_ct_deferred(orc, db_ntt, dims, query_cts, galois_keys, rk):
    """processQuery with deferred rounding -> (rc, reply [1][2][k][N])."""
    rc, sv = orc.oblivious_expansion_multi(query_cts, sum(dims), galois_keys)
    if rc != 0:
        return rc, None
    rc, out = levels_ct_deferred(orc, db_ntt, dims, sv, rk)
    return rc, None if out is None else out[None]
