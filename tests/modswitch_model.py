"""CPU model of modulus-switched results (pirgpu_params.result_primes), in Python integers.

One drop step, on canonical residues x_i in [0, q_i) of the current primes q_0..q_m, with h = floor(q_m / 2):

    a = (x_m + h) mod q_m
    x_i' = (x_i - (a mod q_i) + (h mod q_i)) * q_m^-1 mod q_i          (i < m)

which is floor((x + h) / q_m) mod q_0...q_{m-1} on the CRT representative x in [0, q_0...q_m) -- the project's reading of
SEAL 3.5.6 Evaluator::mod_switch_to_next_inplace for BFV (divide_and_round_q_last_inplace); not verified against a SEAL
build.  Switching from k to r primes is k - r such steps, last prime first.

The module states the step twice (on residues: `drop_step` / `switch_residues`; on CRT-composed integers: `switch_crt`),
composes a switched PIRDatabase::multiply out of the oracle's own pieces (`multiply_switched`,
`process_query_switched`) and decrypts at a prefix level with the oracle client's secret key (`decrypt_level`,
`noise_budget_level`, `process_reply_level`).  Arrays of Python integers (dtype=object) keep every product exact."""
import math

import numpy as np


def _obj(a):
    return np.asarray(a).astype(object)


# ---------------------------------------------------------------------------------------------------- the drop step

def drop_step(x, q):
    """x: residues [m + 1, ...] (any trailing shape) of the primes q[0..m] -> residues [m, ...] of q[0..m-1]."""
    q = [int(v) for v in q]
    m = len(q) - 1
    x = _obj(x)
    assert x.shape[0] == m + 1 and m >= 1
    qm = q[m]
    h = qm // 2
    a = (x[m] + h) % qm
    out = np.empty((m,) + x.shape[1:], dtype=object)
    for i in range(m):
        inv = pow(qm % q[i], -1, q[i])
        out[i] = ((x[i] - (a % q[i]) + (h % q[i])) * inv) % q[i]
    return out


def switch_residues(cts, q, r):
    """cts [..., k, N] uint64 over the data primes q[0..k-1] -> [..., r, N] uint64: k - r drop steps, last prime first."""
    cts = np.asarray(cts)
    k = cts.shape[-2]
    q = [int(v) for v in q[:k]]
    assert 1 <= r <= k
    x = np.moveaxis(_obj(cts), -2, 0)
    for m in range(k - 1, r - 1, -1):
        x = drop_step(x, q[:m + 1])
    return np.ascontiguousarray(np.moveaxis(x, 0, -2).astype(np.uint64))


def crt_compose(x, q):
    """residues [n, ...] of q[0..n-1] -> integers in [0, prod q)."""
    q = [int(v) for v in q]
    Q = math.prod(q)
    x = _obj(x)
    acc = np.zeros(x.shape[1:], dtype=object)
    for i, qi in enumerate(q):
        M = Q // qi
        acc = (acc + x[i] * (M * pow(M % qi, -1, qi))) % Q
    return acc


def crt_residues(v, q):
    return np.stack([_obj(v) % int(qi) for qi in q])


def switch_crt(v, q, r):
    """The independent statement: v = integers in [0, q_0...q_{k-1}) -> floor((v + floor(q_m/2)) / q_m) mod
    q_0...q_{m-1}, for m = k-1 down to r.  A quotient that reaches the smaller modulus wraps to 0."""
    q = [int(x) for x in q]
    v = _obj(v)
    for m in range(len(q) - 1, r - 1, -1):
        v = ((v + q[m] // 2) // q[m]) % math.prod(q[:m])
    return v


# ----------------------------------------------------------------------------------- the switched PIRDatabase::multiply

def local_ratios(orc, r):
    """(digit width, CiphertextReencoder's digits per residue) for the first r data primes: floor(log2 t) and
    ceil(log2(q_j) / that), both in doubles like ct_reencoder.cpp:29-38."""
    b = int(math.log2(float(orc.t)))
    return b, [int(math.ceil(math.log2(float(int(orc.moduli[j]))) / b)) for j in range(r)]


def reencode_level(orc, ct, r):
    """Encode of a ciphertext [2, r, N] at level r: (poly, j < r, digit < ler_j) in the reference's order -> [E', N]."""
    b, ler = local_ratios(orc, r)
    mask = np.uint64((1 << b) - 1)
    out = []
    for p in range(2):
        for j in range(r):
            for i in range(ler[j]):
                out.append((ct[p, j] >> np.uint64(i * b)) & mask)
    return np.stack(out)


def redecode_level(orc, pts, r):
    """Decode (ct_reencoder.cpp:79-111) of E' plaintexts -> [2, r, N]."""
    b, ler = local_ratios(orc, r)
    out = np.zeros((2, r, orc.N), dtype=np.uint64)
    e = 0
    for p in range(2):
        for j in range(r):
            for i in range(ler[j]):
                out[p, j] += np.asarray(pts[e], dtype=np.uint64) << np.uint64(i * b)
                e += 1
    assert e == len(pts)
    return out


def expansion_ratio_level(orc, r):
    return sum(local_ratios(orc, r)[1])


def _sum_products(orc, pts_ntt, sv):
    """sum_i sv[i] * pts_ntt[i], returned in coefficient form [2, k, N]: the oracle's one-dimensional multiply."""
    n = pts_ntt.shape[0]
    rc, out = orc.db_multiply(np.ascontiguousarray(pts_ntt), [n], np.ascontiguousarray(sv[:n]).copy())
    assert rc == 0 and out.shape[0] == 1
    return out[0]


def multiply_switched(orc, db_ntt, dims, sv, r, trace=None):
    """PIRDatabase::multiply (database.cpp:170-258) with every level result switched to r primes right after its
    inverse transform and before Encode reads it.  db_ntt [P, k, N]; sv = the coefficient-form selection vector
    [dim_sum, 2, k, N]; -> reply [E'^(d-1), 2, r, N].  trace (a list) receives every level's switched ciphertexts."""
    dims = list(dims)
    d = len(dims)
    q = [int(v) for v in orc.moduli[:orc.k]]
    off = [sum(dims[:l]) for l in range(d)]
    P = db_ntt.shape[0]
    cols = dims[-1]
    # level d - 1: one sum per row of the scanned matrix
    rows = -(-P // cols) if d > 1 else 1
    sv_last = sv[off[d - 1]:off[d - 1] + cols]
    level = [[switch_residues(_sum_products(orc, db_ntt[x * cols:min((x + 1) * cols, P)], sv_last), q, r)]
             for x in range(rows)]
    if trace is not None:
        trace.append(level)
    for l in range(d - 2, -1, -1):
        sv_l = sv[off[l]:off[l] + dims[l]]
        parents = -(-len(level) // dims[l])
        nxt = []
        for node in range(parents):
            kids = level[node * dims[l]:(node + 1) * dims[l]]
            res = []
            for cc in range(len(kids[0])):
                enc = [reencode_level(orc, kid[cc], r) for kid in kids]            # per child: [E', N]
                for e in range(enc[0].shape[0]):
                    pts = orc.db_from_coeffs([c[e] for c in enc])
                    res.append(switch_residues(_sum_products(orc, pts, sv_l), q, r))
            nxt.append(res)
        level = nxt
        if trace is not None:
            trace.append(level)
    assert len(level) == 1
    return np.stack(level[0])


def process_query_switched(orc, db_ntt, dims, query, keys, r):
    """processQuery (server.cpp:173-195) with switched level results: oblivious expansion by the oracle, then
    multiply_switched."""
    rc, sv = orc.oblivious_expansion_multi(query, sum(dims), keys)
    assert rc == 0
    return multiply_switched(orc, db_ntt, dims, sv, r)


# ------------------------------------------------------------------------------------------- decryption at a level

def _phase_level(client, ct, r):
    o = client.o
    res = [o.poly_add(j, ct[0, j], o.ntt_inv(j, o.dyadic_mul(j, o.ntt_fwd(j, ct[1, j]), client.s_ntt[j])))
           for j in range(r)]
    return crt_compose(np.stack(res), client.q[:r])


def decrypt_level(client, ct, r):
    """ct [2, r, N] over q_0..q_{r-1} -> plaintext coefficients: round(t x / Q_r) mod t on the phase x."""
    t, Q = client.t, math.prod(client.q[:r])
    x = _phase_level(client, np.asarray(ct), r)
    return (((x * t + (Q >> 1)) // Q) % t).astype(np.uint64)


def noise_budget_level(client, ct, r):
    """Invariant noise budget in bits at level r (the oracle client's formula over Q_r)."""
    t, Q = client.t, math.prod(client.q[:r])
    x = _phase_level(client, np.asarray(ct), r)
    worst = 0
    for v in ((x * t) % Q).tolist():
        worst = max(worst, min(v, Q - v))
    if worst == 0:
        return float(Q.bit_length())
    return max(0.0, math.log2(Q) - math.log2(worst) - 1)


def process_reply_level(client, n_dims, reply, r):
    """ProcessReplyCiphertextDecomp (client.cpp:219-255) on a reply at level r -> plaintext coefficients."""
    E = 2 * expansion_ratio_level(client.o, r)
    assert reply.shape[0] == E ** (n_dims - 1)
    cts = [np.asarray(c) for c in reply]
    pts = []
    for _ in range(n_dims):
        pts = [decrypt_level(client, c, r) for c in cts]
        if len(pts) <= 1:
            break
        cts = [redecode_level(client.o, pts[i * E:(i + 1) * E], r) for i in range(len(cts) // E)]
    return pts[0]


# ------------------------------------------------------------------------------------------- inputs on the step's edges

def boundary_values(q, rng):
    """CRT integers in [0, Q) that sit on the step's edges, for every step m = k-1 .. 1 (a value w at level m + 1 is
    reached exactly from w * q_{m+1} ... q_{k-1}: floor((w q + floor(q/2)) / q) = w)."""
    k = len(q)
    out = [0, math.prod(q) - 1]
    for m in range(k - 1, 0, -1):
        Qm, qm, h = math.prod(q[:m + 1]), q[m], q[m] // 2
        lift = math.prod(q[m + 1:])
        ws = [Qm - 1, Qm - h - 1, Qm - h, Qm - h + 1]                       # the quotient reaches Q_m / q_m: wraps to 0
        for i in range(m):
            for c in (int(rng.integers(1, 1000)) * q[i], int(rng.integers(1, 1000)) * q[i] - 1):   # quotient = 0 and = -1 mod q_i
                c = int(c) % (Qm // qm)
                ws += [c * qm - h + int(u) for u in (0, qm - 1, rng.integers(0, qm))]
        out += [w * lift for w in ws if 0 <= w < Qm]
    return out


def switch_inputs(q, N, rng):
    """[4, 2, k, N] canonical residues: random, with the boundary cases written over the first coefficients of
    ciphertext 0 (both components: even and odd lanes of a thread's pair) and the last ones of ciphertext 3."""
    k = len(q)
    cts = np.empty((4, 2, k, N), dtype=np.uint64)
    for j in range(k):
        cts[:, :, j, :] = rng.integers(0, q[j], size=(4, 2, N), dtype=np.uint64)
    cols = [[0] * k, [x - 1 for x in q]]                                           # every residue 0 / q_i - 1
    for m in range(1, k):                                                          # x_m around q_m - h: a wraps
        for v in (q[m] - q[m] // 2 - 1, q[m] - q[m] // 2, q[m] - q[m] // 2 + 1, q[m] - 1, 0):
            col = [int(rng.integers(0, x)) for x in q]
            col[m] = v
            cols.append(col)
    cols += [[v % x for x in q] for v in boundary_values(q, rng)]
    special = np.array(cols, dtype=np.uint64).T                                    # [k, n_special]
    n = special.shape[1]
    assert 2 * n + 1 < N
    cts[0, 0, :, :n] = special
    cts[0, 1, :, 1:n + 1] = special
    cts[3, 1, :, N - n:] = special
    return cts
