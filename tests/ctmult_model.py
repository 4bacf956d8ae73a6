"""CPU model of the ciphertext-multiplication mode -- TEST INFRASTRUCTURE ONLY.

The project's ct x ct product is the EXACT BFV product, stated here once in Python integers:

    A = (a0, a1), B = (b0, b1) in coefficient form, c(.) the centred CRT lift into [-h, h], h = (Q - 1) / 2
    x0 = a0 b0,  x1 = a0 b1 + a1 b0,  x2 = a1 b1        over Z[x] / (x^N + 1)
    d_i = floor((t x_i + h) / Q)   per coefficient (floor towards minus infinity; Q is odd, never a tie)

stored as canonical residues mod q_j.  Relinearisation is the oracle's key switch with the relinearisation key standing
where the Galois key of element 1 stands: (d0, d1, d2) -> apply_galois_ct((d0, d2), 1, rk) + (0, d1).

`rns_*` restate lift and scale the way the kernels compute them (Garner digits, centring by digit comparison, Horner into
the target moduli, an auxiliary base B of k + 2 primes) so that the formulation itself is checked against the integers
without a GPU.  `plan` restates pirgpu_ctmult_plan."""
import numpy as np

import oracle

# ---------------------------------------------------------------------------------------------- integers


def prod(xs):
    r = 1
    for x in xs:
        r *= int(x)
    return r


def crt_lift(res, q, centred=True):
    """res [k][N] canonical residues -> list of N Python ints: the centred lift (or the one in [0, Q))."""
    q = [int(x) for x in q]
    Q = prod(q)
    h = (Q - 1) // 2
    cols = []
    for j, qj in enumerate(q):
        Mj = Q // qj
        f = Mj * pow(Mj % qj, -1, qj) % Q
        cols.append((f, np.asarray(res[j]).tolist()))
    out = []
    for i in range(len(cols[0][1])):
        x = 0
        for f, col in cols:
            x += col[i] * f
        x %= Q
        out.append(x - Q if centred and x > h else x)
    return out


def to_residues(xs, q):
    return np.array([[x % int(qj) for x in xs] for qj in q], dtype=np.uint64)


def _pack(a, W):
    """signed ints |a_i| < 2^(W - 1) -> sum a_i 2^(W i) (one big integer)."""
    off, nb = 1 << (W - 1), W // 8
    v = int.from_bytes(b"".join((x + off).to_bytes(nb, "little") for x in a), "little")
    return v - off * (((1 << (W * len(a))) - 1) // ((1 << W) - 1))


def _unpack(v, n, W):
    off, nb = 1 << (W - 1), W // 8
    v += off * (((1 << (W * n)) - 1) // ((1 << W) - 1))
    raw = v.to_bytes(nb * n, "little")
    return [int.from_bytes(raw[i * nb:(i + 1) * nb], "little") - off for i in range(n)]


def negacyclic_mul(a, b):
    """a, b: N signed ints each -> their product in Z[x] / (x^N + 1), by Kronecker substitution (a constant operand
    multiplies coefficient by coefficient)."""
    N = len(a)
    for u, v in ((a, b), (b, a)):
        if not any(v[1:]):
            return [x * v[0] for x in u]
    bound = max(1, max(abs(x) for x in a)) * max(1, max(abs(x) for x in b)) * N
    W = (bound.bit_length() + 2 + 7) // 8 * 8
    full = _unpack(_pack(a, W) * _pack(b, W), 2 * N - 1, W) + [0]
    return [full[i] - full[i + N] for i in range(N)]


def tensor(A, B, q):
    """A, B [2][k][N] -> (x0, x1, x2) as integer lists (the products of the centred lifts)."""
    a0, a1, b0, b1 = (crt_lift(p, q) for p in (A[0], A[1], B[0], B[1]))
    # (a big product costs half a second at N = 8192: equal operands share theirs)
    p00 = negacyclic_mul(a0, b0)
    p01 = p00 if b1 == b0 else negacyclic_mul(a0, b1)
    p10 = p00 if a1 == a0 else negacyclic_mul(a1, b0)
    p11 = p10 if b1 == b0 else (p01 if a1 == a0 else negacyclic_mul(a1, b1))
    return p00, [u + v for u, v in zip(p01, p10)], p11


def scale(x, q, t):
    Q = prod(q)
    h = (Q - 1) // 2
    return [(t * v + h) // Q for v in x]


def scaled_residues(x, q, t):
    """(x0, x1, x2) integer polynomials -> [3][k][N] canonical residues of floor((t x_i + h) / Q)."""
    return np.stack([to_residues(scale(xi, q, t), q) for xi in x])


def multiply_ct(A, B, q, t):
    """The exact BFV product: [2][k][N] x [2][k][N] -> [3][k][N] canonical residues."""
    return scaled_residues(tensor(A, B, q), q, t)


# ---------------------------------------------------------------------------------------------- the plan


def plan(N, q, special, t):
    """pirgpu_ctmult_plan restated: (aux primes, ok).  The k + 2 largest primes == 1 mod 2N below 2^bits, bits = the size
    of the largest data prime, descending, that are neither in the chain nor the special prime; ok = both bounds hold."""
    q = [int(x) for x in q]
    bits = max(q).bit_length()
    aux, v = [], (1 << bits) - 2 * N + 1
    while len(aux) < len(q) + 2 and v > (1 << (bits - 1)):
        if v not in q and v != special and oracle.is_prime(v):
            aux.append(v)
        v -= 2 * N
    if len(aux) < len(q) + 2:
        return aux, False
    Q, Bp = prod(q), prod(aux)
    ok = Q * Bp > 2 * (t * N * (Q - 1) ** 2 // 2 + Q) and Bp > 2 * (t * N * Q + 2)
    return aux, ok


# The chains of the GPU ladder (tests/test_gpu_ctmult_ladder.py): (id, N, bits of the data primes,
# bits of t).  The chain is oracle.coeff_modulus_create(N, bits + [max(bits)]), t = oracle.plain_modulus_batching(N, t_bits).
LADDER = [("k1", 2048, [54], 20), ("k2-tight", 4096, [30, 30], 46), ("k3-mixed", 4096, [30, 36, 40], 20),
          ("k3-wide", 4096, [47, 47, 47], 20), ("k3-pack7", 8192, [48, 48, 48], 20), ("k5", 4096, [41] * 5, 20),
          ("k6-f64", 4096, [40] * 6, 20), ("k6-int", 4096, [60] * 6, 59), ("n16384", 16384, [46, 46], 20)]
# The pairs of hook_inputs a rung with k >= 5 or N = 16384 keeps
SUB_FAMILY = ["random 0", "all q_j - 1", "full h", "full h + 1", "delta -1", "delta 0", "delta 1"]

# ---------------------------------------------------------------------------------------------- RNS formulation


def garner(res, p):
    """residues res[j] mod p[j] -> mixed-radix digits v: x = v0 + v1 p0 + v2 p0 p1 + ... (word arithmetic only)."""
    v = []
    for j, pj in enumerate(p):
        u = res[j]
        for i in range(j):
            u = (u - v[i]) * pow(p[i], -1, pj) % pj
        v.append(u)
    return v


def convert(res, p, targets, centred):
    """Exact base conversion of one value: residues mod p -> residues mod targets of the lift in [0, P), or of the centred
    lift.  Centring decision: digit-wise comparison with the digits of (P - 1) / 2, most significant first."""
    v = garner(res, p)
    P = prod(p)
    above = False
    if centred:
        hd = garner([((P - 1) // 2) % pj for pj in p], p)
        for a, b in zip(reversed(v), reversed(hd)):
            if a != b:
                above = a > b
                break
    out = []
    for m in targets:
        r = v[-1] % m
        for j in range(len(p) - 2, -1, -1):
            r = (r * (p[j] % m) + v[j] % m) % m
        out.append((r - P % m) % m if above else r)
    return out


def rns_lift(res, q, aux):
    """Lift kernel: [k][N] canonical residues mod Q -> [kb][N] residues of the centred lift at the auxiliary base."""
    q, aux = [int(x) for x in q], [int(x) for x in aux]
    cols = np.asarray(res).T.tolist()
    return np.array([convert(c, q, aux, True) for c in cols], dtype=np.uint64).T


def rns_scale(xq, xb, q, aux, t):
    """Scale kernel on one polynomial: residues of the integer x at Q ([k][N]) and at B ([kb][N]) -> canonical residues of
    floor((t x + h) / Q) at Q."""
    q, aux = [int(x) for x in q], [int(x) for x in aux]
    Q = prod(q)
    h = (Q - 1) // 2
    out = []
    for cq, cb in zip(np.asarray(xq).T.tolist(), np.asarray(xb).T.tolist()):
        wq = [(t * x + h) % m for x, m in zip(cq, q)]
        wb = [(t * x + h) % m for x, m in zip(cb, aux)]
        rb = convert(wq, q, aux, False)                      # r = w mod Q, exactly, at B
        y = [(w - r) * pow(Q % m, -1, m) % m for w, r, m in zip(wb, rb, aux)]
        out.append(convert(y, aux, q, True))
    return np.array(out, dtype=np.uint64).T


def rns_multiply_ct(A, B, q, aux, t):
    """multiply_ct the way the device computes it, with exact integer ring products standing in for the transforms."""
    q = [int(x) for x in q]
    x = tensor(A, B, q)
    return np.stack([rns_scale(to_residues(xi, q), to_residues(xi, aux), q, aux, t) for xi in x])


# ---------------------------------------------------------------------------------------------- keys, relinearisation


def relin_key(client):
    """Relinearisation key of the oracle client's secret, in the shape of client.galois_key: [k][2][k + 1][N], NTT form,
    one RLWE sample per RNS digit carrying p * s^2."""
    o, k, km = client.o, client.k, client.k + 1
    new_key = np.stack([o.dyadic_mul(i, client.s_ntt[i], client.s_ntt[i]) for i in range(km)])
    key = np.empty((k, 2, km, client.N), dtype=np.uint64)
    p = client.q[k]
    for j in range(k):
        c0, c1 = client._rlwe_zero_sym()
        factor = np.full(client.N, p % client.q[j], dtype=np.uint64)
        c0[j] = o.poly_add(j, c0[j], o.dyadic_mul(j, new_key[j], factor))
        key[j, 0], key[j, 1] = c0, c1
    return key


def relinearize(orc, d, rk):
    """(d0, d1, d2) [3][k][N] -> (d0 + KS0(d2), d1 + KS1(d2)) with the oracle's key switch (Galois element 1)."""
    rc, out = orc.apply_galois_ct(np.stack([d[0], d[2]]), 1, np.ascontiguousarray(rk))
    assert rc == 0
    for j in range(orc.k):
        out[1, j] = orc.poly_add(j, out[1, j], np.ascontiguousarray(d[1, j]))
    return out


def ct_add(orc, a, b):
    return np.stack([np.stack([orc.poly_add(j, np.ascontiguousarray(a[c, j]), np.ascontiguousarray(b[c, j]))
                               for j in range(orc.k)]) for c in range(2)])


def mul_relin(orc, A, B, rk):
    q = orc.moduli[:orc.k]
    return relinearize(orc, multiply_ct(A, B, q, orc.t), rk)


# ---------------------------------------------------------------------------------------------- the query path


def levels_ct(orc, db_ntt, dims, sv, rk):
    """PIRDatabase::multiply in ciphertext-multiplication mode on coefficient-form selectors sv [dim_sum][2][k][N]:
    row sums with the oracle's d = 1 path, then one exact product + relinearisation per child of every upper level,
    summed over the children that exist.  -> [2][k][N], or (rc, None) when a row sum fails (transparent)."""
    dims = list(dims)
    d = len(dims)
    off = [sum(dims[:l]) for l in range(d)]
    cols = dims[-1]
    P = db_ntt.shape[0]
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
            acc = None
            for i, child in enumerate(lower[r * dims[l]:(r + 1) * dims[l]]):
                term = mul_relin(orc, child, sv[off[l] + i], rk)
                acc = term if acc is None else ct_add(orc, acc, term)
            upper.append(acc)
        lower = upper
    assert len(lower) == 1
    return 0, lower[0]


def process_query_ct(orc, db_ntt, dims, query_cts, galois_keys, rk):
    """processQuery in ciphertext-multiplication mode -> (rc, reply [1][2][k][N])."""
    rc, sv = orc.oblivious_expansion_multi(query_cts, sum(dims), galois_keys)
    if rc != 0:
        return rc, None
    rc, out = levels_ct(orc, db_ntt, dims, sv, rk)
    return rc, None if out is None else out[None]


def process_response_ct(client, params, index, reply):
    """ProcessResponse on the one-ciphertext reply of the mode (reference client.cpp process_reply, multiplication
    branch) -> the item's bytes."""
    assert reply.shape[0] == 1
    pt = client.decrypt(reply[0])
    rc, data = oracle.string_decode(pt, params.eff_bits_per_coeff, params.bytes_per_item,
                                    oracle.calculate_item_offset(index, params.items_per_plaintext, params.bytes_per_item))
    assert rc == 0
    return data


# ---------------------------------------------------------------------------------------------- the hook's input family


def hook_inputs(q, t, N, rng, names=None):
    """One batch of pairs for pirgpu_ct_multiply: (names, A [n][2][k][N], B [n][2][k][N]).  Random pairs, all zero, every
    residue q_j - 1, the centring boundary h and h + 1 as constants and as full polynomials (all four polynomials at h in
    every coefficient puts the top coefficient of x0 at the magnitude bound N h^2, of x1 at twice that), and the constants
    a0 = c((delta - h) / t mod Q), b0 = 1 for delta in {-1, 0, 1}, which put (t x + h) mod Q at Q - 1, 0 and 1.
    `names`: keep these pairs only (a sub-family for the expensive chains; the random pairs drawn are the same either
    way).  check_hook_inputs needs "full h", "full h + 1" and the three "delta" pairs among them."""
    q = [int(x) for x in q]
    k, Q = len(q), prod(q)
    h = (Q - 1) // 2
    keep, names, As, Bs = names, [], [], []

    def const_ct(v0, v1, full=False):
        ct = np.zeros((2, k, N), dtype=np.uint64)
        for c, v in enumerate((v0, v1)):
            for j in range(k):
                if full:
                    ct[c, j, :] = v % q[j]
                else:
                    ct[c, j, 0] = v % q[j]
        return ct

    def rand_ct():
        ct = np.empty((2, k, N), dtype=np.uint64)
        for j in range(k):
            ct[:, j, :] = rng.integers(0, q[j], size=(2, N), dtype=np.uint64)
        return ct

    def add(name, A, B):
        if keep is not None and name not in keep:
            return
        names.append(name)
        As.append(A)
        Bs.append(B)

    add("random 0", rand_ct(), rand_ct())
    B1 = rand_ct()
    B1[1] = B1[0]                       # (b1 = b0: two big products in the model instead of four)
    add("random 1", rand_ct(), B1)
    add("zero", const_ct(0, 0), const_ct(0, 0))
    add("all q_j - 1", const_ct(Q - 1, Q - 1, True), const_ct(Q - 1, Q - 1, True))
    add("constant h", const_ct(h, h), const_ct(h, h))
    add("constant h + 1", const_ct(h + 1, h + 1), const_ct(h + 1, h + 1))
    add("full h", const_ct(h, h, True), const_ct(h, h, True))
    add("full h + 1", const_ct(h + 1, h + 1, True), const_ct(h + 1, h + 1, True))
    for delta in (-1, 0, 1):
        add("delta %d" % delta, const_ct((delta - h) * pow(t, -1, Q) % Q, 0), const_ct(1, 0))
    assert keep is None or sorted(keep) == sorted(names), "unknown pair name in names="
    return names, np.stack(As), np.stack(Bs)


def check_hook_inputs(names, tensors, q, t):
    """The family really reaches what it is built for: the three remainders and the magnitude bound.  tensors[i] = the
    (x0, x1, x2) of pair i (tensor)."""
    q = [int(x) for x in q]
    Q = prod(q)
    h = (Q - 1) // 2
    N = len(tensors[0][0])
    for delta in (-1, 0, 1):
        x0 = tensors[names.index("delta %d" % delta)][0]
        assert (t * x0[0] + h) % Q == delta % Q, (delta, (t * x0[0] + h) % Q)
    x0, x1, x2 = tensors[names.index("full h")]
    assert x0[N - 1] == N * h * h and x1[N - 1] == 2 * N * h * h and x2[N - 1] == N * h * h
    # h + 1 lifts to -h: the same magnitude through the other side of the centring
    assert tensors[names.index("full h + 1")][0][N - 1] == N * h * h
