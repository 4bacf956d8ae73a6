"""Structured worst-case residues at the rungs of test_gpu_modulus_ladder.py.

The budgets of the hand-written arithmetic (ntt_core.h, arith.h, scan_mfma.hip) are worst-case bounds; uniformly random
residues -- all the other GPU tests feed -- stay about a factor sqrt(N) inside them (tests/test_f64_bounds_model.py
shows it on a model).  The inputs here sit on the bounds:

  * transforms: constant vectors at 0, q - 1 and around q / 2, scaled unit vectors, "index bit set -> q - 1" masks and
    their complements, q - 1 - (small random), alternating 0 / q - 1 -- through ntt_forward and ntt_inverse directly
    (the worst case of the inverse is a pattern in the NTT domain), data level and key level, against the oracle and,
    where one exists, a closed form that does not involve the oracle;
  * key switch: keys and ciphertexts whose every residue is q_i - 1 or floor(q_i / 2) + 1;
  * the rounding of the special-prime division, with the accumulator chosen coefficient by coefficient next to 0, p / 2
    and p - 1, against floor((CRT(r) + floor(p / 2)) / p) in Python integers;
  * scan selectors on the boundaries of the digit decomposition for every digit count and top-digit form, against the
    oracle's db_multiply.  (The database side is random here; tests/test_gpu_scan_worst_case.py sets it through constant
    plaintexts and takes the accumulators of the scan to their bounds.)"""
import numpy as np
import pytest

import keyswitch_model
from gpu_helpers import chain, device_to_seal_order, random_ct, structured_patterns
from test_gpu_modulus_ladder import BY_ID, RUNGS, Setup, assert_path, server
from test_gpu_mfma_scan import setup_with_dims
from test_scan_digit_model import vmax

pytestmark = pytest.mark.gpu

# every fp64 rung of the ladder and one integer rung
VALUE_RUNGS = [r.id for r in RUNGS if r.mode != 0] + ["n8192_50bit"]


def _as_cts(polys_per_modulus, k):
    """[k][P, N] -> ciphertext-shaped [ceil(P / 2), 2, k, N] (zero padded)."""
    P, N = polys_per_modulus[0].shape
    out = np.zeros((2 * ((P + 1) // 2), k, N), dtype=np.uint64)
    for j in range(k):
        out[:P, j] = polys_per_modulus[j]
    return out.reshape(-1, 2, k, N)


@pytest.mark.parametrize("rung", VALUE_RUNGS)
def test_transforms_on_structured_patterns(rung):
    r = BY_ID[rung]
    N = r.N
    s = Setup(12, 1, N, r.moduli())
    orc, k = s.orc, s.orc.k
    db, srv = server(s)
    assert_path(srv, r)
    rng = np.random.default_rng(N)
    pats = [structured_patterns(q, N, rng) for q in orc.moduli]            # per modulus, the special prime included
    names = [n for n, _ in pats[0]]
    P = len(names)
    vals = [np.stack([v for _, v in pats[i]]) for i in range(k + 1)]        # [k + 1][P, N]
    # data level
    cts = _as_cts(vals[:k], k)
    fwd, inv = srv.ntt_forward(cts).reshape(-1, k, N), srv.ntt_inverse(cts).reshape(-1, k, N)
    # key level
    kl = np.stack(vals, axis=1)                                              # [P, k + 1, N]
    fk, ik = srv.ntt_forward(kl, key_level=True), srv.ntt_inverse(kl, key_level=True)
    for i in range(k + 1):
        q = int(orc.moduli[i])
        for p in range(P):
            ef, ei = orc.ntt_fwd(i, vals[i][p]), orc.ntt_inv(i, vals[i][p])
            assert np.array_equal(fk[p, i], ef), ("forward, key level", names[p], i)
            assert np.array_equal(ik[p, i], ei), ("inverse, key level", names[p], i)
            if i < k:
                assert np.array_equal(fwd[p, i], ef), ("forward", names[p], i)
                assert np.array_equal(inv[p, i], ei), ("inverse", names[p], i)
        # closed forms, independent of the oracle: NTT(c delta_0) = all-c, inverse(all-c) = c delta_0
        for c in (1, q - 1, q // 2, q // 2 + 1):
            delta = np.zeros(N, dtype=np.uint64)
            delta[0] = c
            flat = np.full(N, c, dtype=np.uint64)
            one = np.zeros((1, k + 1, N), dtype=np.uint64)
            one[0, i] = delta
            assert np.array_equal(srv.ntt_forward(one, key_level=True)[0, i], flat), (c, i)
            one[0, i] = flat
            assert np.array_equal(srv.ntt_inverse(one, key_level=True)[0, i], delta), (c, i)
    db.close()


def _extreme_ct_and_key(orc, kind):
    """Ciphertext and key whose every residue is q_i - 1 ("top") or floor(q_i / 2) + 1 ("half")."""
    f = (lambda q: q - 1) if kind == "top" else (lambda q: q // 2 + 1)
    ct = np.empty((2, orc.k, orc.N), dtype=np.uint64)
    key = np.empty((orc.k, 2, orc.k + 1, orc.N), dtype=np.uint64)
    for j in range(orc.k):
        ct[:, j, :] = f(int(orc.moduli[j]))
    for i in range(orc.k + 1):
        key[:, :, i, :] = f(int(orc.moduli[i]))
    return ct, key


def _key_switch_extremes(s, srv, rng):
    N, orc = s.params.N, s.orc
    for kind in ("top", "half"):
        ct, key = _extreme_ct_and_key(orc, kind)
        for g in (3, N + 1):
            srv.set_galois_keys({g: key})
            for c, label in ((ct, "extreme ct"), (random_ct(orc, rng)[0], "random ct")):
                rc, exp = orc.apply_galois_ct(c, g, key)
                assert rc == 0 and np.array_equal(srv.substitute_power_x_inplace(c.copy(), g), exp), (kind, g, label)
        keys = {(N >> j) + 1: key for j in range(4)}
        srv.set_galois_keys(keys)
        rc, exp = orc.oblivious_expansion(ct, 11, keys)
        assert rc == 0 and np.array_equal(srv.oblivious_expansion(ct, 11), exp), kind


@pytest.mark.parametrize("rung", VALUE_RUNGS)
def test_key_switch_with_extreme_keys_and_ciphertexts(rung):
    r = BY_ID[rung]
    s = Setup(12, 1, r.N, r.moduli())
    db, srv = server(s)
    assert_path(srv, r)
    _key_switch_extremes(s, srv, np.random.default_rng(r.N + 1))
    db.close()


# (N, bits, expected flavour, expected packed width) for k = 1 .. 4 data primes
K_RUNGS = [(4096, 39, 1, 5), (4096, 40, 1, 6), (8192, 46, 1, 6), (8192, 47, 2, 6), (8192, 49, 2, 7), (8192, 50, 0, 8)]


@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("N,bits,mode,pack", K_RUNGS)
def test_key_switch_extremes_for_every_digit_count(N, bits, mode, pack, k):
    s = Setup(12, 1, N, chain(N, [bits] * k))
    db, srv = server(s)
    a = srv.arith_info()
    assert a["ntt_mode"] == mode and a["pack_bytes"] == pack, a
    _key_switch_extremes(s, srv, np.random.default_rng(N + k))
    db.close()


def test_key_switch_extremes_at_ring32k():
    """N = 32768 has a key switch of its own (ntt_ring32k.hip)."""
    N = 32768
    s = Setup(12, 1, N, chain(N, 55))
    db, srv = server(s)
    assert srv.arith_info()["ntt_mode"] == 0
    _key_switch_extremes(s, srv, np.random.default_rng(N))
    db.close()


# ---------------------------------------------------------------- the special-prime rounding at its boundaries

# rungs where the flavour or the packed width changes: (N, bits of every prime, expected flavour, expected packed width).
# With p and q of 39 / 40 bits the stored x + q just fits / no longer fits 40 bits.
ROUNDING_RUNGS = [(4096, 36, 1, 5), (4096, 39, 1, 5), (4096, 40, 1, 6), (8192, 46, 1, 6), (8192, 47, 2, 6), (8192, 48, 2, 7),
                  (8192, 49, 2, 7), (8192, 50, 0, 8), (4096, 60, 0, 8)]


@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("N,bits,mode,pack", ROUNDING_RUNGS)
def test_special_prime_rounding_at_its_boundaries(N, bits, mode, pack, k):
    """c1 = the constant 1 makes every decomposition digit the all-ones vector in NTT form; a key that is zero except
    key[0, c, I] = NTT_I(r[c, I]) then makes the key-switch accumulator, in coefficient form, exactly r[c, I] for every
    modulus I, the special prime p included.  r is drawn per coefficient from the values next to the rounding
    boundaries of the division by p, and the output is compared with floor((CRT(r) + floor(p / 2)) / p) mod q_j
    (+ sigma_g(c0) on component 0) in Python integers, on all N coefficients, and with the oracle.  Both forms of key
    residency (set_galois_keys; install_keyset + use_keyset -- substitute_power_x_inplace honours the selected set).

    What the values decide: the integer kernels add floor(p / 2) to the special-prime residue and subtract
    floor(p / 2) mod q_j again, so any disagreement between the two constants moves every coefficient.  The fp64 kernels
    only CENTRE the signed representative the inverse transform left (|c| <= (p - 1) / 2); a wrong centring constant
    shows on the coefficients whose representative arrives as exactly +-(p + 1) / 2, which needs r = (p +- 1) / 2 AND a
    product that left the transform off-centre -- a few coefficients per polynomial at some rungs, none at others."""
    moduli = chain(N, [bits] * k)
    s = Setup(12, 1, N, moduli)
    orc = s.orc
    p = int(moduli[k])
    db, srv = server(s)
    a = srv.arith_info()
    assert a["ntt_mode"] == mode and a["pack_bytes"] == pack, a
    rng = np.random.default_rng(N + 7 * bits + k)
    ct = random_ct(orc, rng)[0]
    ct[1] = 0
    ct[1, :, 0] = 1
    r = np.empty((2, k + 1, N), dtype=np.uint64)
    special = np.array([0, 1, p // 2 - 1, p // 2, p // 2 + 1, p - 2, p - 1], dtype=np.uint64)
    r[:, k, :] = special[rng.integers(0, len(special), size=(2, N))]
    for j in range(k):
        q = int(moduli[j])
        data = np.array([0, 1, q - 1, q // 2, q // 2 + 1, (p // 2) % q, (p // 2 + 1) % q, (p - 1) % q], dtype=np.uint64)
        r[:, j, :] = data[rng.integers(0, len(data), size=(2, N))]
    key = np.zeros((k, 2, k + 1, N), dtype=np.uint64)
    for c in range(2):
        for i in range(k + 1):
            key[0, c, i] = orc.ntt_fwd(i, r[c, i])
    rounded = np.empty((2, k, N), dtype=np.uint64)
    for c in range(2):
        cols = [[int(v) for v in r[c, i]] for i in range(k + 1)]
        for n in range(N):
            x = (keyswitch_model.crt([col[n] for col in cols], moduli) + p // 2) // p
            for j in range(k):
                rounded[c, j, n] = x % int(moduli[j])
    for g in (3, N + 1):
        expected = rounded.copy()
        for j in range(k):
            expected[0, j] = orc.poly_add(j, expected[0, j], orc.apply_galois_poly(j, ct[0, j], g))
        rc, exp_orc = orc.apply_galois_ct(ct, g, key)
        assert rc == 0 and np.array_equal(exp_orc, expected), g      # the reference stays inside the contract
        srv.set_galois_keys({g: key})
        got = srv.substitute_power_x_inplace(ct.copy(), g)
        assert np.array_equal(got, expected), (g, "set_galois_keys", np.argwhere(got != expected)[:8])
        srv.set_galois_keys({})
        slot = srv.install_keyset(b"rounding-%d" % g, {g: key})
        srv.use_keyset(slot)
        got = srv.substitute_power_x_inplace(ct.copy(), g)
        assert np.array_equal(got, expected), (g, "keyset", np.argwhere(got != expected)[:8])
        srv.use_keyset(0)
        srv.release_keyset(slot)
    db.close()


# ---------------------------------------------------------------- scan boundary selectors, every L and top-digit form

# (label, N, data bits, digits, nibble by default)
SCAN_FORMS = [("L5 nibble", 4096, 36, 5, True), ("L5 byte 37", 4096, 37, 5, False), ("L5 byte 39", 4096, 39, 5, False),
              ("L6 nibble", 4096, 44, 6, True), ("L6 byte 45", 4096, 45, 6, False), ("L6 byte 47", 4096, 47, 6, False),
              ("L7", 4096, 49, 7, False), ("L7 55", 4096, 55, 7, False)]


def boundary_residues(q, bits, L):
    """Residues on the boundaries of the centring and of the balanced base-256 digits of the scan operands."""
    q = int(q)
    half, vm, top = q >> 1, vmax(L), 256 ** (L - 1)
    run = lambda b: int.from_bytes(bytes([b]) * L, "little")
    mixed = int.from_bytes(bytes([0x80, 0x7F] * L)[:L], "little")
    cases = [0, 1, q - 1, q - 2, half, half + 1, half - 1, half + 2, 0x7F, 0x80, 0x81,
             run(0x7F) % q, run(0x80) % q, mixed % q, q - 0x80, q - 0x8080,
             vm % q, (vm + 1) % q, (vm + 2) % q, (vm - 1) % q, 2 ** (bits - 1), 2 ** (bits - 1) - 1, 2 ** (bits - 1) + 1,
             (2 ** (bits - 1) - run(0x80) % 2 ** (bits - 1)) % q, (7 * top) % q, (7 * top - 1) % q,
             (run(0x80) & (16 * top - 1) | 15 * top) % q]
    assert all(0 <= c < q for c in cases)
    return np.array(sorted(set(cases)), dtype=np.uint64)


def _scan_variants(monkeypatch, s, sv_dev, count, expect_nibble):
    """Replies of the MFMA scan (default top digit), the MFMA scan with a byte top digit and the 64-bit scan."""
    k, N = s.orc.k, s.params.N
    replies = []
    for mfma, top4 in (("1", "1"), ("1", "0"), ("0", "1")):
        monkeypatch.setenv("PIRGPU_SCAN_MFMA", mfma)
        monkeypatch.setenv("PIRGPU_SCAN_MFMA_TOP4", top4)
        db, srv = server(s)
        info = srv.scan_info()
        assert info["mfma"] == (mfma == "1"), info
        assert info["top_digit_nibble"] == (mfma == "1" and top4 == "1" and expect_nibble), info
        srv.set_galois_keys(s.galois_keys)
        srv.set_concurrency(8)
        srv.stage_batch(np.zeros((count, 1, 2, k, N), dtype=np.uint64))   # sizes the reply buffers
        srv.batch_run_selectors(sv_dev.data_ptr(), count)
        replies.append(srv.fetch_batch())
        replies.append(info)
        db.close()
    return replies


def _check_against_db_multiply(s, sv, replies):
    """sv: [count, dim_sum, 2, k, N] in device order, NTT form."""
    seal = device_to_seal_order(sv)
    for i in range(sv.shape[0]):
        rc, exp = s.orc.db_multiply(s.db_ntt, s.params.dimensions, seal[i].copy(),
                                    sv_is_ntt=np.ones(seal.shape[1], np.uint8))
        assert rc == 0
        assert np.array_equal(replies[0][i], exp), i                  # against the reference
    assert np.array_equal(replies[0], replies[2]) and np.array_equal(replies[0], replies[4])    # the kernels agree
    assert replies[0].any()


@pytest.mark.parametrize("label,N,bits,L,nibble", SCAN_FORMS, ids=[f[0] for f in SCAN_FORMS])
def test_scan_boundary_selectors_against_the_oracle(monkeypatch, label, N, bits, L, nibble):
    import torch
    s = setup_with_dims(1, 2048, [17, 19], N=N, plain_bits=24, moduli=chain(N, bits))
    p, k = s.params, s.orc.k
    count = 3
    rng = np.random.default_rng(123 + bits)
    sv = np.empty((count, p.dim_sum, 2, k, N), dtype=np.uint64)
    for j in range(k):
        cases = boundary_residues(s.orc.moduli[j], bits, L)
        sv[:, :, :, j, :] = cases[rng.integers(0, len(cases), size=(count, p.dim_sum, 2, N))]
    replies = _scan_variants(monkeypatch, s, torch.from_numpy(sv.view(np.int64)).cuda(), count, nibble)
    assert replies[1]["digits"] == L, replies[1]
    _check_against_db_multiply(s, sv, replies)


# (label, N, bits, digits, nibble by default, columns): the widest chunk each kernel holds -- 7 k-steps of 64 columns at L <= 6, 6 at L = 7
WIDEST = [("L5 nibble", 4096, 36, 5, True, 440), ("L5 byte", 4096, 39, 5, False, 440), ("L6 nibble", 4096, 44, 6, True, 440),
          ("L6 byte", 4096, 47, 6, False, 440), ("L7", 4096, 55, 7, False, 380)]


@pytest.mark.parametrize("label,N,bits,L,nibble,cols", WIDEST, ids=[w[0] for w in WIDEST])
def test_scan_with_every_selector_at_one_extreme_residue(monkeypatch, label, N, bits, L, nibble, cols):
    """All selectors equal to the same extreme residue -- vmax(L), the largest value the asymmetric centring keeps
    positive, and vmax(L) + 1, the most negative one; for moduli too wide for the nibble form the centred extremes
    floor(q / 2) and floor(q / 2) + 1 as well -- over the widest chunk.  Only the selector side is extreme: the database
    is the transform of random bytes, so the digit products of a row sum add like a random walk and the int32 sums stay
    near 2^19, far below their bound (the groups and fp64 chunks likewise).  tests/test_gpu_scan_worst_case.py makes both
    sides coherent and reaches the bounds."""
    import torch
    s = setup_with_dims(0, 2048, [9, cols], N=N, plain_bits=24, moduli=chain(N, bits))
    p, k = s.params, s.orc.k
    values = [lambda q: vmax(L) % q, lambda q: (vmax(L) + 1) % q, lambda q: q // 2, lambda q: q // 2 + 1]
    sv = np.empty((len(values), p.dim_sum, 2, k, N), dtype=np.uint64)
    for i, f in enumerate(values):
        for j in range(k):
            sv[i, :, :, j, :] = f(int(s.orc.moduli[j]))
    replies = _scan_variants(monkeypatch, s, torch.from_numpy(sv.view(np.int64)).cuda(), len(values), nibble)
    info = replies[1]
    assert info["digits"] == L and info["chunks"] == 1 and info["ksteps"] == (7 if L <= 6 else 6), info
    _check_against_db_multiply(s, sv, replies)
