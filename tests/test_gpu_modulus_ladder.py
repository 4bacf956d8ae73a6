"""The modulus sizes at which the kernels change their arithmetic, one rung on each side of every cut-off, each rung bit
for bit against the CPU oracle.  The rules (ctx.hip, scan_mfma.hip `mfma_geometry`; DESIGN.md "limits that are tested"):

  transform flavour        exact fp64 below 2^46, wide fp64 below 2^49, else integer
  lazy inverse transform   exact fp64 only, bits(q_max) + log2 N <= 52
  packed key-switch width  5 / 6 / 7 bytes up to 39 / 47 / 55 bits of ALL moduli (the integer flavour: 5 bytes or u64)
  scan digits              L = 5 / 6 / 7 up to 39 / 47 / 55 bits of the DATA moduli, above: the 64-bit scan
  top scan digit a nibble  up to 36 bits at L = 5, 44 at L = 6, never at L = 7
  fp64 fold of the scan    data moduli below 2^50
  lazy_limit               2^(128 - 2 bits), capped at 2^30

Every rung asserts the path it expects to have run (`ntt_mode`, `arith_info`, `scan_info`): a changed rule shows up as
a failing expectation, not as a silent change of path.  The expectations are literal; they are not recomputed from the
rules.  The chains are CoeffModulus::Create(N, [bits, ...]): the largest primes of that size, the ones closest to the
cut-off.  test_gpu_extreme_values.py feeds the same rungs structured worst-case residues."""
import numpy as np
import pytest

import oracle
import pir_amd
from gpu_helpers import chain, random_ct, random_key, to_product_params
from pir_fixtures import generate_test_db

pytestmark = pytest.mark.gpu


class Rung:
    def __init__(self, N, data, special, mode, lazy, pack, L, nibble, below50=True, lazy_limit=1 << 30):
        self.N, self.data, self.special = N, data, special
        self.mode, self.lazy, self.pack, self.L, self.nibble = mode, lazy, pack, L, nibble
        self.below50 = below50          # every data modulus < 2^50: limb accumulators and the fp64 fold of the scan
        self.lazy_limit = lazy_limit
        self.bits = data if isinstance(data, int) else max(data)
        self.all_bits = max(self.bits, special or 0)

    @property
    def id(self):
        d = str(self.data) if isinstance(self.data, int) else "-".join(map(str, self.data))
        return "n%d_%sbit%s" % (self.N, d, "_p%d" % self.special if self.special else "")

    def moduli(self):
        return chain(self.N, self.data, self.special)


#        N      data  special | flavour lazy   pack L  nibble
RUNGS = [
    # nibble -> byte top digit at L = 5, by the moduli
    Rung(4096, 36, None, 1, True, 5, 5, True),
    Rung(4096, 37, None, 1, True, 5, 5, False),
    # 5 -> 6 packed bytes, L = 5 -> 6; 40 bits is the last lazy-inverse rung at N = 4096
    Rung(4096, 39, None, 1, True, 5, 5, False),
    Rung(4096, 40, None, 1, True, 6, 6, True),
    # lazy inverse on -> off: bits + log2 N = 52 / 53, with three, four and 4 + 4 + 3-stage passes
    Rung(4096, 41, None, 1, False, 6, 6, True),
    Rung(16384, 38, None, 1, True, 5, 5, False),
    Rung(16384, 39, None, 1, False, 5, 5, False),
    Rung(2048, 41, None, 1, True, 6, 6, True),
    Rung(2048, 42, None, 1, False, 6, 6, True),
    # nibble -> byte at L = 6
    Rung(8192, 44, None, 1, False, 6, 6, True),
    Rung(8192, 45, None, 1, False, 6, 6, False),
    # exact fp64 -> wide fp64 at its budget; 46 bits at N = 16384 is the "14 stages" case of ntt_core.h
    Rung(4096, 46, None, 1, False, 6, 6, False),
    Rung(8192, 46, None, 1, False, 6, 6, False),
    Rung(16384, 46, None, 1, False, 6, 6, False),
    Rung(4096, 47, None, 2, False, 6, 6, False),
    Rung(8192, 47, None, 2, False, 6, 6, False),
    Rung(16384, 47, None, 2, False, 6, 6, False),
    # 6 -> 7 packed bytes, L = 6 -> 7
    Rung(8192, 48, None, 2, False, 7, 7, False),
    # wide fp64 -> integer
    Rung(8192, 49, None, 2, False, 7, 7, False, lazy_limit=1 << 30),
    Rung(8192, 50, None, 0, False, 8, 7, False, lazy_limit=1 << 28),
    # limb accumulators and fp64 fold of the scan -> 128-bit accumulators: the rule is q < 2^50, which a 50-bit prime
    # still meets -- the cut-off sits between 50 and 51 bits, one rung above the change of flavour
    Rung(8192, 51, None, 0, False, 8, 7, False, below50=False, lazy_limit=1 << 26),
    # L = 7 -> no MFMA scan: the 64-bit kernels take over
    Rung(4096, 55, None, 0, False, 8, 7, False, below50=False, lazy_limit=1 << 18),
    Rung(4096, 56, None, 0, False, 8, 0, False, below50=False, lazy_limit=1 << 16),
    # the integer flavour at SEAL's largest size, and at the largest size the context accepts
    Rung(4096, 60, None, 0, False, 8, 0, False, below50=False, lazy_limit=1 << 8),
    Rung(16384, 60, None, 0, False, 8, 0, False, below50=False, lazy_limit=1 << 8),
    Rung(4096, 61, None, 0, False, 8, 0, False, below50=False, lazy_limit=1 << 6),
    # mixed chains: the scan reads the data primes, the packed width all primes
    Rung(4096, 36, 40, 1, True, 6, 5, True),
    Rung(4096, [30, 36, 40], 40, 1, True, 6, 6, True),
]
BY_ID = {r.id: r for r in RUNGS}
assert len(BY_ID) == len(RUNGS)


class Setup:
    """PirSetup without the client (its key generation is the expensive part at N = 16384): parameters, oracle,
    database."""

    def __init__(self, n_pt, d, N, moduli, plain_bits=20):
        self.params = p = oracle.create_pir_parameters(n_pt, 0, d, N=N, plain_bits=plain_bits, moduli=moduli)
        self.orc = oracle.Oracle.from_params(p)
        self.raw = generate_test_db(n_pt, p.bytes_per_item)
        rc, self.db_ntt = self.orc.db_encode(self.raw.tobytes(), n_pt, p.bytes_per_item, p.items_per_plaintext,
                                             p.eff_bits_per_coeff, p.num_pt)
        assert rc == 0


def server(s):
    pp = to_product_params(s.params)
    db = pir_amd.PIRDatabase.Create(pp)
    db.populate(s.raw)
    return db, pir_amd.PIRServer(db, pp)


def forced_pack(rung, mode):
    """Packed width of a rung under a forced flavour: the integer flavour knows 5 bytes or u64 words only."""
    return rung.pack if mode != 0 or rung.pack == 5 else 8


def assert_path(srv, rung, mode=None):
    mode = rung.mode if mode is None else mode
    a = srv.arith_info()
    assert srv.ntt_mode() == mode and a["ntt_mode"] == mode, a
    assert a["f64_lazy_inv"] == (rung.lazy and mode == 1), a
    assert a["pack_bytes"] == forced_pack(rung, mode), a
    assert a["lazy_limit"] == rung.lazy_limit, a
    # the tree between the fused levels is packed with the digits, except with 7-byte residues at N = 16384
    assert a["tree40"] == (a["pack_bytes"] <= 7 and not (a["pack_bytes"] == 7 and rung.N >= 16384)), a


def transform_and_key_switch_families(s, db, srv, rng):
    """What test_gpu_ntt_modes.test_transform_and_key_switch_flavours runs, key-level transforms included."""
    N, orc = s.params.N, s.orc
    cts = random_ct(orc, rng, 2)
    fwd = srv.ntt_forward(cts)
    assert np.array_equal(fwd, np.stack([orc.ct_ntt_fwd(c) for c in cts]))
    assert np.array_equal(srv.ntt_inverse(fwd), cts)
    assert np.array_equal(srv.ntt_inverse(cts), np.stack([orc.ct_ntt_inv(c) for c in cts]))   # not only as a round trip
    kl = np.stack([rng.integers(0, q, size=(2, N), dtype=np.uint64) for q in orc.moduli], axis=1)     # [2, k + 1, N]
    fk = srv.ntt_forward(kl, key_level=True)
    ik = srv.ntt_inverse(kl, key_level=True)
    for b in range(2):
        for i in range(orc.k + 1):
            assert np.array_equal(fk[b, i], orc.ntt_fwd(i, kl[b, i])), (b, i)
            assert np.array_equal(ik[b, i], orc.ntt_inv(i, kl[b, i])), (b, i)
    for g in (3, N + 1, N // 4 + 1):
        key = random_key(orc, rng)
        srv.set_galois_keys({g: key})
        rc, exp = orc.apply_galois_ct(cts[0], g, key)
        assert rc == 0 and np.array_equal(srv.substitute_power_x_inplace(cts[0].copy(), g), exp), g
    keys = {(N >> j) + 1: random_key(orc, rng) for j in range(4)}
    srv.set_galois_keys(keys)
    rc, exp = orc.oblivious_expansion(cts[1], 11, keys)
    assert rc == 0 and np.array_equal(srv.oblivious_expansion(cts[1], 11), exp)
    for i in range(s.params.num_pt):
        assert np.array_equal(db.read_plaintext(i), s.db_ntt[i]), i


@pytest.mark.parametrize("rung", [r.id for r in RUNGS])
def test_rung_default_flavour(rung):
    """One context of 70 plaintexts (9 x 8: enough rows for the MFMA scan where the moduli allow it): transforms, key
    switch, expansion and database encode, then a d = 2 query alone and in a batch of 3."""
    r = BY_ID[rung]
    N = r.N
    s = Setup(70, 2, N, r.moduli())
    assert [int(q).bit_length() for q in s.params.moduli] == ([r.data] * 2 if isinstance(r.data, int) else r.data) + \
        [r.special or r.bits]
    db, srv = server(s)
    assert_path(srv, r)
    info, a = srv.scan_info(), srv.arith_info()
    assert info["rows"] == 9 and info["mfma"] == (r.L != 0), info
    if r.L:
        assert info["digits"] == r.L and info["top_digit_nibble"] == r.nibble, info
        assert info["single_query_mfma"], info
    # the single-query fold is on from 6 digits (ctx.hip: measured slower at 5), the group fold whenever the moduli allow
    assert a["scan_limb"] == r.below50 and a["scan_f64_fold_batch"] == r.below50, a
    assert a["scan_f64_fold"] == (r.below50 and r.L >= 6), a
    rng = np.random.default_rng(N + r.all_bits)
    transform_and_key_switch_families(s, db, srv, rng)
    keys = {(N >> j) + 1: random_key(s.orc, rng) for j in range(N.bit_length() - 1)}
    srv.set_galois_keys(keys)
    queries = random_ct(s.orc, rng, 3)[:, None]
    exp = []
    for q in queries:
        rc, e = s.orc.process_query(s.db_ntt, s.params.dimensions, q, keys)
        assert rc == 0
        exp.append(e)
    assert np.array_equal(srv.process_query(queries[0]), exp[0])
    batch = srv.process_batch(queries, n_workers=3)
    for i in range(3):
        assert np.array_equal(batch[i], exp[i]), i
    db.close()


FORCED = [(r.id, m) for r in RUNGS for m in (0, 2) if m != r.mode and (m == 0 or r.all_bits <= 49)]


@pytest.mark.parametrize("rung,mode", FORCED)
def test_rung_forced_flavour(monkeypatch, rung, mode):
    """The other flavours the moduli allow (integer everywhere, wide fp64 below 2^49) on the transform and key-switch
    families: at 46 bits all three flavours run and must be indistinguishable."""
    r = BY_ID[rung]
    monkeypatch.setenv("PIRGPU_NTT_MODE", str(mode))
    s = Setup(12, 1, r.N, r.moduli())
    db, srv = server(s)
    assert_path(srv, r, mode)
    transform_and_key_switch_families(s, db, srv, np.random.default_rng(r.N + r.all_bits + mode))
    db.close()


def test_a_62_bit_modulus_is_refused():
    """61-bit primes are the largest the context accepts (Harvey's forward range 4q = 2^63 still fits a word); one bit
    more is an error, not a wrong reply."""
    moduli = chain(4096, 62)
    p = oracle.create_pir_parameters(12, 0, 1, N=4096, plain_bits=20, moduli=chain(4096, 61))
    p.moduli = moduli
    with pytest.raises(pir_amd.PirGpuError) as e:
        pir_amd.PIRDatabase.Create(to_product_params(p))
    assert e.value.code == pir_amd.StatusCode.INVALID_ARGUMENT


# ---------------------------------------------------------------- N = 32768 (ntt_ring32k.hip: integer flavour only)

@pytest.mark.parametrize("bits,L", [(55, 7), (56, 0)])
def test_ring32k_scan_leaves_the_mfma_path_at_56_bits(bits, L):
    """One pair at the expensive degree: the scan goes from 7 digits to the 64-bit kernels; the intermediates are u64
    words there whatever the moduli."""
    N = 32768
    s = Setup(70, 2, N, chain(N, bits))
    db, srv = server(s)
    a, info = srv.arith_info(), srv.scan_info()
    assert a["ntt_mode"] == 0 and not a["f64_lazy_inv"] and a["pack_bytes"] == 8 and not a["tree40"], a
    assert info["mfma"] == (L != 0) and (not L or (info["digits"] == L and not info["top_digit_nibble"])), info
    rng = np.random.default_rng(bits)
    keys = {(N >> j) + 1: random_key(s.orc, rng) for j in range(15)}
    srv.set_galois_keys(keys)
    queries = random_ct(s.orc, rng, 2)[:, None]
    rc, exp = s.orc.process_query(s.db_ntt, s.params.dimensions, queries[0], keys)
    assert rc == 0 and np.array_equal(srv.process_query(queries[0]), exp)
    batch = srv.process_batch(queries, n_workers=2)
    assert np.array_equal(batch[0], exp)
    rc, exp1 = s.orc.process_query(s.db_ntt, s.params.dimensions, queries[1], keys)
    assert rc == 0 and np.array_equal(batch[1], exp1)
    db.close()
