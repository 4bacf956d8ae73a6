"""Every sequence of level forms the oblivious expansion (expand_core in pir_amd/csrc/ctx.hip, planned by
pir_amd/csrc/expansion_plan.h) can take, against the CPU oracle, bit for bit -- no tolerance anywhere:

  A  deep sweep        N = 2048, one 27-bit data prime, d = 1: every group size 1 .. 8 at every depth 1 .. 11, n a power
                       of two, n = N, n = N + 3 (a second query ciphertext expanding three slots)
  B  double selectors  the same ring at d = 2 ([8, n - 8]): the int8-MFMA scan reads the selectors as doubles
  C  head split        HEAD_MODE = 2 with HEAD_LEVELS = 1 .. 8: the tree handed across streams at every level
  D  options           TREE40, PACK40, FUSE_MAC_COMBINE, LAST_NTT, FUSE_LAST, LOOP_TRANSFORMS off, C0_NTT = 1 / 2, the
                       integer flavour: one run per distinct walk
  E  production ring   N = 4096, two data primes (the loop threshold moves to 512 nodes), d = 2: one run per distinct walk

Member i of every group is ciphertext i of 8 fixed random ciphertexts per ring, expanded with the Galois keys of client
i (install_keyset / set_batch_keysets): a key or an output taken from a neighbour shows at every group size.  The
databases are random non-zero plaintexts, so every selector reaches the reply.  The oracle's replies are computed once
per (ring, d, n, member) and shared by all group sizes and parts.

Every run asserts its path (scan_info / expansion_forms' selector bit) and that the walk pirgpu_expansion_forms reports
is the walk `walk_by_rule` below -- the rule table of DESIGN.md section 4 restated -- says it meant to run.  The last
test compares the level records of all runs with what tests/cpp/expansion_plan_test.cpp --reachable finds reachable."""
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle
import pir_amd
from gpu_helpers import random_ct, to_product_params
from oracle.client import Client

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RINGS = {"A": dict(N=2048, bits=[27, 27], plain_bits=14), "E": dict(N=4096, bits=None, plain_bits=20)}
GROUPS = range(1, 9)
N_A = sorted({2 ** (m - 1) + 1 for m in range(1, 12)} | {64, 128, 256, 2048, 127, 511, 2051})
N_B, B_B = (65, 129, 200, 257, 513, 1025), (1, 2, 3, 5, 7, 8)
N_E = (65, 129, 257)      # (with 513 the part took 19.9 s, about half of it the oracle's six expansions of 513 slots: cut)
OPTIONS = ("TREE40=0", "PACK40=0", "FUSE_MAC_COMBINE=0", "LAST_NTT=0", "FUSE_LAST=0", "LOOP_TRANSFORMS=0", "C0_NTT=1",
           "C0_NTT=2", "PIRGPU_NTT_MODE=0")
RECORD = ("form", "tin40", "tout40", "c0_in_digit", "loop_targets", "c0ntt")
RAN = {}     # (ring, option setting) -> level records of the runs made, for the coverage condition
DONE = set()    # the cases of parts A, D and E that ran in this process (the coverage test runs the others itself)
REPLIES = {}    # (ring, d, n, member) -> the oracle's reply: computed once for all group sizes and parts


def walk_by_rule(N, k, B, n, option=None, head=0):
    """The walk of a group of B queries expanding n slots, from the rule table alone: [(form, tin40, tout40,
    c0_in_digit, loop_targets, c0ntt, on_head)] per level."""
    off = lambda name: option == name + "=0"
    fp64 = option != "PIRGPU_NTT_MODE=0"
    depth = (n - 1).bit_length()
    fused_last = fp64 and not off("FUSE_LAST")
    last_ntt = fused_last and not off("LAST_NTT")
    fuse_from = 64 if B > 1 else 128

    def form(j):
        if j + 1 == depth and fused_last:
            return "last_ntt" if last_ntt else "last_coeff"
        return "fused" if fp64 and not off("FUSE_MAC_COMBINE") and (B << j) >= fuse_from else "unfused"
    forms = [form(j) for j in range(depth)]
    c0_path = option in ("C0_NTT=1", "C0_NTT=2") and last_ntt
    split = head if B > 1 and head and depth >= head + 2 else 0
    out, tin40 = [], False
    for j, f in enumerate(forms):
        nodes = B << j
        c0ntt = c0_path and (f == "fused" or (f == "last_ntt" and j > 0 and forms[j - 1] == "fused"))
        c0_in_digit = f == "last_ntt" and not c0ntt and nodes >= 256 and nodes % 8 == 0
        tout40 = False
        if f == "fused" and j + 1 < depth and not off("TREE40") and not off("PACK40") and (1 << j) < N // 16:
            if j + 2 == depth:      # into the last level: only the NTT-domain one reads 5-byte polynomials, and needs c0
                tout40 = last_ntt and (c0ntt or (2 * nodes >= 256 and 2 * nodes % 8 == 0))
            else:
                tout40 = forms[j + 1] == "fused"
        loop = fp64 and not off("LOOP_TRANSFORMS") and nodes * k >= 1024
        out.append((f, tin40, tout40, c0_in_digit, loop, c0ntt, j < split))
        tin40 = tout40
    return out


def reported(srv, B, n, head_split=False):
    forms = srv.expansion_forms(B, n, head_split)
    assert [f["level"] for f in forms] == list(range(len(forms))) and not any(f["invalid"] for f in forms), forms
    return forms, [tuple(f[key] for key in RECORD) + (f["on_head"],) for f in forms]


class World:
    """One ring: the oracle, 8 clients with their Galois keys, 8 random query ciphertext pairs."""

    def __init__(self, ring):
        r = RINGS[ring]
        self.ring, self.N = ring, r["N"]
        self.moduli = oracle.coeff_modulus_create(r["N"], r["bits"]) if r["bits"] else None
        probe = self.params(1, 16)
        self.orc = oracle.Oracle.from_params(probe)
        self.k = self.orc.k
        self.keys = [Client(self.orc, seed=100 + i).galois_keys() for i in range(8)]
        self.queries = random_ct(self.orc, np.random.default_rng(2048 + self.N), 16).reshape(8, 2, 2, self.k, self.N)
        self.queries.setflags(write=False)

    def params(self, d, n):
        r = RINGS[self.ring]
        kw = dict(N=r["N"], plain_bits=r["plain_bits"], moduli=self.moduli)
        if d == 1:
            return oracle.create_pir_parameters(n, 0, 1, **kw)
        p = oracle.create_pir_parameters(8 * (n - 8), 0, 2, **kw)
        p.dimensions = [8, n - 8]       # (forced, as tests/test_gpu_db_update.py forces its dimensions)
        return p


@functools.lru_cache(maxsize=None)
def world(ring):
    return World(ring)


class Case:
    """One database of one ring: d = 1 with n plaintexts or d = 2 as [8, n - 8]; dim_sum = n either way."""

    def __init__(self, ring, d, n):
        self.w, self.d, self.n = world(ring), d, n
        self.p = self.w.params(d, n)
        assert sum(self.p.dimensions) == n and self.p.num_pt == int(np.prod(self.p.dimensions))
        self.nq = n // self.w.N + 1      # query ciphertexts per query (server.cpp:154-158: one more than expanded at n = N)
        rng = np.random.default_rng(1000 * n + d)
        self.rows = rng.integers(1, self.p.t, size=(self.p.num_pt, self.w.N), dtype=np.uint64)
        self.db_ntt = self.w.orc.db_from_coeffs(list(self.rows))
        self.key = (ring, d, n)

    def query(self, i):
        return self.w.queries[i, :self.nq]

    def want(self, i):
        if self.key + (i,) not in REPLIES:
            rc, exp = self.w.orc.process_query(self.db_ntt, self.p.dimensions, np.ascontiguousarray(self.query(i)), self.w.keys[i])
            assert rc == 0
            REPLIES[self.key + (i,)] = exp
        return REPLIES[self.key + (i,)]

    def server(self, option=None, head=0, head_mode=None):
        pp = to_product_params(self.p)
        db = pir_amd.PIRDatabase.Create(pp)
        if option and not option.startswith("PIRGPU_"):
            name, value = option.split("=")
            db.set_option(name, int(value))
        if head_mode is not None:
            db.set_option("HEAD_MODE", head_mode)
        if head:
            db.set_option("HEAD_LEVELS", head)
        db.populate_coeffs(self.rows)
        srv = pir_amd.PIRServer(db, pp)
        srv.set_galois_keys(self.w.keys[0])
        self.slots = [srv.install_keyset(b"member-%d" % i, keys) for i, keys in enumerate(self.w.keys)]
        return db, srv


@functools.lru_cache(maxsize=3)          # (a d = 2 database of this file is up to 130 MB; the parts ask in order of n)
def case(ring, d, n):
    return Case(ring, d, n)


def check_path(c, srv, option, forms):
    """d = 1: the 64-bit scan; d = 2: the int8-MFMA scan with the group's selectors as doubles wherever the NTT-domain
    last level, which writes them, exists."""
    info = srv.scan_info()
    assert info["mfma"] == (c.d == 2), info
    assert srv.ntt_mode() == (0 if option == "PIRGPU_NTT_MODE=0" else 1)
    doubles = c.d == 2 and option not in ("LAST_NTT=0", "FUSE_LAST=0", "PIRGPU_NTT_MODE=0")
    assert all(f["sel_f64"] == doubles for f in forms), (option, forms)


def run_group(c, srv, B, option=None, head=0, runs=2):
    """A group of B: staged, run `runs` times without a fetch in between, fetched; the walk recorded."""
    forms, got_walk = reported(srv, B, min(c.n, c.w.N), head_split=bool(head))
    assert got_walk == walk_by_rule(c.w.N, c.w.k, B, min(c.n, c.w.N), option, head if c.n < c.w.N else 0), (B, c.n, option, head)
    check_path(c, srv, option, forms)
    RAN.setdefault((c.w.ring, option or "default"), set()).update(t[:6] for t in got_walk)
    if c.n > c.w.N:     # the second query ciphertext's few slots
        RAN[(c.w.ring, option or "default")].update(t[:6] for t in reported(srv, B, c.n - c.w.N)[1])
    srv.set_concurrency(B)
    srv.stage_batch(np.stack([c.query(i) for i in range(B)]))
    srv.set_batch_keysets(c.slots[:B])
    for _ in range(runs):
        srv.run_batch()
    return srv.fetch_batch()


def assert_members(c, got, B, members=None, what=None):
    assert got.shape[0] == B
    for i in (range(B) if members is None else members):
        assert np.array_equal(got[i], c.want(i)), (what, c.d, c.n, "B = %d" % B, "member %d" % i)


# ------------------------------------------------------------------------------------------------------ A: deep sweep

@pytest.mark.parametrize("n", N_A)
def test_deep_sweep(n):
    c = case("A", 1, n)
    assert c.w.k == 1 and c.w.orc.N == 2048
    db, srv = c.server()
    for B in GROUPS:
        assert_members(c, run_group(c, srv, B), B)
    db.close()
    DONE.add(("A", n))


# ------------------------------------------------------------------------------------------ B: double-form selectors

@pytest.mark.parametrize("n", N_B)
def test_double_form_selectors(n):
    c = case("A", 2, n)
    db, srv = c.server()
    for B in B_B:
        assert_members(c, run_group(c, srv, B), B)
    db.close()


# ------------------------------------------------------------------------------------------------------ C: head split

@functools.lru_cache(maxsize=None)
def without_head(d, n):
    """Replies of the groups of 2, 5 and 8 from a context with HEAD_MODE = 0."""
    c = case("A", d, n)
    db, srv = c.server(head_mode=0)
    out = {B: run_group(c, srv, B) for B in (2, 5, 8)}
    db.close()
    return out


@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("h", range(1, 9))
def test_head_split(h, d):
    """Levels [0, h) on the head stream, the rest on the lane: three batches back to back, so that the lane's two head
    slots are both used and the first is used again while the lane may still read it."""
    for n in (2 ** (h + 1) + 1, 1025):
        if d == 2 and n < 65:
            continue                        # ([8, n - 8] with the MFMA scan's column groups: part B's sizes)
        c = case("A", d, n)
        db, srv = c.server(head=h, head_mode=2)
        plain = without_head(d, n)
        for B in (2, 5, 8):
            walk = reported(srv, B, n, head_split=True)[1]
            assert [t[6] for t in walk] == [j < h for j in range(len(walk))], (h, n, B, walk)
            got = run_group(c, srv, B, head=h, runs=3)
            assert_members(c, got, B, what="head %d" % h)
            assert np.array_equal(got, plain[B]), (h, n, B)
        db.close()


# ---------------------------------------------------------------------------------------------------------- D and E

def representatives(ring, option, sizes):
    """One (n, B) per distinct walk that `option` gives the (n, B) of `sizes`: the smallest n, then the smallest B."""
    c = case(ring, 1, 16)
    db, srv = c.server(option)
    seen = {}
    for n, B in sorted(sizes):
        key = tuple(f["word"] & ~(1 << 15) for f in srv.expansion_forms(B, min(n, c.w.N)))
        if n > c.w.N:
            key += (-1,) + tuple(f["word"] & ~(1 << 15) for f in srv.expansion_forms(B, n - c.w.N))
        seen.setdefault(key, (n, B))
    db.close()
    return sorted(seen.values())


@pytest.mark.parametrize("option", OPTIONS)
def test_options(option, monkeypatch):
    """One option away from the defaults: every distinct walk of part A's sizes at d = 1 and of part B's at d = 2."""
    if option.startswith("PIRGPU_"):
        monkeypatch.setenv("PIRGPU_NTT_MODE", "0")      # (read when a context is created)
    ran = []
    for d, sizes in ((1, [(n, B) for n in N_A for B in GROUPS]), (2, [(n, B) for n in N_B for B in B_B])):
        reps = representatives("A", option, sizes)
        for n in sorted({n for n, _ in reps}):
            c = case("A", d, n)
            db, srv = c.server(option)
            for B in [B for m, B in reps if m == n]:
                assert_members(c, run_group(c, srv, B, option), B, what=option)
                ran.append((d, n, B))
            db.close()
    DONE.add(("D", option))
    print("%s: %d distinct walks run: %s" % (option, len(ran), ran))


@pytest.mark.parametrize("n", N_E)
def test_production_ring(n):
    """N = 4096, k = 2: members 0, B / 2 and B - 1 against the oracle, every member against the same context's
    single-query reply (which the oracle vouches for through those three)."""
    reps = [B for m, B in representatives("E", None, [(m, B) for m in N_E for B in GROUPS]) if m == n]
    c = case("E", 2, n)
    assert c.w.k == 2 and c.w.orc.N == 4096 and reps
    db, srv = c.server()
    single = []
    for i in range(8):
        srv.use_keyset(c.slots[i])
        single.append(srv.process_query(np.ascontiguousarray(c.query(i))))
    for B in reps:
        got = run_group(c, srv, B)
        assert_members(c, got, B, members=sorted({0, B // 2, B - 1}))
        for i in range(B):
            assert np.array_equal(got[i], single[i]), (n, B, i)
    db.close()
    DONE.add(("E", n))
    print("production ring, n = %d: %d distinct walks run: B = %s" % (n, len(reps), reps))


# ----------------------------------------------------------------------------------------------------------- coverage

def reachable(tmp_path, ring, sizes):
    exe = str(tmp_path / "expansion_plan_test")
    if not os.path.exists(exe):
        subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "cpp", "expansion_plan_test.cpp"), "-o", exe],
                       check=True)
    w = world(ring)
    r = subprocess.run([exe, "--reachable", str(w.N), str(w.k)] + [str(n) for n in sizes], capture_output=True, text=True,
                       check=True)
    out = {}
    for line in r.stdout.splitlines():
        setting, record = line.split(" : ")
        name, split = setting.rsplit(" split=", 1)
        f, *flags = record.split()
        out.setdefault((name, int(split)), set()).add(({"u": "unfused", "F": "fused", "N": "last_ntt", "C": "last_coeff"}[f],)
                                                      + tuple(x == "1" for x in flags))
    return out


def test_every_reachable_level_record_was_run(tmp_path, monkeypatch):
    """The union of the level records of the runs above against what the plan can produce at these rings for B = 1 .. 8
    and the sizes of the parts (every n of a ring with every option the ring is run with; the head splits with the
    defaults).  Runs the cases it needs that have not run in this process."""
    for n in N_A:
        if ("A", n) not in DONE:
            test_deep_sweep(n)
    for n in N_E:
        if ("E", n) not in DONE:
            test_production_ring(n)
    for option in OPTIONS:
        if ("D", option) not in DONE:
            test_options(option, monkeypatch)
            monkeypatch.undo()
    missing = {}
    for ring, sizes, options in (("A", sorted(set(N_A) | set(N_B) | {3}), ("default",) + OPTIONS), ("E", N_E, ("default",))):
        can = reachable(tmp_path, ring, sizes)
        for option in options:
            want = set().union(*[recs for (name, split), recs in can.items() if name == option])
            assert want, (ring, option)
            if want - RAN[(ring, option)]:
                missing[(ring, option)] = sorted(want - RAN[(ring, option)])
    assert not missing, missing
