"""Seed-compressed key objects expanded on the device: the kernel behind pirgpu_expand_seeds
and pirgpu_keyset_set_keys_seeded against the two host restatements of SEAL's BlakePRNG + sample_poly_uniform -- the
server's own (pirgpu_wire_sample_poly_uniform) and the tests' independent one (seal_wire.sample_poly_uniform) --, with
moduli that reject nothing, moduli that reject one draw in eight on every data residue (so every later residue starts
mid-block, hundreds of candidates late), chains that mix the two, and the wire path that uses it."""
import ctypes as C

import numpy as np
import pytest

import oracle
import pir_amd
import seal_wire as W
from pir_amd import capi, parameters as P
from gpu_helpers import chain_low, random_ct, random_key, to_product_params
from pir_fixtures import PirSetup, generate_test_db

pytestmark = pytest.mark.gpu

SEEDS = [bytes(range(64)), bytes(64), bytes(range(64, 128)), bytes([255 - i for i in range(64)]), b"seed-expand".ljust(64, b"\x5a")]
MAX_RANDOM = 0x7FFFFFFFFFFFFFFF


def host_sample(seed, moduli, N):
    lib = capi.load()
    lib.pirgpu_wire_sample_poly_uniform.argtypes = [C.c_char_p, C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32,
                                                    C.POINTER(C.c_uint64)]
    lib.pirgpu_wire_sample_poly_uniform.restype = None
    out = np.empty((len(moduli), N), dtype=np.uint64)
    lib.pirgpu_wire_sample_poly_uniform(seed, (C.c_uint64 * len(moduli))(*moduli), len(moduli), N,
                                        out.ctypes.data_as(capi.u64p))
    return out


def model_rejections(seed, moduli, N):
    """Draws the Python model rejects per modulus (the model's own loop, counting)."""
    rng, rej = W.SealPrng(seed), []
    for q in moduli:
        max_multiple, n, r = MAX_RANDOM - MAX_RANDOM % q - 1, 0, 0
        while n < N:
            a, b = rng.u32(), rng.u32()
            if ((a << 31) | (b >> 1)) < max_multiple:
                n += 1
            else:
                r += 1
        rej.append(r)
    return rej


def bare_server(N, moduli, plain_bits=20):
    """A context over this chain with no database and no keys: the hook needs the key-level moduli alone."""
    p = oracle.create_pir_parameters(4, 0, 1, N=N, plain_bits=plain_bits, moduli=[int(m) for m in moduli])
    pp = to_product_params(p)
    db = pir_amd.PIRDatabase.Create(pp)
    return db, pir_amd.PIRServer(db, pp)


# ---------------------------------------------------------------- 1. the hook, no rejections

@pytest.mark.parametrize("N,moduli,plain_bits", [(2048, oracle.coeff_modulus_create(2048, [27, 27]), 14),
                                                 (4096, oracle.BFV_DEFAULT[4096], 20)], ids=["2048-k1", "4096-k2"])
def test_hook_equals_the_host_sampler_without_rejections(N, moduli, plain_bits):
    db, srv = bare_server(N, moduli, plain_bits)
    before = srv.keyset_seed_stats()
    got = srv.expand_seeds(SEEDS)
    for i, seed in enumerate(SEEDS):
        assert np.array_equal(got[i], host_sample(seed, moduli, N)), i
        assert np.array_equal(got[i], W.sample_poly_uniform(seed, moduli, N)), i
    after = srv.keyset_seed_stats()
    assert after["rejected"] == before["rejected"]          # 27- and 36-bit primes reject about q draws in 2^63: none here
    assert after["objects"] == before["objects"] + len(SEEDS)
    db.close()


# ---------------------------------------------------------------- 2. rejections on every data residue

def test_hook_with_rejections_on_every_data_residue():
    """Two data primes just above 2^60: 2^63 - 1 = 7 q + r with r just below q, so one draw in eight is rejected and
    the residues after the first start hundreds of candidates late, mid-block."""
    N = 4096
    moduli = [int(m) for m in chain_low(N, 61)]
    seeds = SEEDS[:3]
    rej = [model_rejections(s, moduli, N) for s in seeds]
    for r in rej:                       # a condition on the inputs, not on the code under test
        assert r[0] > 0 and r[1] > 0, rej
    assert rej[0] == [637, 610, 0]      # seed bytes(range(64)): the figures the Python model gives ...
    assert (N + 637) % 8 and (2 * N + 637 + 610) % 8        # ... residues 1 and 2 start inside a 64-byte block
    db, srv = bare_server(N, moduli)
    want = [host_sample(s, moduli, N) for s in seeds]
    for s, w in zip(seeds, want):
        assert np.array_equal(w, W.sample_poly_uniform(s, moduli, N))
    for s, w, r in zip(seeds, want, rej):
        before = srv.keyset_seed_stats()["rejected"]
        assert np.array_equal(srv.expand_seeds([s])[0], w)
        assert srv.keyset_seed_stats()["rejected"] == before + sum(r)
    # two objects in one call: each walks its own positions
    before = srv.keyset_seed_stats()["rejected"]
    got = srv.expand_seeds([seeds[1], seeds[2]])
    assert np.array_equal(got[0], want[1]) and np.array_equal(got[1], want[2])
    assert srv.keyset_seed_stats()["rejected"] == before + sum(rej[1]) + sum(rej[2])
    db.close()


# ---------------------------------------------------------------- 3. moduli of different sizes

@pytest.mark.parametrize("bits", [[61, 36], [36, 61]], ids=["rejecting-first", "rejecting-second"])
def test_hook_when_the_moduli_differ_in_size(bits):
    """max_multiple switches exactly at the boundary between a rejecting and a non-rejecting modulus."""
    N = 4096
    moduli = [int(m) for m in chain_low(N, bits)]
    seeds = SEEDS[:2]
    rej = [model_rejections(s, moduli, N) for s in seeds]
    big = bits.index(61)
    for r in rej:
        assert r[big] > 0 and r[1 - big] == 0, rej
    db, srv = bare_server(N, moduli)
    before = srv.keyset_seed_stats()["rejected"]
    got = srv.expand_seeds(seeds)
    for i, s in enumerate(seeds):
        assert np.array_equal(got[i], host_sample(s, moduli, N)), i
        assert np.array_equal(got[i], W.sample_poly_uniform(s, moduli, N)), i
    assert srv.keyset_seed_stats()["rejected"] == before + sum(sum(r) for r in rej)
    db.close()


# ---------------------------------------------------------------- 4. set_keys_seeded equals set_keys

@pytest.mark.parametrize("N,moduli,plain_bits", [(2048, oracle.coeff_modulus_create(2048, [27, 27]), 14), (4096, None, 20)],
                         ids=["2048-k1", "4096-k2"])
def test_seeded_install_equals_expanded_install(N, moduli, plain_bits):
    s = PirSetup(10, 0, 1, N=N, plain_bits=plain_bits, moduli=moduli)
    pp = to_product_params(s.params)
    db = pir_amd.PIRDatabase.Create(pp)
    db.populate(s.raw)
    srv = pir_amd.PIRServer.Create(db, pp)
    k, km = s.orc.k, s.orc.k + 1
    rng = np.random.default_rng(N)
    elts = sorted(s.galois_keys)
    keys, seeded = {}, {}
    for g in elts:
        key = random_key(s.orc, rng)
        seeds = [rng.integers(0, 256, 64, dtype=np.uint8).tobytes() for _ in range(k)]
        for j in range(k):
            key[j, 1] = host_sample(seeds[j], [int(m) for m in s.orc.moduli[:km]], N)
        keys[g] = key
        seeded[g] = (np.ascontiguousarray(key[:, 0]), b"".join(seeds))
    up0 = srv.keyset_stats()["key_uploads"]
    slot_a = srv.install_keyset(b"expanded", keys)
    up1 = srv.keyset_stats()["key_uploads"]
    slot_b = srv.install_keyset_seeded(b"seeded", seeded)
    up2 = srv.keyset_stats()["key_uploads"]
    assert slot_a != slot_b
    assert up1 - up0 == len(elts) and up2 - up1 == len(elts)
    assert srv.keyset_seed_stats()["objects"] == len(elts) * k
    ct = random_ct(s.orc, rng)[0]
    for g in elts:
        srv.use_keyset(slot_a)
        a = srv.substitute_power_x_inplace(ct.copy(), g)
        srv.use_keyset(slot_b)
        b = srv.substitute_power_x_inplace(ct.copy(), g)
        assert np.array_equal(a, b), g
    n = 8
    rc, want = s.orc.oblivious_expansion(ct, n, keys)
    assert rc == 0
    got_b = srv.oblivious_expansion(ct, n)
    srv.use_keyset(slot_a)
    got_a = srv.oblivious_expansion(ct, n)
    assert np.array_equal(got_a, want) and np.array_equal(got_b, want)
    srv.use_keyset(0)
    db.close()


# ---------------------------------------------------------------- 5. the wire, end to end

def _fields(request):
    f = W._parse(request)
    return [p for n, p in f if n == 1], [p for n, p in f if n == 2], [p for n, p in f if n == 3]


def _objects(blob, k):
    """Key objects (entries x digits) a serialized GaloisKeys / RelinKeys holds."""
    (dim1,) = np.frombuffer(blob, dtype="<u8", count=1, offset=48)
    off, n = 56, 0
    for _ in range(int(dim1)):
        (dim2,) = np.frombuffer(blob[off:off + 8], dtype="<u8")
        off += 8
        for _ in range(int(dim2)):
            (size,) = np.frombuffer(blob[off + 8:off + 16], dtype="<u8")
            off += int(size)
            n += 1
    return n


def _wire_setup(ct_multiplication=False):
    enc = P.generate_encryption_params(4096, 16 if ct_multiplication else 24)
    if ct_multiplication:
        pp = P.create_pir_parameters(256, 0, 2, enc, True, 6)   # 6 bits per coefficient: the reference tuple's at 500 items
    else:
        pp = P.create_pir_parameters(256, 288, 2, enc)
    raw = generate_test_db(256, pp.bytes_per_item)
    return pp, raw


def _fresh_server(pp, raw, ct_multiplication=False):
    db = pir_amd.PIRDatabase.Create(pp, raw, ct_multiplication=True) if ct_multiplication else pir_amd.PIRDatabase.Create(pp, raw)
    return db, pir_amd.PIRServer.Create(db, pp)


def test_wire_seeded_request_takes_the_device_path(monkeypatch):
    pp, raw = _wire_setup()
    k = len(pp.encryption_parameters.coeff_modulus) - 1
    client = pir_amd.PIRClient.Create(pp, seed=b"seed-expand")
    idx = [3, 200]
    queries = [client.create_query_for(i) for i in idx]
    seeded = client.SaveRequest(queries)
    client.set_seeded_keys(False)
    expanded = client.SaveRequest(queries)
    client.set_seeded_keys(True)
    _, g_seeded, relin = _fields(seeded)
    _, g_expanded, _ = _fields(expanded)
    n_obj = _objects(bytes(g_seeded[0]), k)
    assert n_obj >= k

    db, srv = _fresh_server(pp, raw)
    r_seeded = srv.ProcessRequest(seeded)
    assert srv.keyset_seed_stats()["objects"] == n_obj
    assert client.ProcessResponse(idx, r_seeded) == [raw[i].tobytes() for i in idx]
    assert srv.ProcessRequest(expanded) == r_seeded           # the expanded twin of the same keys: the host path
    assert srv.keyset_seed_stats()["objects"] == n_obj
    db.close()

    # a mixed set (the first object expanded, the others seeded) is the host's
    mixed = _mixed_blob(bytes(g_seeded[0]), bytes(g_expanded[0]), min(_entry_spans(bytes(g_seeded[0]))))
    db, srv = _fresh_server(pp, raw)
    mixed_request = b"".join(W._field(1, bytes(x)) for x in _fields(seeded)[0]) + W._field(2, mixed) + W._field(3, bytes(relin[0]))
    assert srv.ProcessRequest(mixed_request) == r_seeded
    assert srv.keyset_seed_stats() == {"objects": 0, "rejected": 0}
    db.close()

    # the switch: off on a fresh context
    monkeypatch.setenv("PIRGPU_ALLOW_ENV", "1")
    monkeypatch.setenv("PIRGPU_WIRE_SEED_EXPAND", "0")
    db, srv = _fresh_server(pp, raw)
    assert srv.ProcessRequest(seeded) == r_seeded
    assert srv.keyset_seed_stats()["objects"] == 0
    db.close()


def _entry_spans(blob):
    """{index: (begin, end)} of the present entries' PublicKey objects inside a serialized KSwitchKeys."""
    (dim1,) = np.frombuffer(blob, dtype="<u8", count=1, offset=48)
    off, spans = 56, {}
    for index in range(int(dim1)):
        (dim2,) = np.frombuffer(blob[off:off + 8], dtype="<u8")
        off += 8
        begin = off
        for _ in range(int(dim2)):
            (size,) = np.frombuffer(blob[off + 8:off + 16], dtype="<u8")
            off += int(size)
        if dim2:
            spans[index] = (begin, off)
    return spans


def _mixed_blob(seeded, expanded, index):
    """The seeded object with entry `index` replaced by its expanded form."""
    s, e = _entry_spans(seeded), _entry_spans(expanded)
    body = seeded[16:s[index][0]] + expanded[e[index][0]:e[index][1]] + seeded[s[index][1]:]
    return W.header(16 + len(body)) + body


def test_wire_relin_key_of_a_ct_multiplication_context():
    pp, raw = _wire_setup(ct_multiplication=True)
    k = len(pp.encryption_parameters.coeff_modulus) - 1
    client = pir_amd.PIRClient.Create(pp, seed=b"seed-expand-ct")
    idx = [1, 5]
    queries = [client.create_query_for(i) for i in idx]
    seeded = client.SaveRequest(queries)
    client.set_seeded_keys(False)
    expanded = client.SaveRequest(queries)
    _, g, relin = _fields(seeded)
    n_obj = _objects(bytes(g[0]), k) + _objects(bytes(relin[0]), k)
    db, srv = _fresh_server(pp, raw, True)
    r = srv.ProcessRequest(seeded)
    assert srv.keyset_seed_stats()["objects"] == n_obj         # Galois keys and the relinearisation key
    assert client.ProcessResponse(idx, r) == [raw[i].tobytes() for i in idx]
    db.close()
    db, srv = _fresh_server(pp, raw, True)
    assert srv.ProcessRequest(expanded) == r
    assert srv.keyset_seed_stats()["objects"] == 0
    db.close()


# ---------------------------------------------------------------- 6. a coefficient out of range

def test_wire_seeded_set_with_a_coefficient_equal_to_its_modulus():
    pp, raw = _wire_setup()
    client = pir_amd.PIRClient.Create(pp, seed=b"seed-expand-bad")
    request = client.CreateRequest([7])
    q, g, relin = _fields(request)
    blob = bytearray(bytes(g[0]))
    begin = min(b for b, _ in _entry_spans(bytes(blob)).values())
    word = begin + 16 + 16 + 32 + 33 + 16 + 8          # PublicKey header, Ciphertext header, parms_id, members, IntArray header, count
    assert int.from_bytes(blob[word - 8:word], "little") == 3 * 4096      # the seeded form: c0 alone
    blob[word:word + 8] = int(pp.encryption_parameters.coeff_modulus[0]).to_bytes(8, "little")
    bad = b"".join(W._field(1, bytes(x)) for x in q) + W._field(2, bytes(blob)) + W._field(3, bytes(relin[0]))
    db, srv = _fresh_server(pp, raw)
    resident = srv.keyset_stats()["resident"]
    with pytest.raises(pir_amd.PirGpuError) as e:
        srv.ProcessRequest(bad)
    assert e.value.code == pir_amd.StatusCode.INVALID_ARGUMENT
    assert "ciphertext data is invalid (coefficient out of range)" in e.value.message
    assert srv.keyset_stats()["resident"] == resident
    assert srv.keyset_seed_stats()["objects"] == 0
    assert client.ProcessResponse([7], srv.ProcessRequest(request)) == [raw[7].tobytes()]
    db.close()
