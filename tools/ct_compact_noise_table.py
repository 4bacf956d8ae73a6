"""The noise table of DESIGN.md section 6.6 ("compact replies"), from the CPU models (tests/ctmult_model.py,
tests/modswitch_model.py, tests/reply_pack_model.py + the oracle): what switching the FINISHED reply of the
ciphertext-multiplication mode to r primes (PIRGPU_CREATE_CT_COMPACT_REPLY with result_primes = r) costs in invariant
noise budget, and what the reply weighs afterwards.  No GPU.

Per shape: PirSetup with data seed 42 and client seed 99, d = 2, one query; the reply of process_query_ct at k primes,
its budget there (noise_budget_level at level k), then for every r < k switch_residues(reply, q, r), its budget at level
r, whether decrypt_level + the string decoder recover the item, and the reply bytes: 8 * 2 k N now, 8 * ct_words(N, q, r)
switched and packed.

    python tools/ct_compact_noise_table.py [--quick]        (--quick: the N = 4096 rows only)"""
from __future__ import annotations

import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ctmult_model as C  # noqa: E402
import modswitch_model as M  # noqa: E402
import oracle  # noqa: E402
import reply_pack_model as rpm  # noqa: E402
from pir_fixtures import PirSetup  # noqa: E402

ROWS = [  # N, data prime bits (+ special; None: SEAL's default chain, [36, 36 | 37] at N = 4096, in ITS order of the
    # primes), plain bits, items, bits per coefficient (0: full width), index
    (4096, None, 16, 9, 10, 5),                       # correctness_test.cpp:99
    (4096, None, 16, 500, 6, 125),                    # correctness_test.cpp:100 (23 x 22)
    (8192, [43, 43, 44, 44, 44], 20, 9, 10, 5),
    (8192, [43, 43, 44, 44, 44], 42, 9, 0, 5),
]


def recovered(s, index, ct, r):
    p = s.params
    rc, data = oracle.string_decode(M.decrypt_level(s.client, ct, r), p.eff_bits_per_coeff, p.bytes_per_item,
                                    oracle.calculate_item_offset(index, p.items_per_plaintext, p.bytes_per_item))
    return rc == 0 and data == s.item(index)


def row(N, bits, plain_bits, items, bpc, index):
    t0 = time.time()
    s = PirSetup(items, 0, 2, N=N, plain_bits=plain_bits, bits_per_coeff=bpc,
                 moduli=None if bits is None else oracle.coeff_modulus_create(N, bits))
    p, k = s.params, s.orc.k
    q = [int(v) for v in s.orc.moduli[:k]]
    bits = [v.bit_length() for v in q] + [0]
    rk = C.relin_key(s.client)
    query = s.client.create_query_for(p, index)
    rc, reply = C.process_query_ct(s.orc, s.db_ntt, p.dimensions, query, s.galois_keys, rk)
    assert rc == 0 and reply.shape == (1, 2, k, N)
    full = M.noise_budget_level(s.client, reply[0], k)
    ok_full = recovered(s, index, reply[0], k)
    now = 8 * 2 * k * N
    rs = list(range(k - 1, 0, -1))
    budgets, oks, sizes = [], [], []
    for r in rs:
        sw = M.switch_residues(reply, q, r)
        budgets.append(M.noise_budget_level(s.client, sw[0], r))
        oks.append(recovered(s, index, sw[0], r))
        assert rpm.pack(sw, q).shape == (1, rpm.ct_words(N, q, r))
        sizes.append(8 * rpm.ct_words(N, q, r))
    print("| %d, %s | %d-bit | %d items (%d × %d), %s, index %d | %.2f (%s) | r = %s: %s | %s | %d (r = 0 packed: %d) → %s | (%.0f s)" %
          (N, bits[:-1], plain_bits, items, p.dimensions[0], p.dimensions[1],
           "%d bits per coefficient" % bpc if bpc else "full-width coefficients", index, full,
           "recovered" if ok_full else "NOT recovered", " / ".join(str(r) for r in rs),
           " / ".join("%.2f" % b for b in budgets), " / ".join("recovered" if ok else "NOT recovered" for ok in oks),
           now, 8 * rpm.ct_words(N, q, k), " / ".join(str(v) for v in sizes), time.time() - t0), flush=True)


def main():
    print("| ring, data primes (bits) | t | database, query | reply budget at k primes (bits) | budget after the switch (bits) | "
          "item after the switch | reply bytes now → switched and packed |")
    print("|---|---|---|---|---|---|---|")
    for r in ROWS:
        if "--quick" in sys.argv and r[0] != 4096:
            continue
        row(*r)
    return 0


if __name__ == "__main__":
    sys.exit(main())
