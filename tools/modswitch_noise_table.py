"""The noise table of DESIGN.md section 6.4, from the CPU model (tests/modswitch_model.py + the oracle): what switching
every level result to r primes costs in invariant noise budget.  No GPU.

Per row: a database of full-plaintext items (d = 2), the query for plaintext num_pt - 2 from the oracle's client, the
budget of the selected row's level-1 ciphertext and the smallest budget over the reply, at the full modulus
(oracle.db_multiply) and switched (multiply_switched), and whether the model's client recovers the item.

    python tools/modswitch_noise_table.py [--quick]        (--quick: the N = 4096 rows only)"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import modswitch_model as M  # noqa: E402
import oracle  # noqa: E402
from pir_fixtures import PirSetup  # noqa: E402

ROWS = [  # N, data prime bits (+ special), plaintexts, plain bits, r
    (4096, [36, 36, 37], 100, 24, 1),
    (4096, [36, 36, 37], 1640, 24, 1),            # 41 x 40: the plaintext count of the reference's 2^16-item benchmark
    (4096, [36, 36, 37], 100, 20, 1),
    (4096, [36, 36, 37], 100, 16, 1),
    (8192, [43, 43, 44, 44], 100, 24, 1),         # cfg 4's chain
    (8192, [43, 43, 44, 44], 100, 24, 2),
    (16384, [48, 48, 48, 49, 49], 81, 24, 1),     # cfg 5's chain
    (16384, [48, 48, 48, 49, 49], 81, 24, 2),
]


def row(N, bits, n_pt, plain_bits, r):
    t0 = time.time()
    s = PirSetup(n_pt, 0, 2, N=N, plain_bits=plain_bits, moduli=oracle.coeff_modulus_create(N, bits))
    p = s.params
    index = p.num_pt - 2
    q = s.client.create_query_for(p, index)
    rc, sv = s.orc.oblivious_expansion_multi(q, p.dim_sum, s.galois_keys)
    assert rc == 0
    k, cols = s.orc.k, p.dimensions[1]
    sel = index // cols
    trace_full, trace = [], []
    full = M.multiply_switched(s.orc, s.db_ntt, p.dimensions, sv, k, trace=trace_full)      # r = k: the oracle's multiply
    rc, want = s.orc.db_multiply(s.db_ntt, p.dimensions, sv.copy())
    assert rc == 0 and np.array_equal(full, want)
    reply = M.multiply_switched(s.orc, s.db_ntt, p.dimensions, sv, r, trace=trace)
    l1 = (s.client.noise_budget(trace_full[0][sel][0]), M.noise_budget_level(s.client, trace[0][sel][0], r))
    rep = (min(s.client.noise_budget(c) for c in full), min(M.noise_budget_level(s.client, c, r) for c in reply))
    pt = M.process_reply_level(s.client, 2, reply, r)
    rc, data = oracle.string_decode(pt, p.eff_bits_per_coeff, p.bytes_per_item, 0)
    ok = rc == 0 and data == s.item(index)
    E, Er = 2 * s.orc.expansion_ratio(), 2 * M.expansion_ratio_level(s.orc, r)
    print("| %d, %s | %d-bit | %d × %d | %d | %d → %d | %.1f → %.1f | %.1f → %.1f | %s | (%.0f s)" %
          (N, bits[:-1], plain_bits, p.dimensions[0], p.dimensions[1], r, E, Er, l1[0], l1[1], rep[0], rep[1],
           "yes" if ok else "NO", time.time() - t0), flush=True)


def main():
    print("| ring, data primes (bits) | t | dims | r | E → E' | level-1 budget, full → switched (bits) | reply budget, full → "
          "switched (bits) | item recovered |")
    print("|---|---|---|---|---|---|---|---|")
    for r in ROWS:
        if "--quick" in sys.argv and r[0] != 4096:
            continue
        row(*r)
    return 0


if __name__ == "__main__":
    sys.exit(main())
