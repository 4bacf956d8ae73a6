"""The block split of an upper level in ciphertext-multiplication mode (post_scan_ctm_level): the
children of a level are multiplied in blocks of bj = max(1, cap / nq) children of every query of the group, cap = the
pairs the scratch holds (option CT_SCRATCH_MB, floored at 8 pairs), and ctm_accumulate_kernel carries a row's sum from
block to block, clips a block to the rows it touches and leaves the others alone.  With the default scratch (136 pairs at
N = 4096, k = 2) no level of the suite's shapes is ever split; here ct_scratch_mb = 1 gives cap = 8:

  1. one row, nq = 1, bj = 8: 10 children in the blocks {0 .. 7}, {8, 9} -- the carry;
  2. d = 3, a group of nq = 3, bj = 2: level 1 has 8 children in rows of 3 -- {0, 1}, {2, 3}, {4, 5}, {6, 7}: a block
     that straddles two rows, blocks that leave a row untouched, a last row that is short because the database ends
     there -- and level 0 has 3 children in {0, 1}, {2}: the carry in a group;
  3. d = 2, groups of nq = 8 and 1 under two clients' keys: bj = 1, one child of every query per block, and bj = 8.

Every shape is compared bit for bit with process_query_ct (tests/ctmult_model.py), then the same queries run on a
context with the default scratch: equal replies, and exactly one block per upper level and query or group there.  The
number of blocks is read from the counter option CT_BLOCKS, so that the split is observed and not inferred from the
sizing rule.  The scans are the int8-MFMA ones wherever a batch is to form groups (8 rows and more: the 64-bit scans
run every query of a batch on its own)."""
import numpy as np
import pytest

import test_gpu_ctmult as T
from gpu_helpers import chain

pytestmark = pytest.mark.gpu


def test_carry_within_one_row():
    """d = 2, 100 plaintexts in 10 x 10, one query for an item of row 9: blocks {0 .. 7} and {8, 9} of the one row.  A
    lost carry leaves the sum of the products 8 and 9 alone, which differs in its bits from the sum of all ten."""
    s, index, q, want = T.single_case(100, 2)
    assert s.params.dimensions == [10, 10] and index // 10 == 9
    db, srv = T.ct_server(s, ct_scratch_mb=1)
    got = srv.process_query(q)
    assert db.get_option("ct_blocks") == 2
    assert np.array_equal(got, want)
    db.close()
    db, srv = T.ct_server(s)
    assert np.array_equal(srv.process_query(q), got)
    assert db.get_option("ct_blocks") == 1
    db.close()


def test_blocks_across_rows_in_a_group_of_three():
    """d = 3, dims [3, 3, 2], 15 plaintexts at N = 2048 on two 27-bit primes (a model product costs a quarter of one at
    N = 4096; the scratch still holds 8 pairs): 8 row sums -- enough rows for the int8-MFMA scan, so the batch of 3 is one
    group -- in level-1 rows {0, 1, 2}, {3, 4, 5}, {6, 7}: the last is short, and plaintext 14 is alone in the last row
    sum.  bj = 8 / 3 = 2, which neither divides nor equals 3:

      level 1   {0, 1} row 0 | {2, 3} rows 0 and 1, row 0 carried | {4, 5} row 1 carried, rows 0 and 2 untouched |
                {6, 7} row 2, which ends there
      level 0   {0, 1} | {2} carried

    6 blocks for the group against 2 with the default scratch."""
    N = 2048
    s = T.setup(15, 3, N=N, moduli=[int(x) for x in chain(N, 27)])
    assert s.params.dimensions == [3, 3, 2] and s.params.num_pt == 15
    idx = [14, 7, 3]                                   # (14: the lone plaintext of the short last row)
    qs = np.stack([s.client.create_query_for(s.params, i) for i in idx])
    want = [T.expected(s, q) for q in qs]
    replies = []
    for mb, blocks in ((1, 6), (None, 2)):
        db, srv = T.ct_server(s, ct_scratch_mb=mb)
        assert srv.scan_info()["mfma"] == 1
        srv.set_concurrency(8)
        srv.stage_batch(qs)
        srv.run_batch()
        out = srv.fetch_batch()
        assert db.get_option("ct_blocks") == blocks, mb
        assert out.shape == (3, 1, 2, s.orc.k, N)
        for i in range(3):
            bad = np.argwhere(out[i] != want[i])
            assert bad.size == 0, "scratch %s, query %d: first mismatch at [ct, poly, residue, coefficient] = %s" % (
                mb, i, bad[:1].tolist())
        replies.append(out)
        db.close()
    assert np.array_equal(replies[0], replies[1])


def test_one_child_per_block_under_two_key_sets():
    """d = 2, 8 x 2 plaintexts, 9 queries alternating two clients' key sets (the batch of
    test_gpu_ctmult.test_batch_of_nine_under_two_clients_keys and its model replies; 8 rows because a batch forms groups
    on the int8-MFMA scan only): the group of 8 has bj = 1 -- 8 blocks of one child of every query, pair p under key
    p mod 8, every row sum carried seven times -- the group of 1 has bj = 8 and one block."""
    s, clients, qs, want = T.nine_case()
    assert s.params.dimensions == [8, 2]
    replies = []
    for mb, blocks in ((1, 9), (None, 2)):
        db, srv = T.ct_server(s, ct_scratch_mb=mb)
        assert srv.scan_info()["mfma"] == 1
        out = T.run_nine(srv, clients, qs)
        assert db.get_option("ct_blocks") == blocks, mb
        for i in range(9):
            assert np.array_equal(out[i], want[i]), "scratch %s, query %d of the batch" % (mb, i)
        replies.append(out)
        db.close()
    assert np.array_equal(replies[0], replies[1])
