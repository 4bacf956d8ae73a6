// options.h -- every option pirgpu_set_option / pirgpu_get_option know, declared once.  Host only: no HIP, no context.
#pragma once
// One row per option: name (upper case; the environment variable is PIRGPU_<NAME>), kind, description.  The row makes the
// id OPT_<NAME> that the readers in ctx.hip use, so a read cannot name an option the table lacks.  DESIGN.md section 6
// has the same rows as a table with the defaults (tests/test_options_registry.py holds the two together).
//
// Kinds:
//   Early    shapes the workspace: refused (FailedPrecondition) once the context has been used
//   Live     accepted at any time; the context resolves it into a field when the workspace is built and at every set
//   Counter  not a choice: get returns a running count of the context, set overwrites it (negative: 0); the
//            environment plays no part
//
// A value is resolved in this order: set by name, else PIRGPU_<NAME> in the environment (honoured only with
// PIRGPU_ALLOW_ENV=1, env_gate.h; an empty string counts as unset), else the default the READER gives.  Values are stored
// raw; clamping is the reader's business.
//
// Not options -- environment only, read through pirgpu_env by ctx.hip when a context is created: PIRGPU_NTT_MODE (the
// arithmetic flavour of the transforms) and PIRGPU_F64_LAZY_INV (0 turns the lazy inverse transform of the fp64 flavours
// off).
#include <stdint.h>
#include <stdlib.h>

#include "env_gate.h"

namespace pirgpu {

enum class OptKind : uint8_t { Early, Live, Counter };

// clang-format off
#define PIRGPU_OPTIONS(X)                                                                                              \
  X(UPPER_BLOCKS, Early,                                                                                               \
    "target workgroup count of upper_fused_kernel; its chunk partial sums are sized by it (at least 1)")              \
  X(UPPER_BLOCKS_BATCH, Early,                                                                                         \
    "the same per query in batch mode, where other queries fill the chip too: fewer chunks = fewer partial sums to "  \
    "write and fold (at most UPPER_BLOCKS: the scratch is sized for that)")                                           \
  X(SCAN_LIMB, Early,                                                                                                  \
    "64-bit scan kernels: 28-bit limb accumulators when all data moduli are below 2^50; 0 forces the generic "        \
    "128-bit accumulators")                                                                                           \
  X(SCAN_MQ_SINGLE, Early,                                                                                             \
    "0 routes single queries through scan_kernel instead of the LDS-shared scan_mq_kernel")                           \
  X(SCAN_ROWS, Early, "64-bit scan kernels: rows accumulated per thread (1, 2, 3, 4, 6, 8)")                          \
  X(SCAN_BLOCK, Early, "64-bit scan kernels: workgroup size (64 .. 256)")                                             \
  X(SCAN_NSPLIT, Early,                                                                                                \
    "64-bit scan kernels: column splits (partial sums reduced by reduce_splits_kernel); by default the columns are "  \
    "split only when whole rows cannot fill the chip (d = 1 / few rows)")                                             \
  X(FUSE_LAST, Early, "last expansion level fused with the selector NTT; 0: off")                                     \
  X(FUSE_MAC_COMBINE, Early,                                                                                           \
    "levels below the last: combine step inside the data residues' MAC + inverse-NTT kernel; 0: a separate "          \
    "ks_combine pass")                                                                                                \
  X(LAST_NTT, Early, "the fused last expansion level is carried out in the NTT domain; 0: coefficient form")          \
  X(C0_NTT, Early,                                                                                                     \
    "c0 of the expansion tree in NTT form from the first fused level on (needs the fused levels and the NTT-domain "  \
    "last level; fp64 flavours).  0: off (the default: measured -4 % as two launches, -7.6 % as one kernel, "         \
    "profiles/r06_ab_c0_ntt_*.txt), 1: both components of a level in one kernel, 2: component 0 as a launch of its "  \
    "own")                                                                                                            \
  X(SEL_F64, Early,                                                                                                    \
    "batch lanes keep their selectors as exact doubles between the last expansion level and their two consumers "     \
    "(sel_pack, upper level): no u64 round trip (fp64 flavours, MFMA scan, NTT-domain last level); 0: off")           \
  X(TREE40, Early, "expansion tree between fused wide levels as packed polynomials; 0: doubles")                      \
  X(SPLIT_UPPER, Early,                                                                                                \
    "upper level as transform-to-scratch + elementwise MAC.  Default: on from N = 16384 in the fp64 flavours, "       \
    "where the fused kernel spills; never in the integer flavour below N = 32768, always at N = 32768 (that "         \
    "degree's table has no upper_fused)")                                                                             \
  X(SPLIT_UPPER_MB, Early, "megabytes of scratch of the split upper level per lane / worker")                         \
  X(PACK40, Early, "key-switch digits and products stored packed instead of as doubles / u64; 0: off")                \
  X(PACK_BYTES, Early,                                                                                                 \
    "packed storage of the key-switch intermediates: the fp64 flavours store x + q (|x| <= q) in the fewest whole "   \
    "bytes -- 5 for q < 2^39, 6 for q < 2^47 (cfg 4: 43 / 44 bits), 7 for q < 2^55 (cfg 5: 48 / 49 bits) -- "         \
    "instead of doubles; the integer flavour knows the 5-byte form only.  5 | 6 | 7 forces a (sufficient) width, "    \
    "8 = doubles; N = 32768 always keeps u64")                                                                        \
  X(TREE40_WIDE, Early,                                                                                                \
    "1 keeps the packed tree at N >= 16384 with 7-byte residues too.  Default 0: the combine kernel that also reads " \
    "and writes the TREE packed needs 68 bytes of scratch under the 128-register cap of a 1024-thread workgroup -- "  \
    "the tree stays in doubles there, digits and products are packed")                                                \
  X(SCAN_MFMA, Early, "0 keeps the 64-bit multiply-accumulate kernels for d >= 2 as well")                            \
  X(SCAN_MFMA_WIDE, Early,                                                                                             \
    "0 / 1 forces the 8-wave / 4-wave (one wave per SIMD, up to 7 k-steps) scan kernel; unset: chosen by the "        \
    "matrix width")                                                                                                   \
  X(SCAN_MFMA_TOP4, Early,                                                                                             \
    "0 keeps the top digit of database and selectors as a full byte instead of a nibble (scan_mfma.hip TOP4)")        \
  X(SCAN_MFMA_NQ, Early, "queries per database pass of the MFMA scan in batch mode (1 .. 8)")                         \
  X(SCAN_MFMA_SINGLE, Early,                                                                                           \
    "single queries use the MFMA scan too.  Default: only on a matrix of one column chunk -- a single query on a "    \
    "wider matrix pays the partial-sum round trip for one query only; there the 64-bit kernels on the u64 copy are "  \
    "faster (cfg 4: 5.6 vs 6.4 ms).  Always on with a streamed database, which has no u64 copy")                      \
  X(HEAD_LEVELS, Early,                                                                                                \
    "expansion levels of a batch group that run ahead on the head stream (0: none, at most 8)")                       \
  X(HEAD_MODE, Early,                                                                                                  \
    "when the head stream is used: 0 never, 1 batches staged with pirgpu_batch_stage_async, 2 always")                \
  X(SCAN_F64_FOLD, Early,                                                                                              \
    "fp64 fold of the scan's digit diagonals (moduli below 2^50).  Default: on from 6 digits per residue (cfg 4: "    \
    "scan 4.53 against 4.76 ms, cfg 5: 8.33 against 8.57, same box); at 5 digits (cfg 3) the single-query pass "      \
    "measured 3 % slower with it (0.212 against 0.206 ms) and the batch step 0.5 % faster: off")                      \
  X(SCAN_F64_FOLD_BATCH, Early,                                                                                        \
    "the same choice for the launches that serve a GROUP of queries (batch pipeline on part of the chip, "            \
    "slot-sharded step): on whenever the moduli allow -- with 16 result columns per tile instead of 2 the fold is "   \
    "8 x the work per database byte, and there the cheaper fold pays at 5 digits too (round 6, same box, three "      \
    "alternating runs: 5 362 / 5 426 / 5 363 against 5 322 / 5 331 / 5 319 queries/s; "                               \
    "profiles/r06_ab_scan_store_fold.txt)")                                                                           \
  X(LOOP_TRANSFORMS, Early,                                                                                            \
    "the digit kernel of the wide expansion levels and the transform kernel of the split upper level run all "        \
    "transforms of one source polynomial in ONE workgroup: one load and one permutation per source, stores drain "    \
    "under the next transform (fp64 flavours); 0: one transform per workgroup everywhere")                            \
  X(DB_STREAM_MB, Early,                                                                                               \
    "streamed database: megabytes of encoded plaintexts per load chunk, rounded down to whole row bands (at least "   \
    "one)")                                                                                                           \
  X(CT_SCRATCH_MB, Early,                                                                                              \
    "ciphertext-multiplication mode: megabytes of product scratch per worker / lane; the children of a level are "    \
    "multiplied in blocks that fit it (at least one child of every query of a group)")                                \
  X(CT_SHARED_SEL, Early,                                                                                              \
    "ciphertext-multiplication mode: 1 = the selectors of a level, the same for every row and plane, are lifted and " \
    "transformed once per level and group and only the ciphertext half of a pair per block (ctmult_shared.hip); "     \
    "0 = all four polynomials of every pair.  Default: 1 on a context with wide items, 0 elsewhere -- and get "       \
    "reports that default, not -1")                                                                                   \
  X(SCAN_MFMA_WGS_BATCH, Live,                                                                                         \
    "persistent workgroups (= CUs) of a database pass of the MFMA scan that shares the chip with another group "      \
    "(batch pipeline); 0 = all CUs")                                                                                  \
  X(SLOTS_SCAN_WGS, Live,                                                                                              \
    "slot-sharded step: workgroups of its database pass, which shares the chip with the other lane's expansion "      \
    "like the single-GPU batch pass; 0 = one per CU.  Unset: follows SCAN_MFMA_WGS_BATCH")                            \
  X(SLOTS_GATHER_NTT, Live,                                                                                            \
    "slot-sharded step: the inverse transform of the row sums gathers them from the ranks' blocks of the receive "    \
    "buffer; 0: a separate assembly pass, then the plain in-place transform")                                         \
  X(SLOTS_SCAN_BLK_MAJOR, Live,                                                                                        \
    "slot-sharded step: scan units in (slot block, group) order: the workgroups running side by side then read the "  \
    "same database tiles for different groups -- the launch was 6 % (cfg 3) / 11 % (cfg 4) shorter than with one "    \
    "sweep of the slots per group, the step 1.2 - 1.5 %")                                                             \
  X(TABLES_ONE_LAUNCH, Live,                                                                                           \
    "contexts with tables: 0 = one database-pass launch per run of equal tables instead of one per group (A/B)")      \
  X(CT_ROWSUM_SPLITS, Live,                                                                                            \
    "deferred rounding (A/B, tests): at most this many workgroups share a row's children; 1: never split; 0: "        \
    "chosen by the grid size")                                                                                        \
  X(SCAN_LAUNCHES, Counter, "the database-pass launches the batch pipeline queued so far")                            \
  X(CT_BLOCKS, Counter,                                                                                                \
    "the product blocks the upper levels of the ciphertext-multiplication mode queued so far (one per level and "     \
    "query or group when the level's children fit CT_SCRATCH_MB)")                                                    \
  X(UPPER_PARTS, Counter,                                                                                              \
    "the parts the upper recursion levels cut a row's children into so far -- chunks of the fused kernel (their "     \
    "sums meet in reduce_splits_kernel) or blocks of the split form (carried in `acc`), counted once per level and "  \
    "query or group")                                                                                                 \
  X(CT_RELINS, Counter,                                                                                                \
    "the ciphertexts the levels of the ciphertext-multiplication mode have key-switched so far -- one per pair, or "  \
    "(deferred rounding) one per row and query")                                                                      \
  X(CT_LIFTS, Counter,                                                                                                 \
    "the polynomials those levels have lifted to the auxiliary base so far -- 4 per pair, or (CT_SHARED_SEL) 2 per "  \
    "pair and 2 dims[l] per query, level and group; the hooks pirgpu_ct_multiply and pirgpu_ct_multiply_sum count "   \
    "the same way, 2 per selector of the call")
// clang-format on

enum OptId : int {
#define PIRGPU_OPT_ID(name, kind, doc) OPT_##name,
  PIRGPU_OPTIONS(PIRGPU_OPT_ID)
#undef PIRGPU_OPT_ID
  OPT_COUNT
};

struct OptRow {
  const char* name;   // upper case
  const char* env;    // "PIRGPU_" + name
  OptKind kind;
  const char* doc;
};

inline constexpr OptRow kOptRows[] = {
#define PIRGPU_OPT_ROW(name, kind, doc) {#name, "PIRGPU_" #name, OptKind::kind, doc},
    PIRGPU_OPTIONS(PIRGPU_OPT_ROW)
#undef PIRGPU_OPT_ROW
};
static_assert(sizeof(kOptRows) / sizeof(kOptRows[0]) == OPT_COUNT && OPT_COUNT == 42, "one row per option");

// The option a caller names, in any letter case; OPT_COUNT: no such option.
inline OptId find_option(const char* name) {
  auto upper = [](char ch) { return ch >= 'a' && ch <= 'z' ? (char)(ch - 'a' + 'A') : ch; };
  for (int id = 0; id < OPT_COUNT; ++id) {
    const char *a = name, *b = kOptRows[id].name;
    while (*a && upper(*a) == *b) ++a, ++b;
    if (!*a && !*b) return (OptId)id;
  }
  return OPT_COUNT;
}

// What one context was given by name, and its counters.
class OptionStore {
 public:
  // Early / Live: the value set by name, else the environment's, else dflt; *present: one of the first two.
  int64_t value(OptId id, int64_t dflt, bool* present = nullptr) const {
    if (present) *present = true;
    if (given_[id]) return v_[id];
    const char* e = pirgpu_env(kOptRows[id].env);
    if (e && *e) return strtoll(e, nullptr, 10);
    if (present) *present = false;
    return dflt;
  }
  // Counter: the running count.
  int64_t& counter(OptId id) { return v_[id]; }

  // pirgpu_set_option / pirgpu_get_option on a known id (unset: the caller's `unset`, -1 for "the built-in default")
  void set(OptId id, int64_t value) {
    v_[id] = kOptRows[id].kind == OptKind::Counter && value < 0 ? 0 : value;
    given_[id] = true;
  }
  int64_t get(OptId id, int64_t unset = -1) const {
    return kOptRows[id].kind == OptKind::Counter ? v_[id] : value(id, unset);
  }

 private:
  int64_t v_[OPT_COUNT] = {};
  bool given_[OPT_COUNT] = {};
};

}  // namespace pirgpu
