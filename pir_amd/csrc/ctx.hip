// ctx.hip -- device context and C ABI of libpirgpu (see include/pirgpu.h).
//
// Host-side orchestration of the reference's PIRServer::processQuery
// (server.cpp:173-195) and PIRDatabase (database.cpp) on one MI355X: the encoded
// database, the Galois keys and every intermediate live in HBM; the host only
// sequences kernel launches on the context's stream.
//
// Map of this file (search for "[n]"):
//   [1]  state: Worker (one query in flight), BatchLane (a group of 8), KeySet, BatchSet, pirgpu_ctx
//   [2]  helpers: errors, NTT / Encode tables, workspace geometry; resolve_options turns the options (declared once, in
//        options.h) into the context's fields
//   [3]  oblivious expansion: expand_core (levels: ks_digit -> ks_mac_intt -> ks_mac_combine / ks_combine; last level
//        in the NTT domain), expand_query_to_sv
//   [4]  multiply: scan_group_mfma / scan_pair_mfma / scan_on_device, post_scan_stage (inverse NTT, upper levels, fold)
//   [5]  C ABI: create / destroy, options, database loading (db_encode, db_pack), finalize
//   [6]  C ABI: Galois keys, per-client key sets (handles with generations, pins, LRU)
//   [7]  C ABI: single query, join / fork, test hooks
//   [8]  batch pipeline: staging, lanes and what every walk over groups shares (claim_lane, LaneStage, queue_download),
//        expand_group_on_lane, scan_group_runs (tables: one launch for all runs of a group), batch_run_mfma (one body per
//        step of the plan: a group of 8 or a pair).  The plan itself is host arithmetic in batch_plan.h
//   [9]  multi-GPU entry points: u64 exchange, packed row shards, slot shards (pirgpu_slots_*), fix-up, pack40
//   [10] measurement
// The kernels are in kernels.hip, scan_mfma.hip, ntt_kernels.hip (+ ntt_core.h, arith.h); the wire level in wire.cpp.
#include <hip/hip_runtime.h>
#include <ctype.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/pirgpu.h"
#include "batch_plan.h"
#include "expansion_plan.h"
#include "ctmult.h"
#include "device_params.h"
#include "host_math.h"
#include "kernels.h"
#include "options.h"
#include "reply_pack.h"
#include "wire.h"

using namespace pirgpu;

namespace {

thread_local std::string g_create_error;
// last failure of THIS thread (and the context it happened on): pirgpu_last_error stays meaningful when other
// threads use the same context in between
thread_local std::string t_last_error;
thread_local const pirgpu_ctx* t_last_error_ctx = nullptr;
thread_local uint64_t t_last_error_gen = 0;   // generation id of that context (a new context may reuse the address)
std::atomic<uint64_t> g_ctx_generation{0};

struct Fail {
  int code;
  std::string msg;
};

#define HIP_TRY(expr)                                                                     \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      throw Fail{PIRGPU_INTERNAL, std::string(#expr) + ": " + hipGetErrorString(e_)};     \
  } while (0)

enum Phase { PH_EXPAND = 0, PH_SVNTT, PH_SCAN, PH_UPPER, PH_FINAL, PH_COUNT };

// device scratch of one call, freed on every way out
struct DevScratch {
  void* p = nullptr;
  ~DevScratch() {
    if (p) (void)hipFree(p);
  }
  template <typename T>
  T* get(size_t bytes) {
    HIP_TRY(hipMalloc(&p, std::max<size_t>(bytes, 1)));
    return static_cast<T*>(p);
  }
};

}  // namespace

// ======================================================================================================================
// [1] STATE: workers, lanes, key sets, batch sets, the context
// ======================================================================================================================
// Per-query working set: one HIP stream plus every intermediate of one query in flight.
// A context owns one worker by default; pirgpu_set_concurrency adds more so that several
// queries overlap on the GPU (the latency-bound expansion of one hides under the
// bandwidth-bound scan of another).  Database, keys and tables are shared, read-only.
struct Worker {
  hipStream_t stream = nullptr;
  uint32_t keyset = 0;               // key set of the query this worker currently holds
  uint32_t table = 0;                // table its query named (contexts with tables; 0 otherwise)
  uint64_t *res_a = nullptr, *res_b = nullptr, *prod = nullptr, *dig = nullptr, *sv_ntt = nullptr;
  uint64_t* d_query = nullptr;
  uint32_t staged_nq = 0;
  const uint64_t* sv_cur = nullptr;  // selection vector the multiply reads: sv_ntt, or caller-owned memory
  const uint64_t* sv_rows = nullptr; // packed multi-GPU exchange: only this shard's dimension-0 selectors, local index
  std::vector<uint64_t*> lvl;  // per level results; lvl[0] = reply
  uint64_t* last = nullptr;    // result_primes: level 0 at k primes, before the compact switch writes the reply to lvl[0]
                               // (packed replies: level 0 before the pack kernel does)
  uint64_t* pt_buf = nullptr;
  uint64_t* scan_part = nullptr;
  uint64_t* up_scratch = nullptr;    // split upper level (large rings): transformed plaintexts of one block of children
  size_t up_scratch_words = 0;
  uint8_t* selp = nullptr;           // digit-packed selectors of the group this worker leads (MFMA scan)
  bool reply_valid = false;
  hipEvent_t ev_expanded = nullptr, ev_scanned = nullptr;  // batch mode: cross-stream hand-offs
  hipEvent_t ev_done = nullptr;      // batch mode: this worker's reply is complete (its buffers may be reused)
  hipEvent_t ev_join = nullptr;      // pirgpu_join: everything queued on this worker's stream so far
};

// Batch mode with the MFMA scan: a group of up to 8 queries is expanded TOGETHER on one lane (the
// expansion kernels run over nodes x queries, ciphertext index = node * B + query), scanned in one
// database pass, and finished together on the same lane, in the lane's query-major buffers (the workers lend their
// selection vectors only).  Two lanes alternate so that the bandwidth-bound scan of one group overlaps the
// compute-bound expansion of the next.
// The first few levels of a group's expansion tree are a chain of small, latency-bound launches (8-128 tree ciphertexts:
// three dependent launches per level, 5-7 us each on their own, ~20 us each while the other lane's big kernels own the
// chip).  On the lane they cost 0.2-0.35 ms of a group's ~3 ms although they need almost no CU time.  Round 4: they run
// AHEAD on the context's head stream, in small buffers of their own (a ring of two per lane), and the lane picks the
// tree up at level `head_levels` behind an event: the chain is off the lanes' critical path, its few workgroups slip in
// beside the lanes' kernels.
struct HeadSlot {
  uint64_t *res_a = nullptr, *res_b = nullptr, *dig = nullptr, *prod = nullptr;
  hipEvent_t ev_ready = nullptr;    // head stream: the slot holds the tree of its group at level head_levels
  hipEvent_t ev_free = nullptr;     // lane stream: the lane's first level has consumed it
  bool in_use = false;              // ev_free has been recorded at least once
};

struct BatchLane {
  hipStream_t stream = nullptr;
  HeadSlot head[2];
  uint32_t head_next = 0;
  uint64_t *res_a = nullptr, *res_b = nullptr, *prod = nullptr, *dig = nullptr;
  uint8_t* selp = nullptr;
  // paired database pass (PIRGPU_SCAN_MFMA_PAIR): the SECOND group of a pair keeps its selection vectors
  // ([query][dim_sum] ciphertexts: the lane's workers hold the first group's), its packed selectors and its row sums here
  uint64_t* sv2 = nullptr;
  uint8_t* selp2 = nullptr;
  uint64_t* rows2 = nullptr;
  uint8_t* selp_runs = nullptr;      // contexts with tables: packed selectors of up to 8 runs of one group (one launch for all)
  hipEvent_t ev_scanned = nullptr;
  hipEvent_t ev_join = nullptr;      // pirgpu_join: everything queued on this lane so far
  // the multiply of a whole group runs on the lane's stream in these query-major buffers: one launch per kernel
  // for the (up to) 8 queries instead of one stream + one launch per query
  std::vector<uint64_t*> lvl;        // [level][query][lvl_cts[level]][2][k][N]
  uint64_t* last = nullptr;          // result_primes: [query][lvl_cts[0]][2][k][N], level 0 before the compact switch
  uint64_t* pt_buf = nullptr;        // [query][pt_words]
  uint64_t* scan_part = nullptr;     // [query][column chunk][scan_rows][2][k][N] (matrices wider than one chunk)
  uint64_t* up_scratch = nullptr;    // split upper level (large rings)
  size_t up_scratch_words = 0;
};

// Where one multiply (scan results -> reply) runs: a worker's buffers (one query) or a lane's (a group).
struct Stage {
  hipStream_t stream;
  uint64_t* const* lvl;   // per level, query-major
  uint64_t* pt_buf;       // query-major, pt_words each
  uint32_t n;             // queries
  MfmaPtrs sel;           // per query: the selection vector (whole, NTT form) or, with local_rows, only this shard's
  bool local_rows;        // dimension-0 selectors at local index (packed multi-GPU exchange)
  uint64_t** up_scratch = nullptr;   // owner's scratch for the split upper level, grown on demand
  size_t* up_scratch_words = nullptr;
  bool sel_f64 = false;   // the selectors are exact doubles (a lane's own expansion, pirgpu_ctx::sel_f64)
  uint64_t* last = nullptr;     // result_primes: the owner's level-0 buffer at k primes (query-major, lvl_cts[0] each);
                                // the compact switch writes the reply from there to lvl[0]
  bool rows_inverted = false;   // the row sums in lvl[d - 1] are in coefficient form already (slot-sharded step: the
                                // inverse transform gathered them out of the exchange buffer)
  uint32_t ksets[kMaxMfmaQueries] = {};   // ciphertext-multiplication mode: key set of every query (its relinearisation key)
};

// One group of a step of batch_run_mfma's walk: a step is one group, or two halves that share a database pass (half 0 in
// the members' and the lane's usual buffers, half 1 in the lane's second set).  They differ in nothing else.
struct GroupHalf {
  uint32_t first, n;    // its queries, by position in the served order
  uint64_t* sv;         // selection vectors of the lane's own expansion, [query][dim_sum]; null: the members' sv_ntt
  uint64_t* rows;       // its row sums (level d - 1), query-major
  MfmaPtrs sel, col;    // per query: the selection vector, and the column selectors inside it that the pass reads
};

// Ciphertext-multiplication mode: the scratch one owner of a multiply (a worker, a lane) runs its products in, allocated
// on its first level (CT contexts only) and kept.
struct CtmScratch {
  uint64_t* buf = nullptr;    // the products of one block of children (post_scan_ctm)
  size_t words = 0;
  uint64_t* selc = nullptr;   // coefficient-form selectors of the level being served
  size_t selc_words = 0;
  uint64_t* selb = nullptr;   // CT_SHARED_SEL: their centred lifts at the auxiliary base, NTT form [nq][dim][2][kb][N]
};

// One client's Galois keys on the device.  The reference deserialises the keys of every request into a local
// (server.cpp:46-48), so they are per request, not server state; here up to keyset_cap sets stay resident (least
// recently used evicted), slot 0 being the set the direct pirgpu_set_galois_key API installs.
struct KeySet {
  std::map<uint32_t, uint64_t*> keys;   // Galois element -> [k][2][k+1][N], device order, the flavour's element type
  std::vector<uint8_t> blob;            // wire layer: the serialized GaloisKeys object these keys came from
  uint64_t fingerprint = 0;             // sampled hash of `blob` (candidate selection before the full compare)
  uint64_t last_use = 0;
  uint32_t gen = 0;                     // bumped whenever the slot is emptied: a handle of an earlier tenant goes stale
  uint32_t pins = 0;                    // pirgpu_keyset_pin: requests in flight that use this set (never evicted meanwhile)
};

// What the ABI hands out for a key set: (generation << 12) | slot index.  Slot 0 (pirgpu_set_galois_key's set) has the
// handle 0.  A handle whose generation no longer matches names a set that was evicted or released since -- every entry
// point that takes one fails with FailedPrecondition instead of silently switching with another client's keys.
constexpr uint32_t kSlotBits = 12;
constexpr uint32_t kSlotMask = (1u << kSlotBits) - 1;

// One set of batch state: the staged queries and the replies of one batch (device resident), where its replies go,
// its per-query key sets and its pinned host staging.  A context has kBatchSets of them so that two request windows
// can be in flight -- the next one parsed / staged / queued while the previous one's replies are still coming back
// (wire.cpp); lanes, workers and streams are shared, their use is ordered by the streams themselves.
constexpr int kBatchSets = 2;
struct BatchSet {
  uint64_t *d_bquery = nullptr, *d_breply = nullptr;
  uint64_t* ext_reply = nullptr;   // pirgpu_batch_set_reply_buffer: the caller's device buffer batches write replies to
  uint64_t ext_reply_cts = 0;      // its capacity in ciphertexts
  uint64_t* host_reply = nullptr;  // pirgpu_batch_set_host_replies: pinned host memory every group downloads its replies to
  uint64_t host_reply_cts = 0;     // ... its capacity in ciphertexts
  bool host_reply_done = false;    // the batch that just ran queued those downloads: batch_fetch into it only waits
  uint32_t batch_cap = 0, batch_count = 0;   // batch_count: replies the reply buffer holds
  uint32_t staged_count = 0;   // queries pirgpu_batch_stage left in d_bquery (0 again when the buffers are reallocated)
  bool batch_valid = false;
  std::vector<uint32_t> batch_keysets;      // key set INDEX per staged query (all 0 unless pirgpu_batch_set_keysets) ...
  std::vector<uint32_t> batch_keyset_gens;  // ... and the generation it had then: checked again when the batch is run
  std::vector<uint32_t> batch_tables;       // table per staged query (contexts with tables; empty = all 0, pirgpu_batch_set_tables)
  // pirgpu_batch_stage_async: the queries arrive in pieces of kStagePiece queries on the main stream, one event each;
  // a group waits for the pieces that hold its queries instead of the whole upload
  std::vector<hipEvent_t> st_events;
  uint32_t st_pieces = 0;          // 0: staged synchronously, nothing to wait for
  // group-wise reply download (pirgpu_batch_set_host_replies): one event per group of the batch that just ran, recorded
  // behind the group's device-to-host copy; dl_end[i] = one past the last query of group i, dl_next = next to report
  std::vector<hipEvent_t> dl_events;
  std::vector<hipEvent_t> rd_events;   // "this group's replies are final" on the lane's stream: what the copy stream waits for
  std::vector<uint32_t> dl_end;
  size_t dl_next = 0;
  uint64_t *h_query = nullptr, *h_reply = nullptr;   // pinned host staging of the wire layer
  size_t h_query_words = 0, h_reply_words = 0;
};
constexpr uint32_t kStagePiece = 8;
static thread_local int t_batch_set = 0;   // pirgpu_batch_select

struct pirgpu_ctx {
  pirgpu_params prm{};
  uint32_t N = 0, logN = 0, k = 0, d = 0;
  size_t ctw = 0;  // words per ciphertext
  uint32_t rp = 0;   // pirgpu_params.result_primes (0: level results and replies stay at k primes)
  size_t rctw = 0;   // words per REPLY ciphertext: 2 rp N, or ctw -- packed replies: the packed word count (rpa.ct_words)
  // PIRGPU_CREATE_PACKED_REPLIES: level 0 lands in the owner's `last` buffer (as with
  // result_primes) and reply_pack_kernel writes the reply, at the bit width of its moduli, where it went before.  Set by
  // PIRGPU_CREATE_CT_COMPACT_REPLY as well (section 6.6): there rp switches level 0 alone, before the pack
  bool pack = false;
  ReplyPackArgs rpa{};   // ... its argument block: the first (rp ? rp : k) residues of [2][k][N] ciphertexts
  uint32_t dims[PIRGPU_MAX_DIMS]{};
  uint64_t stride[PIRGPU_MAX_DIMS + 1]{};  // plaintexts under one node of level l
  uint32_t sv_off[PIRGPU_MAX_DIMS + 1]{};  // selection-vector offset of dimension l
  uint32_t dim_sum = 0;
  uint32_t er = 0, E = 0;  // ExpansionRatio, 2*ER
  uint64_t reply_cts = 1;
  uint64_t P = 0;              // num_pt of the whole database
  uint32_t sb = 0, se = 0;     // shard of top-level indices
  // slot shard (multi-GPU): this context holds the NTT slots [slot0, slot0 + nslots) of EVERY
  // plaintext (device order) in the scan's operand layout; nslots == k N: the whole ring
  uint32_t slot0 = 0, nslots = 0;
  bool slot_sharded = false;
  hipEvent_t ev_after = nullptr;   // pirgpu_slots_*: the position of the caller's `after` stream
  uint64_t pt_begin = 0, pt_end = 0;  // plaintext range held by this context
  // wide items (pirgpu_params.plaintexts_per_item): `planes` databases of P plaintexts each behind one query.  A plane is
  // an outermost dimension that is not selected: in HBM plane j occupies the rows [j, j + 1) * plane_pad of d_db, every
  // plane padded with zero plaintexts to the full dims[0] x ... x dims[d-1] box so that all planes have the same shape at
  // every recursion level (zero plaintexts add nothing to any sum); the scan and every upper level run over planes x
  // their usual rows with the same selectors, and level 0 keeps `planes` rows -- the reply -- instead of one
  uint32_t planes = 1;
  uint64_t plane_pad = 0;             // plaintext rows of d_db per plane (planes > 1)
  // tables (pirgpu_params.tables): `tables` databases of these parameters behind one context, every
  // query naming the one it is answered from.  A table is an outermost dimension that is selected IN THE CLEAR: in d_db
  // table t occupies the rows [t, t + 1) * table_pad (padded to whole rows of the scanned matrix like a single database),
  // in d_dbp it is a complete operand layout of its own at byte t * dbp_bytes().  Geometry, workspace, expansion and
  // upper levels are those of ONE table; only the scan takes the table's base pointer.
  uint32_t tables = 1;
  uint64_t table_pad = 0;             // plaintext rows of d_db per table (tables > 1)
  uint32_t cur_table = 0;             // table of the single-query entry points and test hooks (pirgpu_query_use_table)
  std::vector<uint64_t> tbl_loaded, tbl_zero;   // per table: plaintexts loaded / identically zero (tables > 1)
  std::vector<uint8_t> tbl_packed;    // per table: its operand layout is up to date (tables > 1)
  uint32_t bits = 0;           // bits per coefficient for item packing

  int device = 0;
  hipStream_t stream = nullptr;
  const NttOps* ops = nullptr;  // NTT kernels for this ring degree
  int mode = kNttInt;           // arithmetic flavour of the NTT kernels (NttMode)
  DevParams hp{};
  DevParams* dp = nullptr;
  std::vector<void*> allocs;

  uint64_t* d_db = nullptr;
  std::vector<uint8_t> loaded;  // per local plaintext
  uint64_t n_loaded = 0;
  std::vector<KeySet> keysets{1};           // resident key sets; [0] = pirgpu_set_galois_key's
  uint32_t keyset_cap = 64;                 // client slots (pirgpu_set_keyset_capacity); 4.7 MB each at N = 4096, k = 2
  uint32_t cur_keyset = 0;                  // slot the single-query entry points use (pirgpu_query_use_keyset) ...
  uint32_t cur_keyset_gen = 0;              // ... and its generation at that time
  uint64_t keyset_clock = 0, key_uploads = 0, keyset_evictions = 0;
  std::vector<uint64_t*> key_pool;          // device key buffers of emptied sets, reused by the next upload (no hipMalloc)
  uint64_t* d_key_stage = nullptr;          // one key in SEAL order on its way to device order (allocated once)
  // seed-compressed keys (pirgpu_keyset_set_keys_seeded): the stage of a GROUP of keys (the
  // expansion kernel fills the c1 halves of a whole group in one launch), the seeds and the kernel's counters on the
  // device; two keys' worth of c0 halves plus the seeds and a copy of the counters in pinned host memory
  uint64_t* d_seed_stage = nullptr;
  size_t seed_stage_keys = 0;
  uint8_t* d_seeds = nullptr;
  size_t d_seeds_cap = 0;
  uint64_t* d_seed_stats = nullptr;         // [0] draws rejected, [1] an object overran its refill bound
  uint64_t* h_seed_pin = nullptr;           // [2][k][k+1][N] words, then kSeedStatWords words of counters
  uint8_t* h_seeds = nullptr;               // pinned, h_seeds_cap bytes
  size_t h_seeds_cap = 0;
  hipEvent_t ev_seed_pin[2] = {nullptr, nullptr};   // "the copy out of this half of h_seed_pin is done"
  uint64_t seed_objects = 0;                // objects expanded on the device so far
  // compact queries (pirgpu_query_stage_compact / pirgpu_batch_stage_compact): the compact words
  // of cq_cap queries as they were uploaded, then 8 seed words per ciphertext gathered by query_unpack_kernel.  Written
  // and read on `stream` only, so its reuse from call to call is covered by stream order
  uint64_t* d_cq_stage = nullptr;
  uint32_t cq_cap = 0;                      // queries the stage holds
  uint64_t* h_cq_stats = nullptr;           // ... their pinned copy, read behind a wait (synchronous calls)
  uint64_t* d_cq_stats = nullptr;           // the expansion kernel's counters for queries: [0] draws rejected, [1] overrun
  uint64_t cq_objects = 0;                  // compact ciphertexts expanded on the device so far
  std::map<uint32_t, uint64_t*> xpow;       // shift -> NTT_j(x^(-shift)), [k][N] doubles (NTT-domain last expansion level)
  std::map<uint32_t, uint16_t*> gperm;      // Galois element g -> [2][N] u16: sigma_g / sigma_(g^-1) on NTT positions (galois_perm_table)

  // workspace geometry (computed on first use) and the workers holding the buffers
  bool ws_ready = false;
  std::vector<Worker> workers;     // workers[0] uses `stream`
  std::vector<uint64_t> lvl_rows;  // nodes per level inside the shard
  std::vector<uint64_t> lvl_cts;   // ciphertexts per level result buffer
  uint64_t m_max = 1;              // expansion tree width (ciphertexts)
  uint64_t pt_words = 0;
  // batch mode (pirgpu_batch_*): kBatchSets independent sets of batch state (BatchSet above); the calling thread's
  // pirgpu_batch_select picks the one its pirgpu_batch_* calls operate on (default 0)
  BatchSet sets[kBatchSets];
  BatchSet& bs();
  uint32_t n_active = 1;
  // Fields that resolve_options / resolve_live_options fill from the options (options.h has what each one means and
  // why its default is what it is; the defaults themselves stand at the reads).  Nothing reads them before
  // ensure_workspace has run.
  uint32_t upper_blocks = 0;     // target workgroup count of upper_fused_kernel (option UPPER_BLOCKS)
  uint32_t upper_blocks_batch = 0;    // the same per query in batch mode (option UPPER_BLOCKS_BATCH)
  // live options, resolved when the workspace is built and whenever pirgpu_set_option sets one: the paths that queue GPU
  // work read these fields, never a name or the environment
  uint32_t scan_wgs_batch = 0;   // persistent workgroups (= CUs) of the MFMA scan in the batch pipeline; 0 = all CUs
                                 // (option SCAN_MFMA_WGS_BATCH)
  int64_t slots_scan_wgs = -1;   // the same for the slot-sharded step; -1: follows scan_wgs_batch (option SLOTS_SCAN_WGS unset)
  bool slots_gather_ntt = false, slots_blk_major = false;   // options SLOTS_GATHER_NTT, SLOTS_SCAN_BLK_MAJOR
  bool tables_one_launch = false;                           // option TABLES_ONE_LAUNCH
  int64_t ctm_rowsum_splits = 0;                            // option CT_ROWSUM_SPLITS
  bool in_batch = false;         // set while the batch pipeline enqueues work
  uint32_t scan_nsplit = 1, scan_cps = 0, scan_rows = 0, scan_cols = 0;
  uint32_t scan_rpt = 0, scan_block = 0;    // rows per thread / workgroup size of the scan kernel
  bool scan_limb = false;                   // 28-bit limb accumulators (all data moduli < 2^50)
  uint32_t mq_nq = 4, mq_rows = 1;          // batch mode: queries per database pass / rows per wave
  bool mq_single = false;                   // use the LDS-shared scan kernel for single queries too
  uint32_t mq_single_rows = 4;              // rows per wave of that kernel for a single query (2 or 4)
  bool mq_single_limb = false;              // single query: 128-bit accumulators need fewer registers (3 WG/CU)
  uint64_t scan_npt = 0;
  // digit-sliced int8-MFMA scan (scan_mfma.hip): d >= 2, database additionally held in operand layout
  bool mfma_on = false;
  MfmaGeom mg{};
  uint32_t mfma_nq = 0;                     // queries per database pass in batch mode
  bool mfma_single = false;                 // single queries use it too (off for matrices wider than one chunk)
  bool scan_f64_fold = false;               // the scan folds its digit diagonals in exact fp64 arithmetic (option
                                            // SCAN_F64_FOLD; every data modulus below 2^50)
  bool scan_f64_fold_batch = false;         // ... in the launches that serve a group of queries (option SCAN_F64_FOLD_BATCH)
  uint32_t scan_pair = 1;                   // two groups per database read (scan_mfma_pair.hip): 0 off, 1 in calls that queue at
                                            // least four groups, 2 whenever a call has two left (PIRGPU_SCAN_MFMA_PAIR)
  bool split_upper = false;                 // upper level as transform-to-scratch + elementwise MAC (N >= 16384 in the fp64
                                            // flavours, where the fused kernel spills; option SPLIT_UPPER overrides)
  uint64_t split_upper_words = 0;           // scratch budget per lane / worker (option SPLIT_UPPER_MB)
  // the digit kernel of the wide expansion levels and the transform kernel of the split upper level run all transforms
  // of one source polynomial in ONE workgroup: one load and one permutation per source, stores drain under the next
  // transform (option LOOP_TRANSFORMS; fp64 flavours)
  bool loop_transforms = false;
  uint32_t loop_min_sources = 1024;         // ... from this many (tree ciphertext, digit) sources per launch on
  uint32_t fuse_mac_nodes = 128;            // ... from this many tree ciphertexts per level on (narrower levels are latency-
                                            // bound: two dependent transform kernels cost more than mac + light combine)
  bool fuse_mac_combine = false;            // levels below the last: combine step in the data residues' MAC + inverse-NTT
                                            // kernel (option FUSE_MAC_COMBINE = 0: separate ks_combine pass)
  bool fuse_last_level = false;             // last expansion level fused with the selector NTT (option FUSE_LAST = 0: off)
  bool last_level_ntt = false;              // ... and carried out in the NTT domain (option LAST_NTT = 0: coefficient form)
  bool tree40 = false;                      // expansion tree between fused wide levels as 5-byte polynomials (option TREE40 = 0: doubles)
  bool c0_ntt = false;                      // the fused levels keep the tree's c0 polynomials in NTT form (option C0_NTT = 1 / 2; measured slower)
  bool c0_ntt_split = false;                // ... with component 0 of a level as a launch of its own (C0_NTT = 2)
  bool want_sel_f64 = false;
  bool sel_f64 = false;                     // batch lanes keep their selectors as exact doubles between the last expansion
                                            // level and their two consumers (sel_pack, upper level): no u64 round trip
                                            // (fp64 flavours, MFMA scan, NTT-domain last level; option SEL_F64 = 0: off)
  bool pack40 = false;                      // key-switch digits stored packed (option PACK40) ...
  int pack_bytes = 5;                       // ... in 5 (all moduli < 2^39), 6 (< 2^47) or 7 (< 2^55) bytes per residue (option PACK_BYTES)
  uint8_t* d_dbp = nullptr;
  bool packed_valid = false;
  bool staging_released = false;            // pirgpu_db_finalize(release): only the operand-layout copy is left
  // streamed database (pirgpu_create_ex, PIRGPU_CREATE_STREAMED_DB): d_db is never allocated,
  // loads encode chunks of whole row bands into a scratch and pack them straight into d_dbp (pack_range)
  bool streamed = false;
  uint64_t stream_bands = 1;                // row bands (16 rows of the scanned matrix) per load chunk (option DB_STREAM_MB)
  // the library's own count of the database's device bytes (pirgpu_db_memory): the two copies, the load / update scratch
  // held right now, and the largest sum of the three so far
  uint64_t db_bytes = 0, dbp_alloc = 0, mem_scratch = 0, mem_peak = 0;
  std::vector<BatchLane> lanes;             // created on the first batch
  uint64_t groups_run = 0;
  hipStream_t head_stream = nullptr;        // the narrow first levels of every group's expansion (HeadSlot)
  uint32_t head_levels = 0;                 // levels 0 .. head_levels - 1 run there (option HEAD_LEVELS; 0: all on the lane)
  uint32_t head_mode = 0;                   // option HEAD_MODE: 0 never, 1 batches staged with pirgpu_batch_stage_async, 2 always
  hipEvent_t ev_head_tail = nullptr;        // the head stream's position (an upload into a batch set waits for it)
  hipStream_t copy_stream = nullptr;        // device-to-host downloads of finished groups (pirgpu_batch_set_host_replies):
                                            // a lane that downloaded its own replies sat idle for 8 MB of PCIe per group
  hipEvent_t ev_fetch[2] = {nullptr, nullptr};   // pirgpu_query_fetch_begin: the two halves of the reply's download
  hipEvent_t ev_fork = nullptr;             // pirgpu_fork: the main stream's position
  hipEvent_t ev_main_join = nullptr;        // pirgpu_join_stream onto a caller's stream: the main stream's position

  // ciphertext-multiplication mode (pirgpu_create_ex, PIRGPU_CREATE_CT_MULTIPLY): the upper levels
  // multiply ciphertext by ciphertext (exact BFV product + relinearisation) instead of re-encoding: E = 1 at every level
  bool ctm = false;
  bool ctm_deferred = false;                // PIRGPU_CREATE_CT_DEFERRED: one rounding and one key switch per row
  bool ctm_compact = false;                 // PIRGPU_CREATE_CT_COMPACT_REPLY: sets `pack`, lets rp be non-zero (reply only)
  uint32_t kb = 0;                          // primes of the auxiliary base (k + 2)
  uint64_t aux_primes[PIRGPU_MAX_PRIMES]{};
  DevParams hp_aux{};                       // the auxiliary base as the "data primes" of a second parameter block:
  DevParams* dp_aux = nullptr;              // ntt_batch transforms at B with the context's own kernels and flavour
  CtmParams* d_ctm = nullptr;               // constants of the exact base conversions (ctmult.h)
  uint64_t ctm_scratch_words = 0;           // product scratch per owner (option CT_SCRATCH_MB)
  bool ctm_shared_sel = false;              // a level's selectors are lifted and transformed once (option CT_SHARED_SEL)
  std::map<hipStream_t, CtmScratch> ctm_ws; // per owner of a multiply, keyed by its stream

  bool prof = false;
  // batch pipeline under profiling: HIP events around the scan launches of the groups (the launch that serves the
  // headline step runs on `scan_wgs_batch` workgroups beside the other lane's kernels -- not the full-chip single-query
  // launch the roofline block quotes); read out by pirgpu_batch_scan_timings
  std::vector<hipEvent_t> bscan_ev;   // pairs (start, stop)
  uint32_t bscan_n = 0, bscan_wgs = 0, bscan_nq = 0;
  static constexpr int kMaxProfRuns = 256;
  std::vector<hipEvent_t> ev;  // kMaxProfRuns x (PH_COUNT + 1), created lazily
  int prof_runs = 0;           // runs recorded since the last read-out
  int prof_cur = -1;           // event set of the run being recorded (-1: not recording)
  float timings[6]{};

  // what pirgpu_set_option was given by name, and the counters (options.h); a name not set here falls back to the
  // environment variable PIRGPU_<NAME> (A/B scripts under tools/), then to the built-in default
  OptionStore options;
  std::string err;
  uint64_t gen = 0;         // unique per context (thread-local error messages are keyed on it, not on the address)
  std::recursive_mutex mu;  // per ABI call; pirgpu_process_request holds it across its whole body
  uint64_t zero_pts = 0;    // all-zero database plaintexts in this shard (SEAL: "result ciphertext is transparent")
  uint64_t remote_zero_pts = 0;   // ... in the other shards of a row-sharded database (pirgpu_set_remote_zero_plaintexts)
  bool allow_transparent = false;

  template <typename T>
  T* dalloc(size_t count) {
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)));
    allocs.push_back(p);
    return static_cast<T*>(p);
  }
  void use_device() { HIP_TRY(hipSetDevice(device)); }
};

BatchSet& pirgpu_ctx::bs() { return sets[t_batch_set]; }

// plaintexts this context must hold before it answers queries (all planes)
static inline uint64_t held_pts(const pirgpu_ctx* c) { return (uint64_t)c->tables * c->planes * (c->pt_end - c->pt_begin); }
// plaintext rows of the matrix the scan and the upper levels walk: the shard, or planes x the padded plane
static inline uint64_t matrix_pts(const pirgpu_ctx* c) {
  return c->planes > 1 ? (uint64_t)c->planes * c->plane_pad : c->pt_end - c->pt_begin;
}
// ABI plaintext index (plane-major: plane * num_pt + pt; table-major: table * num_pt + pt) -> row of d_db
static inline uint64_t db_row(const pirgpu_ctx* c, uint64_t index) {
  if (c->tables > 1) return index / c->P * c->table_pad + index % c->P;
  return c->planes > 1 ? index / c->P * c->plane_pad + index % c->P : index - c->pt_begin;
}
// contexts with tables: the staging rows of table t
static inline const uint64_t* table_db(const pirgpu_ctx* c, uint32_t t) {
  return c->d_db ? c->d_db + (size_t)t * c->table_pad * c->k * c->N : nullptr;
}
// pirgpu_db_memory's peak: called wherever one of the counted sizes grows
static inline void note_mem(pirgpu_ctx* c) {
  c->mem_peak = std::max(c->mem_peak, c->db_bytes + c->dbp_alloc + c->mem_scratch);
}
// device scratch of a load or an update, counted while it is held
struct ScratchNote {
  pirgpu_ctx* c;
  uint64_t bytes;
  ScratchNote(pirgpu_ctx* ctx, uint64_t n) : c(ctx), bytes(n) {
    c->mem_scratch += bytes;
    note_mem(c);
  }
  ~ScratchNote() { c->mem_scratch -= bytes; }
  ScratchNote(const ScratchNote&) = delete;
  ScratchNote& operator=(const ScratchNote&) = delete;
};

namespace {

// ======================================================================================================================
// [2] HELPERS: errors, tables (twiddles, Encode order), options, workspace geometry (ensure_workspace)
// ======================================================================================================================
int fail(pirgpu_ctx* c, int code, const std::string& msg) {
  if (c) {
    std::lock_guard<std::recursive_mutex> lock(c->mu);
    c->err = msg;
    t_last_error = msg;
    t_last_error_ctx = c;
    t_last_error_gen = c->gen;
  }
  return code;
}

template <typename F>
int guarded(pirgpu_ctx* c, F&& f) {
  if (!c) return PIRGPU_INVALID_ARGUMENT;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  try {
    c->use_device();
    return f();
  } catch (const Fail& e) {
    return fail(c, e.code, e.msg);
  } catch (const std::exception& e) {
    return fail(c, PIRGPU_INTERNAL, e.what());
  }
}

// Modulus i of a parameter block: Barrett ratio, twiddle tables (integer and fp64 form) on the device.
void fill_modulus(pirgpu_ctx* c, DevParams& hp, uint32_t i, uint64_t q) {
  const uint32_t N = c->N;
  std::vector<Twiddle> tw(N), itw(N);
  {
    hp.mod[i].q = q;
    hm::u128 ratio = (~(hm::u128)0) / q;  // floor((2^128 - 1) / q) == floor(2^128 / q) for odd q > 1
    hp.mod[i].br_lo = (uint64_t)ratio;
    hp.mod[i].br_hi = (uint64_t)(ratio >> 64);
    const uint64_t psi = hm::minimal_primitive_root(2ull * N, q);
    if (!psi) throw Fail{PIRGPU_INVALID_ARGUMENT, "modulus has no primitive 2N-th root of unity"};
    const uint64_t ipsi = hm::invmod_prime(psi, q);
    uint64_t pw = 1, ipw = 1;
    for (uint32_t j = 0; j < N; ++j) {
      uint32_t r = hm::bitrev(j, c->logN);
      tw[r] = Twiddle{pw, hm::shoup(pw, q)};
      itw[r] = Twiddle{ipw, hm::shoup(ipw, q)};
      pw = hm::mulmod(pw, psi, q);
      ipw = hm::mulmod(ipw, ipsi, q);
    }
    Twiddle* dev = c->dalloc<Twiddle>((size_t)2 * N);
    HIP_TRY(hipMemcpy(dev, tw.data(), N * sizeof(Twiddle), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dev + N, itw.data(), N * sizeof(Twiddle), hipMemcpyHostToDevice));
    hp.tab[i].tw = dev;
    hp.tab[i].itw = dev + N;
    const uint64_t ninv = hm::invmod_prime(N % q, q);
    const uint64_t iw1n = hm::mulmod(itw[1].w, ninv, q);
    hp.tab[i].ninv = Twiddle{ninv, hm::shoup(ninv, q)};
    hp.tab[i].iw1n = Twiddle{iw1n, hm::shoup(iw1n, q)};
    // exact-fp64 flavour: the same constants as signed doubles in (-q/2, q/2]
    auto centered = [q](uint64_t v) { return v > q / 2 ? -(double)(q - v) : (double)v; };
    std::vector<double> twf(N), itwf(N);
    for (uint32_t j = 0; j < N; ++j) {
      twf[j] = centered(tw[j].w);
      itwf[j] = centered(itw[j].w);
    }
    double* devf = c->dalloc<double>((size_t)2 * N);
    HIP_TRY(hipMemcpy(devf, twf.data(), N * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(devf + N, itwf.data(), N * sizeof(double), hipMemcpyHostToDevice));
    hp.tab[i].twf = devf;
    hp.tab[i].itwf = devf + N;
    hp.tab[i].ninv_f = centered(ninv);
    hp.tab[i].iw1n_f = centered(iw1n);
    hp.tab[i].qd = (double)q;
    hp.tab[i].qinvd = 1.0 / (double)q;
  }
}

void build_tables(pirgpu_ctx* c) {
  const uint32_t N = c->N, k = c->k;
  DevParams& hp = c->hp;
  hp.N = N;
  hp.logN = c->logN;
  hp.k = k;
  uint64_t qmax = 0;
  for (uint32_t i = 0; i <= k; ++i) {
    const uint64_t q = i < k ? c->prm.coeff_modulus[i] : c->prm.special_prime;
    qmax = std::max(qmax, q);
    fill_modulus(c, hp, i, q);
  }
  // NTT arithmetic flavour (ntt_core.h).  PIRGPU_NTT_MODE=0 forces the integer path.
  c->mode = qmax < (1ull << 46) ? kNttF64 : (qmax < (1ull << 49) ? kNttF64Wide : kNttInt);
  if (const char* v = pirgpu_env("PIRGPU_NTT_MODE")) {
    int want = atoi(v);
    if (want == kNttInt || (want == kNttF64Wide && c->mode != kNttInt) || want == c->mode) c->mode = want;
  }
  // N = 32768 has the integer flavour only (ntt_ring32k.hip: two-pass transforms through HBM, no fused fp64 kernels),
  // whatever the moduli; a PIRGPU_NTT_MODE asking for an fp64 flavour is ignored there
  if (c->logN >= 15) c->mode = kNttInt;
  hp.ntt_mode = c->mode;
  hp.f64_lazy_inv = (64 - (uint32_t)__builtin_clzll(qmax)) + c->logN <= 52 ? 1u : 0u;
  if (const char* v = pirgpu_env("PIRGPU_F64_LAZY_INV")) hp.f64_lazy_inv = atoi(v) ? hp.f64_lazy_inv : 0u;
  const uint64_t p = c->prm.special_prime, t = c->prm.plain_modulus;
  hp.p_half = p >> 1;
  hp.p_f = (double)p;
  hp.p_half_f = (double)(p >> 1);
  hp.t = t;
  hp.plain_thr = (t + 1) >> 1;
  for (uint32_t j = 0; j < k; ++j) {
    const uint64_t q = hp.mod[j].q;
    hp.p_half_mod[j] = (p >> 1) % q;
    hp.p_inv[j] = hm::invmod_prime(p % q, q);
    hp.p_inv_s[j] = hm::shoup(hp.p_inv[j], q);
    hp.p_inv_f[j] = hp.p_inv[j] > q / 2 ? -(double)(q - hp.p_inv[j]) : (double)hp.p_inv[j];
    hp.lift_inc[j] = q - (t % q);
    uint64_t w = (1ull << 32) % q, acc = w;
    for (int e = 0; e < 3; ++e) {     // 2^(32 (e + 1)) mod q, centred
      hp.fold_w[j][e] = acc > q / 2 ? -(double)(q - acc) : (double)acc;
      acc = hm::mulmod(acc, w, q);
    }
  }
  // modulus switch: the constants of the drop step of every possible last prime q_m (any level is reachable through
  // pirgpu_mod_switch, whatever result_primes says)
  for (uint32_t m = 1; m < k; ++m) {
    const uint64_t qm = hp.mod[m].q;
    hp.ms_half[m] = qm >> 1;
    for (uint32_t i = 0; i < m; ++i) {
      const uint64_t q = hp.mod[i].q;
      hp.ms_half_mod[m][i] = (qm >> 1) % q;
      hp.ms_inv[m][i] = hm::invmod_prime(qm % q, q);
      hp.ms_inv_s[m][i] = hm::shoup(hp.ms_inv[m][i], q);
    }
  }
  // CiphertextReencoder::Encode order (reference ct_reencoder.cpp:49-69); with result_primes the level results have
  // been switched to their first rp residues before Encode reads them
  const uint32_t b = hm::bits_per_coeff(t);
  hp.enc_bits = b;
  uint32_t e = 0;
  for (uint32_t poly = 0; poly < 2; ++poly)
    for (uint32_t j = 0; j < (c->rp ? c->rp : k); ++j) {
      uint32_t ler = hm::local_expansion_ratio(hp.mod[j].q, b);
      for (uint32_t i = 0; i < ler; ++i) {
        if (e >= (uint32_t)kMaxEnc) throw Fail{PIRGPU_INVALID_ARGUMENT, "expansion ratio too large"};
        hp.enc_poly[e] = (uint8_t)poly;
        hp.enc_res[e] = (uint8_t)j;
        hp.enc_shift[e] = (uint8_t)(i * b);
        ++e;
      }
    }
  hp.enc_count = e;
  c->E = e;
  c->er = e / 2;
  uint32_t qbits = 64 - __builtin_clzll(qmax);
  int room = 128 - 2 * (int)qbits;
  hp.lazy_limit = 1u << std::min(30, std::max(0, room));
  c->dp = c->dalloc<DevParams>(1);
  HIP_TRY(hipMemcpy(c->dp, &hp, sizeof(DevParams), hipMemcpyHostToDevice));
}

// Ciphertext-multiplication mode: the auxiliary base as a parameter block of its own (the transforms at B are the
// context's ntt_batch in the context's flavour: the auxiliary primes have the size of the largest data prime, so every
// bound the flavour was chosen by holds for them) and the constants of the base conversions.  After build_tables.
void build_ctm_tables(pirgpu_ctx* c) {
  DevParams& hp = c->hp_aux;
  hp = DevParams{};
  hp.N = c->N;
  hp.logN = c->logN;
  hp.k = c->kb;
  for (uint32_t i = 0; i < c->kb; ++i) fill_modulus(c, hp, i, c->aux_primes[i]);
  hp.ntt_mode = c->mode;
  hp.f64_lazy_inv = c->hp.f64_lazy_inv;
  hp.lazy_limit = c->hp.lazy_limit;
  c->dp_aux = c->dalloc<DevParams>(1);
  HIP_TRY(hipMemcpy(c->dp_aux, &hp, sizeof(DevParams), hipMemcpyHostToDevice));
  CtmParams cp;
  ctm::fill_params(cp, c->N, c->k, c->prm.coeff_modulus, c->aux_primes, c->prm.plain_modulus);
  c->d_ctm = c->dalloc<CtmParams>(1);
  HIP_TRY(hipMemcpy(c->d_ctm, &cp, sizeof(CtmParams), hipMemcpyHostToDevice));
}

uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

std::string upper_case(const char* s) {
  std::string up(s);
  for (char& ch : up) ch = (char)toupper((unsigned char)ch);
  return up;
}

// Streamed database: bytes of one encoded row band -- the 16 rows of the scanned matrix that make up one row tile of the
// operand layout -- as u64 residues (valid once ensure_workspace has fixed the geometry)
uint64_t stream_band_bytes(const pirgpu_ctx* c) { return 16ull * c->scan_cols * c->k * c->N * 8; }

// waits for everything the batch pipeline has enqueued: lane streams (grouped expansion + multiply) and worker streams
void sync_batch_streams(pirgpu_ctx* c) {
  for (BatchLane& ln : c->lanes)
    if (ln.stream) HIP_TRY(hipStreamSynchronize(ln.stream));
  if (c->head_stream) HIP_TRY(hipStreamSynchronize(c->head_stream));
  if (c->copy_stream) HIP_TRY(hipStreamSynchronize(c->copy_stream));   // reply downloads queued behind the lanes
  for (Worker& w : c->workers)
    if (w.stream) HIP_TRY(hipStreamSynchronize(w.stream));
}

bool all_zero_bytes(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (p[i]) return false;
  return true;
}

// loaded[] per local plaintext: 0 = not loaded, 1 = loaded, 2 = loaded and identically zero
void note_plaintext(pirgpu_ctx* c, uint64_t local, bool zero) {
  uint8_t& st = c->loaded[local];
  if (c->tables > 1) {   // the same counts per table (local = table * num_pt + pt)
    const uint64_t t = local / c->P;
    if (!st) ++c->tbl_loaded[t];
    if (st == 2) --c->tbl_zero[t];
    if (zero) ++c->tbl_zero[t];
  }
  if (!st) ++c->n_loaded;
  if (st == 2) --c->zero_pts;
  st = zero ? 2 : 1;
  if (zero) ++c->zero_pts;
}

// A query is answered once ITS database is complete: the whole context, or -- with tables -- the table it names.
bool table_loaded(const pirgpu_ctx* c, uint32_t t) {
  return c->tables > 1 ? c->tbl_loaded[t] == c->P : c->n_loaded == held_pts(c);
}

// Evaluator::multiply_plain throws logic_error("result ciphertext is transparent") when its result has an
// all-zero c1 (SEAL's default build, SEAL_THROW_ON_TRANSPARENT_CIPHERTEXT), which happens for every query as
// soon as one database plaintext is identically zero; PIRDatabase::multiply maps it to InternalError
// (reference database.cpp:308-315).  pirgpu_set_transparent_policy(ctx, 1) returns the mathematically defined
// reply instead.
void check_transparent(pirgpu_ctx* c, uint32_t table = 0) {
  // the reference fails every query as soon as ANY plaintext of the whole database is zero: a row shard also counts
  // the zero plaintexts the other shards reported, so that all ranks of a sharded server take the same decision.
  // Tables: the database of a query is the table it names -- the other tables' plaintexts do not count
  const uint64_t zeros = c->tables > 1 ? c->tbl_zero[table] : c->zero_pts || c->remote_zero_pts;
  if (zeros && !c->allow_transparent) throw Fail{PIRGPU_INTERNAL, "result ciphertext is transparent"};
}

void alloc_worker(pirgpu_ctx* c, Worker& w);
void ensure_expansion_buffers(pirgpu_ctx* c, Worker& w);

// An option as the unsigned number most fields are (a negative value wraps, and the clamps below then cap it).
uint32_t opt_u32(const pirgpu_ctx* c, OptId id, uint32_t dflt) { return (uint32_t)c->options.value(id, dflt); }

bool ctm_shared_sel_default(const pirgpu_ctx* c) { return c->ctm && c->planes > 1; }

// What pirgpu_get_option answers for an option that was given nowhere: -1, "the built-in default applies" -- or the
// default itself where it depends on the context
int64_t unset_report(const pirgpu_ctx* c, OptId id) { return id == OPT_CT_SHARED_SEL ? ctm_shared_sel_default(c) : -1; }

// Live options -> fields.  Runs when the workspace is built and whenever pirgpu_set_option sets one of them, so that the
// paths that queue GPU work read fields only; the environment is read here and nowhere later.
void resolve_live_options(pirgpu_ctx* c) {
  c->scan_wgs_batch = (uint32_t)std::max<int64_t>(0, c->options.value(OPT_SCAN_MFMA_WGS_BATCH, 128));
  bool given = false;   // unset: the slot-sharded pass follows scan_wgs_batch, whatever that is set to later
  const int64_t slots_wgs = c->options.value(OPT_SLOTS_SCAN_WGS, 0, &given);
  c->slots_scan_wgs = given ? std::max<int64_t>(0, slots_wgs) : -1;
  c->slots_gather_ntt = c->options.value(OPT_SLOTS_GATHER_NTT, 1) != 0;
  c->slots_blk_major = c->options.value(OPT_SLOTS_SCAN_BLK_MAJOR, 1) != 0;
  c->tables_one_launch = c->options.value(OPT_TABLES_ONE_LAUNCH, 1) != 0;
  c->ctm_rowsum_splits = c->options.value(OPT_CT_ROWSUM_SPLITS, 0);
}

// Options in, fields out: everything ensure_workspace and the launch paths need to know about the options, read once
// per context (options.h says what each option means and why its default is what it is).  Needs the scan's matrix
// (scan_rows, scan_cols, scan_npt).  The order matters: mfma_geometry takes SCAN_MFMA_WIDE and SCAN_MFMA_TOP4, and the
// defaults of SCAN_MFMA_SINGLE and SCAN_F64_FOLD depend on the geometry it returns.
void resolve_options(pirgpu_ctx* c) {
  const uint32_t N = c->N, k = c->k, d = c->d;
  resolve_live_options(c);
  c->upper_blocks = (uint32_t)std::max<int64_t>(1, c->options.value(OPT_UPPER_BLOCKS, 512));
  c->upper_blocks_batch = (uint32_t)std::max<int64_t>(1, c->options.value(OPT_UPPER_BLOCKS_BATCH, 64));
  c->upper_blocks_batch = std::min(c->upper_blocks_batch, c->upper_blocks);  // the scratch is sized for upper_blocks
  // launch geometry of the 64-bit scan kernels
  c->scan_limb = true;
  for (uint32_t j = 0; j < k; ++j) c->scan_limb = c->scan_limb && (c->hp.mod[j].q >> 50) == 0;
  if (!opt_u32(c, OPT_SCAN_LIMB, 1)) c->scan_limb = false;
  //   (settled in rounds 1 - 2, constants since round 5: 4 queries share one pass of the 64-bit kernels in batch mode,
  //   one row per wave then; a single query takes four rows per wave with limb accumulators off -- HISTORY section 9)
  c->mq_nq = 4;
  c->mq_rows = 1;
  c->mq_single = opt_u32(c, OPT_SCAN_MQ_SINGLE, 1) != 0;
  c->mq_single_rows = 4;
  c->mq_single_limb = false;
  c->scan_rpt = opt_u32(c, OPT_SCAN_ROWS, 4);
  c->scan_block = opt_u32(c, OPT_SCAN_BLOCK, 256);
  const uint32_t xblocks = (k * N / 2 + c->scan_block - 1) / c->scan_block;
  const uint32_t yblocks = (c->scan_rows + c->scan_rpt - 1) / c->scan_rpt;
  uint64_t have = (uint64_t)xblocks * std::max<uint32_t>(yblocks, 1) * c->scan_block / 256;
  // split the columns only when whole rows cannot fill the chip (d = 1 / few rows)
  uint32_t want = have >= 512 ? 1 : (uint32_t)ceil_div(1024, std::max<uint64_t>(have, 1));
  want = opt_u32(c, OPT_SCAN_NSPLIT, want);
  want = std::max<uint32_t>(1, std::min<uint32_t>(want, std::max<uint32_t>(c->scan_cols, 1)));
  c->scan_cps = (uint32_t)ceil_div(std::max<uint32_t>(c->scan_cols, 1), want);
  c->scan_nsplit = (uint32_t)ceil_div(std::max<uint32_t>(c->scan_cols, 1), c->scan_cps);
  // expansion
  c->fuse_last_level = opt_u32(c, OPT_FUSE_LAST, 1) != 0;
  c->fuse_mac_combine = opt_u32(c, OPT_FUSE_MAC_COMBINE, 1) != 0;
  c->last_level_ntt = opt_u32(c, OPT_LAST_NTT, 1) != 0;
  {
    const uint32_t v = opt_u32(c, OPT_C0_NTT, 0);
    c->c0_ntt = v != 0;
    c->c0_ntt_split = v >= 2;
  }
  c->want_sel_f64 = opt_u32(c, OPT_SEL_F64, 1) != 0;
  c->tree40 = opt_u32(c, OPT_TREE40, 1) != 0;
  c->fuse_mac_nodes = 128;       // swept in round 2 (HISTORY section 4): a constant since round 5
  c->head_levels = std::min<uint32_t>(opt_u32(c, OPT_HEAD_LEVELS, 5), 8);
  c->head_mode = std::min<uint32_t>(opt_u32(c, OPT_HEAD_MODE, 1), 2);
  c->split_upper = opt_u32(c, OPT_SPLIT_UPPER, c->logN >= 14 ? 1 : 0) != 0 && c->mode != kNttInt;
  // N = 32768: always the split form, in its integer version (upper_ntt + launch_upper_mac_int) -- that degree's table
  // has no upper_fused
  if (c->logN >= 15) c->split_upper = true;
  c->split_upper_words = (uint64_t)opt_u32(c, OPT_SPLIT_UPPER_MB, 3072) * (1ull << 20) / 8;
  c->loop_transforms = opt_u32(c, OPT_LOOP_TRANSFORMS, 1) != 0 && c->mode != kNttInt;
  // (loop_min_sources: swept 512 - 4096 in round 4, 1 024 stays: a constant since round 5)
  c->pack40 = opt_u32(c, OPT_PACK40, 1) != 0;
  {
    // packed width of the key-switch intermediates: the fewest whole bytes the moduli allow, or the wider one asked for
    uint32_t bits = 0;
    for (uint32_t j = 0; j <= k; ++j) bits = std::max<uint32_t>(bits, 64 - (uint32_t)__builtin_clzll(c->hp.mod[j].q));
    const int need = bits <= 39 ? 5 : (bits <= 47 ? 6 : (bits <= 55 ? 7 : 8));
    int want = (int)opt_u32(c, OPT_PACK_BYTES, (uint32_t)need);
    if (want < need) want = need;
    if (c->mode == kNttInt && want != 5) want = 8;
    if (c->logN >= 15) want = 8;   // N = 32768: the integer kernels there keep their intermediates as u64
    if (want > 7) c->pack40 = false;
    c->pack_bytes = c->pack40 ? want : 5;
    if (c->pack40 && c->pack_bytes == 7 && c->logN >= 14 && !opt_u32(c, OPT_TREE40_WIDE, 0)) c->tree40 = false;
    const NttOps* ops = ntt_ops_for(N, c->pack_bytes);
    if (ops != c->ops) {
      c->ops = ops;
      HIP_TRY(c->ops->configure(c->mode));
    }
  }
  // int8-MFMA scan
  bool wide_given = false;
  const int64_t wide = c->options.value(OPT_SCAN_MFMA_WIDE, 0, &wide_given);
  c->mg = mfma_geometry(c->hp, c->scan_rows, c->scan_cols, wide_given ? (int)(wide != 0) : -1,
                        opt_u32(c, OPT_SCAN_MFMA_TOP4, 1) != 0);
  c->mfma_on = opt_u32(c, OPT_SCAN_MFMA, 1) != 0 && d >= 2 && c->mg.L != 0 && c->scan_rows >= 8 && c->scan_npt > 0;
  if (c->slot_sharded && (!c->mfma_on || c->mg.nchunks != 1 || c->nslots % c->mg.NW))
    throw Fail{PIRGPU_INVALID_ARGUMENT, "a slot shard needs the int8-MFMA scan in one column chunk (d = 2, >= 8 rows, "
                                        "moduli below 2^55, at most 28 column groups)"};
  c->mfma_nq = std::max<uint32_t>(1, std::min<uint32_t>(opt_u32(c, OPT_SCAN_MFMA_NQ, kMaxMfmaQueries), kMaxMfmaQueries));
  c->mfma_single = opt_u32(c, OPT_SCAN_MFMA_SINGLE, c->mg.nchunks == 1 ? 1 : 0) != 0;
  c->scan_f64_fold = opt_u32(c, OPT_SCAN_F64_FOLD, c->mg.L >= 6 ? 1 : 0) != 0;
  c->scan_f64_fold_batch = opt_u32(c, OPT_SCAN_F64_FOLD_BATCH, 1) != 0;
  // Two groups per database read in the batch pipeline (scan_mfma_pair.hip).  Environment only, like PIRGPU_SCAN_MFMA_WGS
  // (tests, A/B; read here, when the workspace is built): 0 off, 1 (the default) in calls that queue at least four groups,
  // so that both lanes get a pair and shorter calls keep the finer pipeline, 2 whenever a call has two groups left.
  // Kernel alone at cfg 3, one paired launch against two single ones: 0.72 of the time on 128 workgroups, 0.63 on 256.
  // Headline, same library, 0 against 1, alternating runs after two of the same setting (spread 0.3 %): 5 530 / 5 548 /
  // 5 577 / 5 574 / 5 575 / 5 574 against 5 797 / 5 822 / 5 814 / 5 830 queries/s (+4.4 %), replies unchanged; one
  // synchronous wire caller 4 790 against 4 936 (profiles/scan_pair_ab.txt): on.
  c->scan_pair = 1;
  if (const char* v = pirgpu_env("PIRGPU_SCAN_MFMA_PAIR"))
    if (*v) c->scan_pair = (uint32_t)std::min<long>(2, std::max<long>(0, strtol(v, nullptr, 10)));
  for (uint32_t j = 0; j < k; ++j) {
    c->scan_f64_fold = c->scan_f64_fold && (c->hp.mod[j].q >> 50) == 0;
    c->scan_f64_fold_batch = c->scan_f64_fold_batch && (c->hp.mod[j].q >> 50) == 0;
  }
  // selectors as doubles inside a lane: every query ciphertext must go through ks_last_ntt_kernel (>= 2 items each)
  const uint64_t rem = c->dim_sum % N;
  c->sel_f64 = c->want_sel_f64 && c->mfma_on && c->mode != kNttInt && c->fuse_last_level && c->last_level_ntt &&
               !c->split_upper && c->dim_sum >= 2 && rem != 1 && !c->ctm;   // (the products read u64 selectors)
  // ciphertext-multiplication mode
  if (c->ctm) c->ctm_scratch_words = (uint64_t)std::max<int64_t>(1, c->options.value(OPT_CT_SCRATCH_MB, 256)) * (1ull << 20) / 8;
  c->ctm_shared_sel = c->ctm && c->options.value(OPT_CT_SHARED_SEL, ctm_shared_sel_default(c)) != 0;
  // streamed database
  if (c->streamed && c->mfma_on) {
    const uint64_t mb = (uint64_t)std::max<int64_t>(0, c->options.value(OPT_DB_STREAM_MB, 256));
    c->stream_bands = std::min<uint64_t>(std::max<uint64_t>(1, (mb << 20) / stream_band_bytes(c)), 65535);
    c->mfma_single = true;   // the 64-bit kernels read the staging copy, which a streamed context never has
  }
}

void ensure_workspace(pirgpu_ctx* c) {
  if (c->ws_ready) return;
  const uint32_t N = c->N, k = c->k, d = c->d;

  const uint64_t m_max = std::min<uint64_t>(N, hm::next_power_two(std::max<uint32_t>(c->dim_sum, 1)));
  c->m_max = m_max;
  const uint64_t shard_pts = matrix_pts(c);
  // base-level scan geometry
  if (d == 1) {
    c->scan_rows = c->planes;
    c->scan_cols = (uint32_t)(shard_pts / c->planes);
  } else {
    c->scan_cols = c->dims[d - 1];
    c->scan_rows = (uint32_t)ceil_div(shard_pts, c->scan_cols);
  }
  c->scan_npt = shard_pts;
  resolve_options(c);
  // per-level node counts inside this shard and result buffers
  c->lvl_rows.assign(d, 0);
  c->lvl_cts.assign(d, 0);
  uint64_t pt_words = 0;
  for (uint32_t l = 0; l < d; ++l) {
    uint64_t rows = l == 0 ? c->planes : ceil_div(shard_pts, c->stride[l]);
    uint64_t C = 1;
    for (uint32_t x = l; x + 1 < d; ++x) C *= c->E;
    c->lvl_rows[l] = rows;
    c->lvl_cts[l] = std::max<uint64_t>(rows, 1) * C;
    if (l + 1 < d) {
      // chunk partial sums of upper_fused_kernel: n_chunks x (rows * C * E * 2 * k) polynomials
      const uint64_t per_chunk = std::max<uint64_t>(rows, 1) * (C / c->E) * c->E * k;
      const uint64_t n_chunks = std::min<uint64_t>(c->dims[l], std::max<uint64_t>(1, ceil_div(c->upper_blocks, per_chunk)));
      pt_words = std::max<uint64_t>(pt_words, (n_chunks + 1) * std::max<uint64_t>(rows, 1) * C * 2 * k * N);
    }
  }
  c->pt_words = pt_words;
  c->ws_ready = true;
  if (c->workers.empty()) c->workers.emplace_back();
  c->workers[0].stream = c->stream;
  for (Worker& w : c->workers) alloc_worker(c, w);
  ensure_expansion_buffers(c, c->workers[0]);  // worker 0 serves the single-query entry points and test hooks
  if (c->streamed && c->mfma_on) {
    // the only copy of a streamed database, allocated once the geometry is fixed.  Zero digits are the zero plaintext:
    // every padding row and column holds the bytes db_pack_band_kernel would store there, whichever ranges are loaded
    const size_t bytes = (size_t)c->nslots * c->mg.RT * c->mg.KG * c->mg.tile_bytes;
    c->d_dbp = c->dalloc<uint8_t>(bytes);
    c->dbp_alloc = bytes;
    note_mem(c);
    HIP_TRY(hipMemsetAsync(c->d_dbp, 0, bytes, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->packed_valid = true;
  }
}

// Expansion tree (ping/pong) and key-switch scratch of one worker, on first use.
void ensure_expansion_buffers(pirgpu_ctx* c, Worker& w) {
  if (w.res_a) return;
  const uint32_t N = c->N, k = c->k;
  w.res_a = c->dalloc<uint64_t>(c->m_max * c->ctw);
  w.res_b = c->dalloc<uint64_t>(c->m_max * c->ctw);
  w.prod = c->dalloc<uint64_t>(std::max<uint64_t>(c->m_max / 2, 1) * 2 * (k + 1) * N);
  w.dig = c->dalloc<uint64_t>(std::max<uint64_t>(c->m_max / 2, 1) * (k + 1) * k * N);
}

// Allocates one worker's buffers (and its stream unless it is the context's main stream).
void alloc_worker(pirgpu_ctx* c, Worker& w) {
  if (w.sv_ntt) return;
  const size_t ctw = c->ctw;
  if (!w.stream) HIP_TRY(hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));
  // the expansion tree / key-switch scratch is allocated on first use (ensure_expansion_buffers): in batch
  // mode the lanes expand, so only a worker that runs single queries needs its own
  w.sv_ntt = c->dalloc<uint64_t>((size_t)std::max<uint32_t>(c->dim_sum, 1) * ctw);
  w.d_query = c->dalloc<uint64_t>((size_t)(c->dim_sum / c->N + 1) * ctw);
  w.lvl.assign(c->d, nullptr);
  for (uint32_t l = 0; l < c->d; ++l) w.lvl[l] = c->dalloc<uint64_t>(c->lvl_cts[l] * ctw);
  if (c->rp || c->pack) w.last = c->dalloc<uint64_t>(c->lvl_cts[0] * ctw);
  if (c->pt_words) w.pt_buf = c->dalloc<uint64_t>(c->pt_words);
  const uint32_t parts = std::max<uint32_t>(c->scan_nsplit, c->mfma_on ? c->mg.nchunks : 1);
  if (parts > 1) w.scan_part = c->dalloc<uint64_t>((size_t)parts * std::max<uint32_t>(c->scan_rows, 1) * ctw);
  HIP_TRY(hipEventCreateWithFlags(&w.ev_expanded, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&w.ev_scanned, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&w.ev_done, hipEventDisableTiming));
}

// ======================================================================================================================
// [3] OBLIVIOUS EXPANSION (server.cpp:105-171): keys per query, expand_core, expand_query_to_sv
// ======================================================================================================================
uint32_t galois_inverse(uint32_t g, uint32_t N) {
  // (Z/2N)^* has exponent dividing N, so g^-1 = g^(N-1) mod 2N
  uint64_t mod = 2ull * N, r = 1, b = g % mod;
  uint32_t e = N - 1;
  while (e) {
    if (e & 1) r = (r * b) % mod;
    b = (b * b) % mod;
    e >>= 1;
  }
  return (uint32_t)r;
}

// The key sets a staged batch / the single-query selection name must still be the ones that were named: a set that was
// evicted or released since (its generation moved on) fails the run with FailedPrecondition instead of switching the
// query with the next tenant's keys.
uint32_t current_keyset(pirgpu_ctx* c) {
  const uint32_t i = c->cur_keyset;
  if (i >= c->keysets.size() || (i && c->keysets[i].gen != c->cur_keyset_gen))
    throw Fail{PIRGPU_FAILED_PRECONDITION, "stale key set handle: the selected set was evicted or released (claim it again)"};
  return i;
}
void check_staged_keysets(pirgpu_ctx* c) {
  BatchSet& b = c->bs();
  for (size_t q = 0; q < b.batch_keysets.size(); ++q) {
    const uint32_t i = b.batch_keysets[q];
    if (i >= c->keysets.size() || (i && q < b.batch_keyset_gens.size() && c->keysets[i].gen != b.batch_keyset_gens[q]))
      throw Fail{PIRGPU_FAILED_PRECONDITION,
                 "stale key set handle: a key set of the staged batch was evicted or released (pirgpu_batch_set_keysets again)"};
  }
}
// key set of query `query` (submission index) of the current batch; 0 where none was assigned (caller-owned selectors)
uint32_t keyset_of(pirgpu_ctx* c, uint32_t query) {
  const std::vector<uint32_t>& ks = c->bs().batch_keysets;
  return query < ks.size() ? ks[query] : 0;
}

const uint64_t* find_key(pirgpu_ctx* c, uint32_t slot, uint32_t g) {
  if (slot >= c->keysets.size()) throw Fail{PIRGPU_INVALID_ARGUMENT, "key set slot out of range"};
  auto& keys = c->keysets[slot].keys;
  auto it = keys.find(g);
  if (it == keys.end())
    throw Fail{PIRGPU_INTERNAL, "Galois key not present"};  // SEAL throws -> InternalError (server.cpp:72-74)
  return it->second;
}

// Keys for Galois element g of the B queries of a group (ksets[q] = key set slot of query q; nullptr: the context's
// current slot for all).  One client -> B = 1, the kernels then index a single pointer.
KeyPtrs keys_for(pirgpu_ctx* c, uint32_t g, const uint32_t* ksets, uint32_t B) {
  KeyPtrs kp{};
  bool same = true;
  for (uint32_t q = 0; q < B; ++q) {
    kp.p[q] = find_key(c, ksets ? ksets[q] : current_keyset(c), g);
    same = same && kp.p[q] == kp.p[0];
  }
  kp.B = same ? 1 : B;
  return kp;
}

void record(pirgpu_ctx* c, Worker& w, int idx) {
  if (c->prof_cur >= 0) HIP_TRY(hipEventRecord(c->ev[(size_t)c->prof_cur * (PH_COUNT + 1) + idx], w.stream));
}

void begin_profiled_run(pirgpu_ctx* c) {
  c->prof_cur = -1;
  if (!c->prof || c->prof_runs >= pirgpu_ctx::kMaxProfRuns) return;
  if (c->ev.empty()) {
    c->ev.resize((size_t)pirgpu_ctx::kMaxProfRuns * (PH_COUNT + 1));
    for (auto& e : c->ev) HIP_TRY(hipEventCreate(&e));
  }
  c->prof_cur = c->prof_runs++;
}

// NTT_j(x^(-shift)) for the k data moduli as doubles in device order (ks_last_ntt_kernel's X); built once per shift.
const uint64_t* xpow_table(pirgpu_ctx* c, hipStream_t st, uint32_t shift) {
  auto it = c->xpow.find(shift);
  if (it != c->xpow.end()) return it->second;
  const uint32_t N = c->N, k = c->k;
  std::vector<uint64_t> h((size_t)k * N, 0);
  for (uint32_t j = 0; j < k; ++j) h[(size_t)j * N + (N - shift)] = c->hp.mod[j].q - 1;   // x^(-s) = -x^(N-s)
  uint64_t* buf = c->dalloc<uint64_t>((size_t)k * N);
  HIP_TRY(hipMemcpy(buf, h.data(), h.size() * 8, hipMemcpyHostToDevice));
  HIP_TRY(c->ops->ntt_batch(st, c->mode, c->dp, buf, k, k, 0, false));
  HIP_TRY(launch_tree_convert(st, c->dp, c->mode, buf, buf, (uint64_t)k * N, true));
  HIP_TRY(hipStreamSynchronize(st));   // other streams use the table without an event
  c->xpow[shift] = buf;
  return buf;
}

// sigma_g acting on NTT-form data (ks_last_ntt_kernel, ks_combine_c0_ntt): SEAL position P holds the evaluation at
// psi^(2 br(P) + 1), so NTT(sigma_g(a)) = NTT(a) o pi_g with pi_g(P) = br(((2 br(P) + 1) g mod 2N - 1) / 2).  The table
// holds, for the thread that owns positions EPT t .. EPT t + EPT - 1, the PADDED LDS word index of pi_g(P)'s device slot
// (ntt_core.h lds_idx), first for g, then for g^-1; built once per Galois element.
const uint16_t* galois_perm_table(pirgpu_ctx* c, hipStream_t st, uint32_t g) {
  auto it = c->gperm.find(g);
  if (it != c->gperm.end()) return it->second;
  const uint32_t N = c->N, logN = c->logN, R = (uint32_t)ntt_log_ept((int)logN), EPT = 1u << R, NT = N >> R;
  auto brev = [&](uint32_t v) {
    uint32_t r = 0;
    for (uint32_t b = 0; b < logN; ++b) r |= ((v >> b) & 1u) << (logN - 1 - b);
    return r;
  };
  std::vector<uint16_t> h((size_t)2 * N);
  const uint32_t gs[2] = {g, galois_inverse(g, N)};
  for (int w = 0; w < 2; ++w)
    for (uint32_t P = 0; P < N; ++P) {
      const uint32_t ex = (uint32_t)(((uint64_t)(2 * brev(P) + 1) * gs[w]) & (2 * N - 1));
      const uint32_t Pin = brev(ex >> 1);
      const uint32_t slot = (Pin & (EPT - 1)) * NT + (Pin >> R);
      h[(size_t)w * N + P] = (uint16_t)(slot + (slot >> R));
    }
  uint16_t* buf = c->dalloc<uint16_t>((size_t)2 * N);
  HIP_TRY(hipMemcpy(buf, h.data(), h.size() * 2, hipMemcpyHostToDevice));
  HIP_TRY(hipStreamSynchronize(st));   // (hipMemcpy of pageable memory is synchronous; other streams use the table without an event)
  c->gperm[g] = buf;
  return buf;
}

// oblivious_expansion(ct, n) on the device (reference server.cpp:105-146).
// Input ciphertext must already be in res_a[0]; returns the buffer holding the
// next_power_two(n) results.
// B queries at once: ciphertext index = node * B + query, so every level is the same three launches
// over B times the nodes (the per-level Galois element and monomial shift are uniform).
// sel_dst (optional, fp64 flavours): per query, where selector 0 of this ciphertext's expansion goes (NTT form).  The
// last level then produces the selectors directly -- in the NTT domain (ks_last_ntt_kernel; the default) or fused with
// their forward transform (ks_last_level_kernel) -- and nullptr is returned: there is no coefficient-form result to
// transform any more.  sel_f64: selectors written as exact doubles (a batch lane's own consumers only).
// Levels: narrow ones digit -> products of all moduli -> combine; wide ones digit -> special-prime product -> data
// products + combine in one kernel, the tree between two such levels in 5-byte polynomials (cur40).
// A tree in the middle of its expansion: handed from the head stream's levels to the lane's (HeadSlot).
struct TreeState {
  uint64_t* cur = nullptr;   // buffer holding the current level's ciphertexts
  bool cur40 = false;        // ... as 5-byte polynomials (between fused levels) instead of doubles
  bool c0ntt = false;        // ... with their c0 polynomials in NTT form (fused levels, ks_combine_c0_ntt)
};

// The context's resolved options as the plan (expansion_plan.h) reads them.
static ExpandOptions expand_options(const pirgpu_ctx* c) {
  ExpandOptions o;
  o.mode = c->mode;
  o.fuse_last_level = c->fuse_last_level;
  o.last_level_ntt = c->last_level_ntt;
  o.fuse_mac_combine = c->fuse_mac_combine;
  o.fuse_mac_nodes = c->fuse_mac_nodes;
  o.tree40 = c->tree40;
  o.pack40 = c->pack40;
  o.c0_ntt = c->c0_ntt;
  o.c0_ntt_split = c->c0_ntt_split;
  o.loop_transforms = c->loop_transforms;
  o.loop_min_sources = c->loop_min_sources;
  return o;
}

// Levels [j_begin, j_end) of the tree (j_end clamped to the tree's depth).  `from` (j_begin > 0): where the earlier levels
// left the tree -- that buffer is only READ; the first level here writes res_a, later ones ping-pong res_a / res_b.
// `to` (j_end < depth): receives the state after level j_end - 1 instead of the function running to the leaves.
// after_first: called when the first level's launches are queued (the `from` buffer may be recycled behind them).
uint64_t* expand_core(pirgpu_ctx* c, hipStream_t st, uint64_t* res_a, uint64_t* res_b, uint64_t* dig, uint64_t* prod,
                      uint32_t n, uint32_t B, const MfmaPtrs* sel_dst = nullptr, bool sel_f64 = false,
                      const uint32_t* ksets = nullptr, uint32_t j_begin = 0, uint32_t j_end = UINT32_MAX,
                      const TreeState* from = nullptr, TreeState* to = nullptr,
                      const std::function<void()>& after_first = nullptr) {
  const uint32_t N = c->N, k = c->k;
  if (n > N) throw Fail{PIRGPU_INVALID_ARGUMENT, "Cannot expand more items from a CT than poly modulus degree"};
  const ExpandOptions eo = expand_options(c);
  if (sel_f64 && !(sel_dst && eo.mode != kNttInt && eo.fuse_last_level && eo.last_level_ntt && n >= 2))
    throw Fail{PIRGPU_INTERNAL, "double-form selectors need the NTT-domain last level"};
  uint64_t *cur = res_a, *nxt = res_b;
  TreeFlags in;
  if (from) {
    cur = from->cur;
    in.cur40 = from->cur40;
    in.c0ntt = from->c0ntt;
    nxt = res_a;
  }
  // every decision of the walk (forms, 5-byte tree, c0 in NTT form, looped transforms) is the plan's: expansion_plan.h
  const ExpandPlan plan = plan_expansion(N, c->logN, k, B, n, sel_dst != nullptr, eo, j_begin, j_end, from ? &in : nullptr);
  for (const ExpandLevel& L : plan.levels) {
    const uint32_t j = L.j, nodes = L.nodes;
    const uint32_t g = (N >> j) + 1;
    const KeyPtrs key = keys_for(c, g, ksets, B);   // per query of the group: its own client's key
    if (L.invalid == kTree40Unreadable) throw Fail{PIRGPU_INTERNAL, "5-byte tree reached a level that cannot read it"};
    // (never in a buffer handed over by another stream: `from` is read-only; its owner converted it after ITS last level)
    if (L.c0_before) HIP_TRY(c->ops->tree_c0_fwd(st, c->mode, c->dp, k, cur, nodes));
    HIP_TRY(c->ops->ks_digit(st, c->mode, c->dp, k, cur, g, nodes, dig, c->pack40, L.c0_in_digit ? prod : nullptr, L.tin40,
                             L.loop_targets));
    if (L.invalid == kTree40Unfused) throw Fail{PIRGPU_INTERNAL, "5-byte tree reached an unfused level"};
    if (L.invalid == kC0NttUnfused) throw Fail{PIRGPU_INTERNAL, "NTT-form c0 reached an unfused level"};
    HIP_TRY(c->ops->ks_mac_intt(st, c->mode, c->dp, k, dig, key, nodes, prod, c->pack40, L.mac_base, L.mac_count));
    switch (L.form) {
      case kLevelFused:
        // special-prime product first (the only one that goes through HBM), then the data residues with the combine
        // step in their epilogue: no data products in HBM, no separate combine pass
        HIP_TRY(c->ops->ks_mac_combine(st, c->mode, c->dp, k, dig, key, prod, cur, g, nodes, 1u << j, nxt, c->pack40, L.tin40,
                                       L.tout40, L.c0ntt() ? xpow_table(c, st, 1u << j) : nullptr,
                                       L.c0ntt() ? galois_perm_table(c, st, g) : nullptr, c->c0_ntt_split));
        break;
      case kLevelLastNtt: {
        // last level in the NTT domain: only the special-prime product is inverse-transformed
        const uint64_t* X = xpow_table(c, st, 1u << j);
        HIP_TRY(c->ops->ks_last_ntt(st, c->mode, c->dp, k, cur, dig, key, prod, X, g, galois_inverse(g, N), 1u << j, n, B,
                                    *sel_dst, nodes, c->pack40, sel_f64, L.c0_in_digit, L.c0ntt() ? (L.tin40 ? 2 : 1) : 0,
                                    galois_perm_table(c, st, g)));
        return nullptr;
      }
      case kLevelLastCoeff:
        HIP_TRY(c->ops->ks_last_level(st, c->mode, c->dp, k, cur, prod, g, 1u << j, n, B, *sel_dst, nodes, c->pack40));
        return nullptr;
      case kLevelUnfused:
        HIP_TRY(launch_ks_combine(st, c->dp, c->mode, N, k, cur, prod, galois_inverse(g, N), nodes, 1u << j, true, L.hi_limit,
                                  c->pack40, nxt, c->pack_bytes));
        break;
    }
    std::swap(cur, nxt);
    if (L.c0_after) HIP_TRY(c->ops->tree_c0_fwd(st, c->mode, c->dp, k, cur, nodes * 2));
    // (picking a tree up from another buffer: after its first level here the ping-pong is res_a <-> res_b)
    if (from && j == j_begin) {
      nxt = res_b;
      if (after_first) after_first();
    }
  }
  if (to) {
    to->cur = cur;
    to->cur40 = plan.out.cur40;
    to->c0ntt = plan.out.c0ntt;
  }
  return cur;
}

uint64_t* expand_on_device(pirgpu_ctx* c, Worker& w, uint32_t n) {
  ensure_expansion_buffers(c, w);
  return expand_core(c, w.stream, w.res_a, w.res_b, w.dig, w.prod, n, 1, nullptr, false, &w.keyset);
}

// expansion of all staged query ciphertexts into sv_ntt (NTT form) -- reference
// server.cpp:148-171 followed by the lazy transform_to_ntt_inplace of
// database.cpp:190,222 applied to every selector.
void expand_query_to_sv(pirgpu_ctx* c, Worker& w, const uint64_t* d_query, uint32_t nq) {
  ensure_expansion_buffers(c, w);
  w.sv_cur = nullptr;
  w.sv_rows = nullptr;
  const uint32_t N = c->N, k = c->k;
  const size_t ctw = c->ctw;
  uint64_t remaining = c->dim_sum;
  uint64_t produced = 0;
  for (uint32_t q = 0; q < nq; ++q) {
    uint32_t n = (uint32_t)std::min<uint64_t>(remaining, N);
    if (n > 0) {
      // the query ciphertext (canonical u64) becomes the root of the expansion tree (the tree's element type)
      HIP_TRY(launch_tree_convert(w.stream, c->dp, c->mode, d_query + (size_t)q * ctw, w.res_a, ctw, true));
      MfmaPtrs dst{};
      dst.p[0] = w.sv_ntt + produced * ctw;
      uint64_t* res = expand_core(c, w.stream, w.res_a, w.res_b, w.dig, w.prod, n, 1, &dst, false, &w.keyset);
      if (res) HIP_TRY(c->ops->ct_ntt_fwd_oop(w.stream, c->mode, c->dp, k, res, w.sv_ntt + produced * ctw, n, true));
    }
    produced += n;
    remaining -= n;
    if (remaining == 0) break;
  }
}

// ======================================================================================================================
// [4] MULTIPLY (database.cpp:170-258): the scan (scan_group_mfma / scan_on_device) and everything after it (post_scan_stage)
// ======================================================================================================================
// PIRDatabase::multiply on the device (reference database.cpp:170-258), with the
// selection vector already in NTT form in sv_ntt.  Leaves the reply in lvl[0].
// selectors of the scanned (last) dimension for this worker's query
const uint64_t* scan_selectors(pirgpu_ctx* c, Worker& w) {
  const uint64_t* sv = w.sv_cur ? w.sv_cur : w.sv_ntt;
  return sv + (size_t)c->sv_off[c->d - 1] * c->ctw + (c->d == 1 ? (size_t)c->sb * c->ctw : 0);
}

bool mq_usable(pirgpu_ctx* c) { return c->scan_nsplit == 1 && c->scan_rows >= 1 && c->scan_cols >= 1; }

// bytes of the operand-layout copy this context holds (its slots of every plaintext)
// (contexts with tables: the bytes of ONE table's layout; table t starts t times that far into d_dbp)
size_t dbp_bytes(const pirgpu_ctx* c) { return (size_t)c->nslots * c->mg.RT * c->mg.KG * c->mg.tile_bytes; }
uint8_t* table_dbp(const pirgpu_ctx* c, uint32_t t) { return c->d_dbp ? c->d_dbp + (size_t)t * dbp_bytes(c) : nullptr; }

// Contexts with tables serve one GPU: the multi-GPU steps (u64 and packed exchange, slot shards) do not name tables.
void refuse_tables(const pirgpu_ctx* c) {
  if (c->tables > 1)
    throw Fail{PIRGPU_FAILED_PRECONDITION, "this context holds several tables (tables > 1): the multi-GPU entry points do "
                                           "not serve them"};
}

// A slot shard holds 1 / G of every plaintext: it serves the pirgpu_slots_* step only.
// Wide items are served by one GPU: the multi-GPU steps (packed row-shard exchange, slot shards) do not know planes.
void refuse_wide(const pirgpu_ctx* c) {
  if (c->planes > 1)
    throw Fail{PIRGPU_FAILED_PRECONDITION, "this context holds wide items (plaintexts_per_item > 1): the multi-GPU entry "
                                           "points do not serve them"};
}

// Modulus switching does not commute with the sum over shards: a context with result_primes serves one GPU.
void refuse_switched(const pirgpu_ctx* c) {
  if (c->rp)
    throw Fail{PIRGPU_FAILED_PRECONDITION, "this context switches its results to fewer primes (result_primes > 0): the "
                                           "multi-GPU entry points do not serve it"};
}

// Ciphertext-multiplication mode serves one GPU (the rounding of a product does not commute with the sum over shards).
void refuse_ctm(const pirgpu_ctx* c) {
  if (c->ctm)
    throw Fail{PIRGPU_FAILED_PRECONDITION, "this context multiplies ciphertexts (PIRGPU_CREATE_CT_MULTIPLY): the multi-GPU "
                                           "entry points do not serve it"};
}

// Packed replies serve one GPU and hand out packed words: what sums replies over shards, or copies them to a device
// buffer whose reader expects residues, does not serve them.
void refuse_packed(const pirgpu_ctx* c) {
  if (c->pack)
    throw Fail{PIRGPU_FAILED_PRECONDITION, "this context packs its replies (PIRGPU_CREATE_PACKED_REPLIES, PIRGPU_CREATE_CT_COMPACT_REPLY): the multi-GPU "
                                           "entry points and the device reply copies do not serve it"};
}

// d = 1 with result_primes or packed replies: the scan's sums are level 0 at k primes -- they go to the worker's `last` buffer
uint64_t* scan_out(const pirgpu_ctx* c, Worker& w) { return (c->rp || c->pack) && c->d == 1 ? w.last : w.lvl[c->d - 1]; }

void refuse_slot_shard(const pirgpu_ctx* c) {
  if (c->slot_sharded)
    throw Fail{PIRGPU_FAILED_PRECONDITION, "this context is a slot shard: it serves the pirgpu_slots_* entry points only"};
}

// Brings the operand-layout copy of the database up to date (after loads); one-time cost per load.
void ensure_packed(pirgpu_ctx* c) {
  if (!c->mfma_on || c->packed_valid) return;
  if (c->streamed)   // (its operand layout is valid from ensure_workspace on; there is no staging copy to pack from)
    throw Fail{PIRGPU_INTERNAL, "streamed database without its operand-layout copy"};
  if (!c->d_dbp) {
    c->d_dbp = c->dalloc<uint8_t>(c->tables * dbp_bytes(c));
    c->dbp_alloc = c->tables * dbp_bytes(c);
    note_mem(c);
  }
  if (c->tables > 1) {
    // every table is a complete layout of its own: the band kernel with table t's staging rows as its source and table
    // t's layout as its destination.  Only the tables a load touched since are packed again
    for (uint32_t t = 0; t < c->tables; ++t) {
      if (c->tbl_packed[t]) continue;
      HIP_TRY(launch_db_pack(c->stream, c->dp, c->mg, table_db(c, t), table_dbp(c, t), c->scan_rows, c->scan_cols,
                             c->k * c->N, 0, c->nslots));
      c->tbl_packed[t] = 1;
    }
  } else {
    HIP_TRY(launch_db_pack(c->stream, c->dp, c->mg, c->d_db, c->d_dbp, c->scan_rows, c->scan_cols, c->k * c->N, c->slot0,
                           c->nslots));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->packed_valid = true;
}

// Streamed database: the first load fixes the geometry like a first query does; without the int8 scan there is no
// operand layout to load into.  Waits for every queued use of the database (a reload overwrites it).
void begin_streamed_load(pirgpu_ctx* c) {
  ensure_workspace(c);
  if (!c->mfma_on)
    throw Fail{PIRGPU_FAILED_PRECONDITION,
               "a streamed database needs the int8-MFMA scan (d >= 2, at least 8 rows, moduli below 2^55, option "
               "SCAN_MFMA not 0): this context scans with the 64-bit kernels, which read the staging copy"};
  if (!c->d_dbp) throw Fail{PIRGPU_INTERNAL, "streamed database without its operand-layout copy"};
  sync_batch_streams(c);
  HIP_TRY(hipStreamSynchronize(c->stream));
}

// Plaintexts per load chunk of a streamed context: whole row bands, no more than `pts` plaintexts need
uint64_t stream_chunk_pts(const pirgpu_ctx* c, uint64_t bands, uint64_t pts) {
  const uint64_t tile = 16ull * c->scan_cols;
  return std::min<uint64_t>(std::max<uint64_t>(bands, 1), std::max<uint64_t>(ceil_div(pts, tile), 1)) * tile;
}
// DbUnits of the ragged head and tail of one pack_range call: each lies inside one row tile
uint64_t stream_unit_bytes(const pirgpu_ctx* c) { return 2ull * 16 * c->mg.KG * sizeof(DbUnit); }

// Streamed load: stores n consecutive plaintexts of the scanned matrix' row-major order, already encoded in the compact
// buffer d_enc[n][k][N], first one at position l0 (db_row), into the operand layout.  The part of the range that covers
// whole row tiles -- 16 * scan_cols aligned plaintexts, or the last, short tile when the range ends where the matrix
// ends (what follows is padding) -- goes through the band kernel: full-tile stores, d_dbp is not read.  The ragged head
// and tail share their tiles with plaintexts outside the range: they go through the read-modify-write column update
// (launch_db_pack_update) with units built here.  d_units: stream_unit_bytes(c) of device scratch.
void pack_range(pirgpu_ctx* c, const uint64_t* d_enc, uint64_t l0, uint64_t n, DbUnit* d_units) {
  if (!n) return;
  const uint32_t kN = c->k * c->N, cols = c->scan_cols;
  const uint64_t tile = 16ull * cols, end = l0 + n;
  if (end > c->scan_npt) throw Fail{PIRGPU_INTERNAL, "pack_range: range past the scanned matrix"};
  const uint64_t head_end = std::min(ceil_div(l0, tile) * tile, end);
  const uint64_t body_end = end == c->scan_npt ? end : std::max(head_end, end / tile * tile);
  std::vector<DbUnit> units[2];
  auto ragged = [&](int which, uint64_t x0, uint64_t x1) {
    std::vector<DbUnit>& u = units[which];
    for (uint64_t l = x0; l < x1; ++l) {
      const uint32_t r = (uint32_t)(l / cols), col = (uint32_t)(l % cols), kg = col / 16;
      if (u.empty() || u.back().r != r || u.back().kg != kg) u.push_back(DbUnit{r, kg, 0u, (uint32_t)(l - l0)});
      u.back().mask |= 1u << (col % 16);
    }
    DbUnit* d = d_units + (size_t)which * 16 * c->mg.KG;
    HIP_TRY(hipMemcpyAsync(d, u.data(), u.size() * sizeof(DbUnit), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_db_pack_update(c->stream, c->dp, c->mg, d_enc, d, (uint32_t)u.size(), c->d_dbp, kN, c->slot0, c->nslots));
  };
  if (head_end > l0) ragged(0, l0, head_end);
  if (body_end > head_end)
    HIP_TRY(launch_db_pack_band(c->stream, c->dp, c->mg, d_enc + (head_end - l0) * kN, c->d_dbp, (uint32_t)(head_end / tile),
                                (uint32_t)ceil_div(body_end - head_end, tile), body_end - head_end, cols, kN, c->slot0,
                                c->nslots));
  if (end > body_end) ragged(1, body_end, end);
  HIP_TRY(hipStreamSynchronize(c->stream));   // the unit lists above are read by the copies queued here
}

// A database pass of the batch pipeline on stream `st`: counted (SCAN_LAUNCHES) and, while profiling is on, timed between
// two events for pirgpu_batch_scan_timings -- the first kMaxBscan launches, with the workgroups and queries of the last.
template <typename Launch>
void timed_scan_launch(pirgpu_ctx* c, hipStream_t st, uint32_t wgs, uint32_t nq, Launch&& launch) {
  constexpr uint32_t kMaxBscan = 64;
  const bool timed = c->prof && c->bscan_n < kMaxBscan;
  if (timed) {
    while (c->bscan_ev.size() < 2 * (size_t)(c->bscan_n + 1)) {
      hipEvent_t e;
      HIP_TRY(hipEventCreate(&e));
      c->bscan_ev.push_back(e);
    }
    HIP_TRY(hipEventRecord(c->bscan_ev[2 * c->bscan_n], st));
  }
  launch();
  ++c->options.counter(OPT_SCAN_LAUNCHES);
  if (timed) {
    HIP_TRY(hipEventRecord(c->bscan_ev[2 * c->bscan_n + 1], st));
    ++c->bscan_n;
    c->bscan_wgs = wgs;
    c->bscan_nq = nq;
  }
}

// One pass of the MFMA scan for up to 8 queries (the caller has ordered stream `st` after their expansions): pack
// the column selectors (unless they arrive packed), scan, fold column chunks.  Row sums of query q go to
// out + q * scan_rows ciphertexts; `part` (query-major as well) holds the per-chunk sums of matrices wider than one chunk.
void scan_group_mfma(pirgpu_ctx* c, hipStream_t st, uint8_t*& selp, const MfmaPtrs& col_sel, uint32_t n, uint64_t* out_base,
                     uint64_t* part, Worker* profiled, const uint8_t* packed = nullptr, bool sel_f64 = false,
                     bool share_chip = false, uint32_t table = 0) {
  const uint32_t kN = c->k * c->N;
  const uint64_t words = (uint64_t)c->scan_rows * c->ctw;
  ensure_packed(c);
  // query q of the group writes at out + q * qstride: the lane's row sums, or -- matrices wider than one chunk -- its
  // per-chunk partial sums
  uint64_t* const out = c->mg.nchunks > 1 ? part : out_base;
  const uint64_t out_qstride = c->mg.nchunks > 1 ? (uint64_t)c->mg.nchunks * words : words;
  if (!packed) {  // with `packed` the group's digit-packed column selectors already exist (multi-GPU exchange)
    if (!selp) selp = c->dalloc<uint8_t>(c->mg.sel_bytes);
    HIP_TRY(launch_sel_pack(st, c->dp, c->mg, col_sel, n, selp, c->scan_cols, kN, sel_f64));
    packed = selp;
  }
  if (profiled) record(c, *profiled, PH_SCAN);  // selector packing counts as selector preparation, not as the scan
  // batch pipeline: the pass runs on part of the chip and overlaps the other lane's transform kernels whenever the
  // call that queued it has a second group for the other lane (share_chip: decided from the batch's shape, not from
  // the streams' state at enqueue time); a lone group gets the whole chip
  const bool share = share_chip && !profiled && c->scan_wgs_batch;
  const uint32_t wgs = share ? c->scan_wgs_batch : 0;
  auto launch = [&] {
    HIP_TRY(launch_scan_mfma(st, c->dp, c->mg, table_dbp(c, table), packed, out, out_qstride, n, c->scan_rows, kN, words, wgs,
                             n > 1 ? (c->scan_f64_fold || c->scan_f64_fold_batch) : c->scan_f64_fold));
  };
  // (a profiled single query has its own phase timings and is no batch pass: not counted, not timed here)
  if (profiled) launch();
  else timed_scan_launch(c, st, wgs, n, launch);
  if (c->mg.nchunks > 1)
    HIP_TRY(launch_reduce_splits(st, c->dp, part, c->mg.nchunks, words, out_base, n, (uint64_t)c->mg.nchunks * words, words));
}

// The same pass for TWO groups on one lane (scan_mfma_pair.hip): both groups' column selectors are packed, then ONE launch
// multiplies every database tile it reads with both.  Half h's row sums go to hv[h].rows, query-major.  One column chunk.
static void scan_pair_mfma(pirgpu_ctx* c, BatchLane& ln, const GroupHalf (&hv)[2], bool sel_f64, bool share_chip) {
  const uint32_t kN = c->k * c->N;
  const uint64_t words = (uint64_t)c->scan_rows * c->ctw;
  hipStream_t st = ln.stream;
  ensure_packed(c);
  if (!ln.selp) ln.selp = c->dalloc<uint8_t>(c->mg.sel_bytes);
  uint8_t* const selp[2] = {ln.selp, ln.selp2};
  ScanGroups grp{};
  grp.n = 2;
  for (uint32_t h = 0; h < 2; ++h) {
    HIP_TRY(launch_sel_pack(st, c->dp, c->mg, hv[h].col, hv[h].n, selp[h], c->scan_cols, kN, sel_f64));
    grp.sel[h] = selp[h];
    grp.out[h] = hv[h].rows;
    grp.nq[h] = (uint8_t)hv[h].n;
  }
  const uint32_t wgs = share_chip && c->scan_wgs_batch ? c->scan_wgs_batch : 0;
  timed_scan_launch(c, st, wgs, hv[0].n + hv[1].n, [&] {
    HIP_TRY(launch_scan_mfma_pair(st, c->dp, c->mg, c->d_dbp, grp, c->scan_rows, words, wgs,
                                  c->scan_f64_fold || c->scan_f64_fold_batch, 0, kN, words, kN));
  });
}

// Base case of PIRDatabase::multiply (reference database.cpp:185-194,238-247): one fused
// multiply_plain + add_inplace pass over the database.  Leaves NTT-form row sums in lvl[d-1].
void scan_on_device(pirgpu_ctx* c, Worker& w) {
  const uint32_t N = c->N, k = c->k;
  const size_t ctw = c->ctw;
  refuse_slot_shard(c);
  if (!table_loaded(c, w.table))
    throw Fail{PIRGPU_FAILED_PRECONDITION, c->tables > 1 ? "table " + std::to_string(w.table) + " not fully loaded"
                                                         : std::string("database not fully loaded")};
  check_transparent(c, w.table);
  if (c->pt_end == c->pt_begin) return;
  if (c->mfma_on && c->mfma_single) {
    MfmaPtrs col{};
    col.p[0] = scan_selectors(c, w);
    scan_group_mfma(c, w.stream, w.selp, col, 1, scan_out(c, w), w.scan_part, &w, nullptr, false, false, w.table);
    return;
  }
  const uint64_t* sv_base = scan_selectors(c, w);
  uint64_t* base_out = scan_out(c, w);
  const uint64_t* db = table_db(c, w.table);   // the 64-bit scans take the table as an offset into the staging copy
  if (c->mq_single && mq_usable(c)) {
    HIP_TRY(launch_scan_mq(w.stream, c->dp, N, k, db, &sv_base, &base_out, 1, c->scan_rows, c->scan_cols,
                           c->mq_single_rows, c->mq_single_limb && c->scan_limb));
    return;
  }
  uint64_t* scan_out = c->scan_nsplit > 1 ? w.scan_part : base_out;
  HIP_TRY(launch_scan(w.stream, c->dp, N, k, db, sv_base, scan_out, c->scan_rows, c->scan_cols, c->scan_npt,
                      c->scan_nsplit, c->scan_cps, c->scan_rpt, c->scan_block, c->scan_limb));
  if (c->scan_nsplit > 1)
    HIP_TRY(launch_reduce_splits(w.stream, c->dp, w.scan_part, c->scan_nsplit, (uint64_t)c->scan_rows * ctw,
                                 base_out));
}

// ---- ciphertext-multiplication mode: products of one block of pairs in an owner's scratch ----
// Regions of the scratch for `cap` pairs.  The tree-form input of the key switch reuses xq, its output yq: both are dead
// once the tensor / the scale kernel has read them.
struct CtmRegions {
  uint64_t *xq, *xb, *yq, *yb, *d, *dig, *prod;
};
size_t ctm_pair_words(const pirgpu_ctx* c) {
  const size_t k = c->k, kb = c->kb;
  return (4 * k + 4 * kb + 3 * k + 3 * kb + 3 * k + (k + 1) * k + 2 * (k + 1)) * c->N;
}
uint32_t ctm_cap_pairs(const pirgpu_ctx* c) {
  return (uint32_t)std::min<uint64_t>(16383, std::max<uint64_t>(kMaxMfmaQueries, c->ctm_scratch_words / ctm_pair_words(c)));
}
CtmRegions ctm_regions(const pirgpu_ctx* c, uint64_t* buf, size_t cap) {
  const size_t k = c->k, kb = c->kb, N = c->N;
  CtmRegions r;
  r.xq = buf;
  r.xb = r.xq + cap * 4 * k * N;
  r.yq = r.xb + cap * 4 * kb * N;
  r.yb = r.yq + cap * 3 * k * N;
  r.d = r.yb + cap * 3 * kb * N;
  r.dig = r.d + cap * 3 * k * N;
  r.prod = r.dig + cap * (k + 1) * k * N;
  return r;
}
CtmScratch& ctm_scratch(pirgpu_ctx* c, hipStream_t st) {
  if (!c->ctm) throw Fail{PIRGPU_FAILED_PRECONDITION, "not a ciphertext-multiplication context (pirgpu_create_ex with PIRGPU_CREATE_CT_MULTIPLY)"};
  CtmScratch& ws = c->ctm_ws[st];
  if (!ws.buf) {
    ws.words = (size_t)ctm_cap_pairs(c) * ctm_pair_words(c);
    ws.buf = c->dalloc<uint64_t>(ws.words);
    uint32_t dmax = 1;
    for (uint32_t l = 0; l + 1 < c->d; ++l) dmax = std::max(dmax, c->dims[l]);
    ws.selc_words = (size_t)kMaxMfmaQueries * dmax * c->ctw;
    ws.selc = c->dalloc<uint64_t>(ws.selc_words);
    if (c->ctm_shared_sel) ws.selb = c->dalloc<uint64_t>((size_t)kMaxMfmaQueries * dmax * 2 * c->kb * c->N);
  }
  return ws;
}

// n pairs (pair p = jj * nq + q: ciphertext a + q * a_qstride + (j0 + jj) * ctw times selector b + (q * dim + (j0 + jj) %
// dim) * ctw, all coefficient form) -> r.d [n][d0, d2, d1][k][N]: lift, transforms at Q and B, tensor, inverse
// transforms, scale.
void ctm_products(pirgpu_ctx* c, hipStream_t st, const CtmRegions& r, const uint64_t* a, uint64_t a_qstride, const uint64_t* b,
                  uint32_t dim, uint32_t nq, uint32_t j0, uint32_t n) {
  const uint32_t N = c->N, k = c->k, kb = c->kb;
  HIP_TRY(launch_ctm_lift(st, c->d_ctm, k, N, a, a_qstride, b, dim, nq, j0, n, r.xq, r.xb));
  HIP_TRY(c->ops->ntt_batch(st, c->mode, c->dp, r.xq, (uint64_t)n * 4 * k, k, 0, false));
  HIP_TRY(c->ops->ntt_batch(st, c->mode, c->dp_aux, r.xb, (uint64_t)n * 4 * kb, kb, 0, false));
  HIP_TRY(launch_ctm_tensor(st, c->dp, k, N, r.xq, r.yq, n));
  HIP_TRY(launch_ctm_tensor(st, c->dp_aux, kb, N, r.xb, r.yb, n));
  HIP_TRY(c->ops->ntt_batch(st, c->mode, c->dp, r.yq, (uint64_t)n * 3 * k, k, 0, true));
  HIP_TRY(c->ops->ntt_batch(st, c->mode, c->dp_aux, r.yb, (uint64_t)n * 3 * kb, kb, 0, true));
  HIP_TRY(launch_ctm_scale(st, c->d_ctm, k, N, r.yq, r.yb, r.d, n));
}

// The selectors of one level and group for the shared-selector path (CT_SHARED_SEL): per query, the NTT-form pair array
// [dim][2][km][N] at Q -- the selection vector as the last expansion level wrote it (canonical residues in the order
// ntt_batch emits) -- and at B (CtmScratch::selb).
struct CtmSel {
  CtmSelPtrs q, b;
};
// ctm_products with the selectors given in NTT form at both bases: only the ciphertext half of every pair is lifted and
// transformed, into the first half of r.xq / r.xb (the regions keep the size of the four-polynomial path, so that blocks
// are cut at the same children either way).
void ctm_products_sel(pirgpu_ctx* c, hipStream_t st, const CtmRegions& r, const uint64_t* a, uint64_t a_qstride,
                      const CtmSel& sel, uint32_t dim, uint32_t nq, uint32_t j0, uint32_t n) {
  const uint32_t N = c->N, k = c->k, kb = c->kb;
  HIP_TRY(launch_ctm_lift_polys(st, c->d_ctm, k, N, a, a_qstride, nq, j0, n, r.xq, r.xb));
  HIP_TRY(c->ops->ntt_batch(st, c->mode, c->dp, r.xq, (uint64_t)n * 2 * k, k, 0, false));
  HIP_TRY(c->ops->ntt_batch(st, c->mode, c->dp_aux, r.xb, (uint64_t)n * 2 * kb, kb, 0, false));
  HIP_TRY(launch_ctm_tensor_sel(st, c->dp, k, N, r.xq, sel.q, dim, nq, j0, r.yq, n));
  HIP_TRY(launch_ctm_tensor_sel(st, c->dp_aux, kb, N, r.xb, sel.b, dim, nq, j0, r.yb, n));
  HIP_TRY(c->ops->ntt_batch(st, c->mode, c->dp, r.yq, (uint64_t)n * 3 * k, k, 0, true));
  HIP_TRY(c->ops->ntt_batch(st, c->mode, c->dp_aux, r.yb, (uint64_t)n * 3 * kb, kb, 0, true));
  HIP_TRY(launch_ctm_scale(st, c->d_ctm, k, N, r.yq, r.yb, r.d, n));
}

// Deferred rounding (PIRGPU_CREATE_CT_DEFERRED), one block: the children [j0, j0 + nj) of every query are lifted and
// transformed as above; their tensors are summed per row in the NTT domain, at Q into r.yq and at B into r.yb
// (accumulator (row - j0 / dim) * nq + q; a row begun in an earlier block is accumulator 0 .. nq - 1 and is added to).  The
// rows whose last child (of nch in all) lies in the block are then transformed back and scaled:
// r.d [finished * nq][d0, d2, d1][k][N], row-major, query-minor.  Returns the number of finished rows; the first of them
// is row j0 / dim.  A row cut by the block's end stays behind them: ctm_carry_row moves it to the front for the next
// block, once the caller is done with r.yq (the key switch writes its output there).
constexpr uint64_t kCtmRowsumWgs = 512;   // two workgroups per CU
uint32_t ctm_rowsum_block(pirgpu_ctx* c, hipStream_t st, const CtmRegions& r, uint32_t cap, const uint64_t* a,
                          uint64_t a_qstride, const uint64_t* b, uint32_t dim, uint32_t nq, uint64_t nch, uint32_t j0, uint32_t nj,
                          const CtmSel* sel = nullptr) {   // sel: the shared-selector path (b is not read)
  const uint32_t N = c->N, k = c->k, kb = c->kb, n = nj * nq;
  const uint64_t end = (uint64_t)j0 + nj;
  const uint32_t row0 = j0 / dim, rows = (uint32_t)((end - 1) / dim) - row0 + 1;
  const bool cut = end < nch && end % dim != 0;   // the last row goes on in the next block
  const uint32_t fin = rows - (cut ? 1 : 0);
  // few rows in flight: below two workgroups per CU a row's children are shared out over several workgroups (partial
  // accumulators behind the block's own, folded by a second launch; modular sums are exact in any order)
  const uint64_t wgs = (uint64_t)rows * nq * k * (N / 256);
  const uint64_t room = (uint64_t)cap / ((uint64_t)rows * nq);   // accumulators per row and query: its own + the partial sums
  uint32_t splits = (uint32_t)std::min<uint64_t>({ceil_div(kCtmRowsumWgs, wgs), (uint64_t)nj, room ? room - 1 : 0});
  // option CT_ROWSUM_SPLITS (A/B, tests): at most this many workgroups share a row's children; 1: never split; 0: as above
  const int64_t most = c->ctm_rowsum_splits;
  if (most > 0) splits = (uint32_t)std::min<int64_t>(splits, most);
  if (splits < 2) splits = 1;
  if ((uint64_t)(splits > 1 ? splits + 1 : 1) * rows * nq > cap) throw Fail{PIRGPU_INTERNAL, "row-sum accumulators exceed the product scratch"};
  if (sel) {
    HIP_TRY(launch_ctm_lift_polys(st, c->d_ctm, k, N, a, a_qstride, nq, j0, n, r.xq, r.xb));
    HIP_TRY(c->ops->ntt_batch(st, c->mode, c->dp, r.xq, (uint64_t)n * 2 * k, k, 0, false));
    HIP_TRY(c->ops->ntt_batch(st, c->mode, c->dp_aux, r.xb, (uint64_t)n * 2 * kb, kb, 0, false));
    HIP_TRY(launch_ctm_tensor_rowsum_sel(st, c->dp, k, N, r.xq, sel->q, r.yq, dim, nq, j0, nj, splits));
    HIP_TRY(launch_ctm_tensor_rowsum_sel(st, c->dp_aux, kb, N, r.xb, sel->b, r.yb, dim, nq, j0, nj, splits));
  } else {
    HIP_TRY(launch_ctm_lift(st, c->d_ctm, k, N, a, a_qstride, b, dim, nq, j0, n, r.xq, r.xb));
    HIP_TRY(c->ops->ntt_batch(st, c->mode, c->dp, r.xq, (uint64_t)n * 4 * k, k, 0, false));
    HIP_TRY(c->ops->ntt_batch(st, c->mode, c->dp_aux, r.xb, (uint64_t)n * 4 * kb, kb, 0, false));
    HIP_TRY(launch_ctm_tensor_rowsum(st, c->dp, k, N, r.xq, r.yq, dim, nq, j0, nj, splits));
    HIP_TRY(launch_ctm_tensor_rowsum(st, c->dp_aux, kb, N, r.xb, r.yb, dim, nq, j0, nj, splits));
  }
  if (fin) {
    HIP_TRY(c->ops->ntt_batch(st, c->mode, c->dp, r.yq, (uint64_t)fin * nq * 3 * k, k, 0, true));
    HIP_TRY(c->ops->ntt_batch(st, c->mode, c->dp_aux, r.yb, (uint64_t)fin * nq * 3 * kb, kb, 0, true));
    HIP_TRY(launch_ctm_scale(st, c->d_ctm, k, N, r.yq, r.yb, r.d, fin * nq));
  }
  return fin;
}
// After a block that finished `fin` rows and ended inside the next one: that row's accumulators to the front.
void ctm_carry_row(pirgpu_ctx* c, hipStream_t st, const CtmRegions& r, uint32_t nq, uint32_t fin) {
  const size_t wq = (size_t)nq * 3 * c->k * c->N, wb = (size_t)nq * 3 * c->kb * c->N;
  if (!fin) return;
  HIP_TRY(hipMemcpyAsync(r.yq, r.yq + fin * wq, wq * 8, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(r.yb, r.yb + fin * wb, wb * 8, hipMemcpyDeviceToDevice, st));
}

// The CtmSel of a hook call (pirgpu_ct_multiply, pirgpu_ct_multiply_sum on a CT_SHARED_SEL context): the n selectors b
// [n][2][k][N], coefficient form, as one query's array of dim = n.  At B their centred lifts, transformed, into selb
// [n][2][kb][N]; at Q the forward transform of a copy in selq [n][2][k][N] -- canonical residues in the order ntt_batch
// emits, which is what the query path reads from the selection vector.  Both buffers are the call's own.
CtmSel ctm_hook_selectors(pirgpu_ctx* c, hipStream_t st, const uint64_t* b, uint64_t n, uint64_t* selq, uint64_t* selb) {
  const uint32_t N = c->N, k = c->k, kb = c->kb;
  for (uint64_t s0 = 0; s0 < n; s0 += 32767)   // (the launch takes 32 767 ciphertexts)
    HIP_TRY(launch_ctm_lift_polys(st, c->d_ctm, k, N, b + (size_t)s0 * c->ctw, 0, 1, 0, (uint32_t)std::min<uint64_t>(32767, n - s0),
                                  nullptr, selb + (size_t)s0 * 2 * kb * N));
  HIP_TRY(c->ops->ntt_batch(st, c->mode, c->dp_aux, selb, n * 2 * kb, kb, 0, false));
  HIP_TRY(hipMemcpyAsync(selq, b, (size_t)n * c->ctw * 8, hipMemcpyDeviceToDevice, st));
  HIP_TRY(c->ops->ntt_batch(st, c->mode, c->dp, selq, n * 2 * k, k, 0, false));
  c->options.counter(OPT_CT_LIFTS) += 2 * n;
  CtmSel sel{};
  sel.q.p[0] = selq;
  sel.b.p[0] = selb;
  return sel;
}

// The relinearisation key of every query of a group: stored as the key of Galois element 1 of its key set (expansion
// never uses element 1; the wire codec maps RelinKeys index 0 the same way).
KeyPtrs relin_keys_for(pirgpu_ctx* c, const uint32_t* ksets, uint32_t nq) {
  for (uint32_t q = 0; q < nq; ++q) {
    const uint32_t slot = ksets[q];
    if (slot >= c->keysets.size() || !c->keysets[slot].keys.count(1))
      throw Fail{PIRGPU_INVALID_ARGUMENT, "RelinKeys missing: ciphertext multiplication at d >= 2 needs the client's "
                                          "relinearisation key (installed as the key of Galois element 1)"};
  }
  return keys_for(c, 1, ksets, nq);
}

// r.d [n][d0, d2, d1] -> r.yq [n][2][k][N] = (d0 + KS0(d2), KS1(d2)), canonical: the key-switch launches of one
// expansion level with Galois element 1 (the identity) and without the tree step; pair p is switched with key.p[p % B].
void ctm_relinearize(pirgpu_ctx* c, hipStream_t st, const CtmRegions& r, uint32_t n, const KeyPtrs& key) {
  const uint32_t N = c->N, k = c->k;
  const uint64_t pw = (uint64_t)k * N;
  HIP_TRY(launch_tree_convert(st, c->dp, c->mode, r.d, r.xq, (uint64_t)n * 2 * pw, true, 2 * pw, 3 * pw));
  HIP_TRY(c->ops->ks_digit(st, c->mode, c->dp, k, r.xq, 1, n, r.dig, c->pack40, nullptr, false, false));
  HIP_TRY(c->ops->ks_mac_intt(st, c->mode, c->dp, k, r.dig, key, n, r.prod, c->pack40, 0, k + 1));
  HIP_TRY(launch_ks_combine(st, c->dp, c->mode, N, k, r.xq, r.prod, 1, n, 0, false, 0, c->pack40, r.yq, c->pack_bytes));
  if (c->mode != kNttInt) HIP_TRY(launch_tree_convert(st, c->dp, c->mode, r.yq, r.yq, (uint64_t)n * 2 * pw, false));
}

// One upper level in ciphertext-multiplication mode (reference database.cpp:196-212,238-254):
// lvl[l][row] = sum over the children i that exist of relin(mul(lvl[l + 1][row * dims[l] + i], sel_l[i])).
void post_scan_ctm_level(pirgpu_ctx* c, const Stage& sg, uint32_t l) {
  const uint32_t N = c->N, k = c->k, nq = sg.n, dim = c->dims[l];
  const size_t ctw = c->ctw;
  // PIRGPU_CREATE_CT_COMPACT_REPLY: level 0 at k primes lands in the owner's `last` buffer (same stride), the carry of a
  // row's sum from block to block included; post_scan_stage switches and packs it from there
  uint64_t* const out = c->pack && l == 0 ? sg.last : sg.lvl[l];
  const uint64_t nch = c->lvl_rows[l + 1], rows = c->lvl_rows[l];
  hipStream_t st = sg.stream;
  if (nq > (uint32_t)kMaxMfmaQueries || sg.local_rows || sg.sel_f64) throw Fail{PIRGPU_INTERNAL, "unexpected stage in ciphertext-multiplication mode"};
  const KeyPtrs key = relin_keys_for(c, sg.ksets, nq);
  CtmScratch& ws = ctm_scratch(c, st);
  const uint32_t cap = ctm_cap_pairs(c);
  const CtmRegions r = ctm_regions(c, ws.buf, cap);
  // the level's selectors back in coefficient form (canonical residues), query-major
  if ((size_t)nq * dim * ctw > ws.selc_words) throw Fail{PIRGPU_INTERNAL, "selector scratch undersized"};
  for (uint32_t q = 0; q < nq; ++q)
    HIP_TRY(hipMemcpyAsync(ws.selc + (size_t)q * dim * ctw, static_cast<const uint64_t*>(sg.sel.p[q]) + (size_t)c->sv_off[l] * ctw,
                           (size_t)dim * ctw * 8, hipMemcpyDeviceToDevice, st));
  HIP_TRY(c->ops->ntt_batch(st, c->mode, c->dp, ws.selc, (uint64_t)nq * dim * 2 * k, k, 0, true));
  // shared selectors: their lifts to B, transformed, once for all rows (and planes) of the level; at Q the selection
  // vector itself is read
  const bool shared = c->ctm_shared_sel;
  CtmSel sel{};
  if (shared) {
    if (!ws.selb) throw Fail{PIRGPU_INTERNAL, "shared-selector scratch missing"};
    for (uint32_t s0 = 0; s0 < nq * dim; s0 += 32767)   // (the launch takes 32 767 ciphertexts)
      HIP_TRY(launch_ctm_lift_polys(st, c->d_ctm, k, N, ws.selc + (size_t)s0 * ctw, 0, 1, 0, std::min<uint32_t>(32767, nq * dim - s0),
                                    nullptr, ws.selb + (size_t)s0 * 2 * c->kb * N));
    HIP_TRY(c->ops->ntt_batch(st, c->mode, c->dp_aux, ws.selb, (uint64_t)nq * dim * 2 * c->kb, c->kb, 0, false));
    c->options.counter(OPT_CT_LIFTS) += (uint64_t)2 * dim * nq;
    for (uint32_t q = 0; q < nq; ++q) {
      sel.q.p[q] = static_cast<const uint64_t*>(sg.sel.p[q]) + (size_t)c->sv_off[l] * ctw;
      sel.b.p[q] = ws.selb + (size_t)q * dim * 2 * c->kb * N;
    }
  }
  const uint32_t bj = std::max<uint32_t>(1, cap / nq);   // children per block (of every query of the group)
  for (uint64_t j0 = 0; j0 < nch; j0 += bj) {
    const uint32_t nj = (uint32_t)std::min<uint64_t>(bj, nch - j0), n = nj * nq;
    ++c->options.counter(OPT_CT_BLOCKS);
    c->options.counter(OPT_CT_LIFTS) += (uint64_t)(shared ? 2 : 4) * n;
    if (c->ctm_deferred) {
      const uint32_t fin = ctm_rowsum_block(c, st, r, cap, sg.lvl[l + 1], c->lvl_cts[l + 1] * ctw, ws.selc, dim, nq, nch,
                                            (uint32_t)j0, nj, shared ? &sel : nullptr);
      if (!fin) continue;
      c->options.counter(OPT_CT_RELINS) += (uint64_t)fin * nq;
      ctm_relinearize(c, st, r, fin * nq, key);
      // relin + (0, d1) into the finished rows: the accumulation with one child per row (pirgpu_relinearize's form)
      HIP_TRY(launch_ctm_accumulate(st, c->dp, k, N, r.yq, r.d, out + (size_t)(j0 / dim) * ctw, c->lvl_cts[l] * ctw, 1,
                                    nq, 0, fin, fin));
      if ((j0 + nj) % dim != 0 && j0 + nj < nch) ctm_carry_row(c, st, r, nq, fin);
      continue;
    }
    c->options.counter(OPT_CT_RELINS) += n;
    if (shared)
      ctm_products_sel(c, st, r, sg.lvl[l + 1], c->lvl_cts[l + 1] * ctw, sel, dim, nq, (uint32_t)j0, n);
    else
      ctm_products(c, st, r, sg.lvl[l + 1], c->lvl_cts[l + 1] * ctw, ws.selc, dim, nq, (uint32_t)j0, n);
    ctm_relinearize(c, st, r, n, key);
    HIP_TRY(launch_ctm_accumulate(st, c->dp, k, N, r.yq, r.d, out, c->lvl_cts[l] * ctw, dim, nq, (uint32_t)j0, nj,
                                  (uint32_t)rows));
  }
}

// Everything after the scan: inverse NTT of the row sums and the upper recursion levels
// (reference database.cpp:196-254).  Leaves the reply in lvl[0].
void post_scan_stage(pirgpu_ctx* c, const Stage& sg, Worker* profiled) {
  const uint32_t N = c->N, k = c->k, d = c->d;
  const size_t ctw = c->ctw;
  const uint64_t shard_pts = matrix_pts(c);
  hipStream_t st = sg.stream;
  if ((c->rp || c->pack) && !sg.last) throw Fail{PIRGPU_INTERNAL, "result_primes / packed replies without a level-0 buffer"};
  // level l's result at k primes: lvl[l], or -- result_primes or packed replies, level 0 -- the owner's `last` buffer,
  // from where the compact switch (or the pack kernel) writes the reply to lvl[0]
  auto level = [&](uint32_t l) { return (c->rp || c->pack) && l == 0 ? sg.last : sg.lvl[l]; };
  // result_primes: every level result is switched right after its inverse transform (all flavours leave canonical u64
  // residues there: Encode reads them as such) -- in place below the reply, compact for the reply itself
  // (ciphertext-multiplication mode: the product is defined over Q, so only the finished level 0 is switched)
  auto switch_level = [&](uint32_t l) {
    if (!c->rp || (c->ctm && l != 0)) return;
    const uint64_t qstride = c->lvl_cts[l] * ctw;
    if (l == 0 && !c->pack)
      HIP_TRY(launch_mod_switch(st, c->dp, sg.last, sg.lvl[0], c->lvl_cts[0], k, c->rp, N, true, sg.n, qstride,
                                c->reply_cts * c->rctw));
    else if (l == 0)   // packed replies: switched where it lies (stride k kept); the pack kernel reads the first rp residues
      HIP_TRY(launch_mod_switch(st, c->dp, sg.last, sg.last, c->lvl_cts[0], k, c->rp, N, false, sg.n, qstride, qstride));
    else
      HIP_TRY(launch_mod_switch(st, c->dp, sg.lvl[l], sg.lvl[l], c->lvl_cts[l], k, c->rp, N, false, sg.n, qstride, qstride));
  };
  if (shard_pts == 0) {
    HIP_TRY(hipMemsetAsync(sg.lvl[0], 0, (size_t)sg.n * c->reply_cts * c->rctw * 8, st));
    return;
  }
  if (profiled) record(c, *profiled, PH_UPPER);  // end of scan phase
  if (!sg.rows_inverted)
    HIP_TRY(c->ops->ntt_batch(st, c->mode, c->dp, level(d - 1), (uint64_t)sg.n * c->scan_rows * 2 * k, k, 0, true));
  switch_level(d - 1);
  // upper levels: fused re-encode + lift + NTT + multiply-accumulate over chunks of children,
  // then one kernel folds the chunk sums and applies the inverse NTT
  uint64_t C = 1;  // ciphertexts per child
  for (int l = (int)d - 2; l >= 0; --l) {
    if (c->ctm) {   // ciphertext by ciphertext: one result ciphertext per node at every level, nothing re-encoded
      if (l == 0 && profiled) record(c, *profiled, PH_FINAL);
      post_scan_ctm_level(c, sg, (uint32_t)l);
      switch_level((uint32_t)l);
      continue;
    }
    const uint64_t nch = ceil_div(shard_pts, c->stride[l + 1]);
    const uint64_t rows = c->lvl_rows[l];
    // dimension-0 selectors: the query's whole selection vector at index sv_off[0] + shard_begin + i, or (packed
    // multi-GPU exchange) a buffer holding just this shard's rows at local index i
    const bool local_rows = l == 0 && sg.local_rows;
    const uint32_t sv_first = local_rows ? 0 : c->sv_off[l] + (l == 0 ? c->sb : 0);
    // enough workgroups to fill the chip: ~1024 over (queries * rows * C * chunks * E * k)
    const uint64_t per_chunk = rows * C * c->E * k;
    const uint32_t target = sg.n > 1 || c->in_batch ? c->upper_blocks_batch : c->upper_blocks;
    // children one output row actually has in this shard: dims[l], or -- at the top level of a row shard -- only the
    // shard's rows (a 20-row shard of 162 used to leave three of its four chunks empty; wide items have planes rows at
    // the top level, each with all dims[0] children: they are never row-sharded)
    const uint64_t kids = rows == 1 ? std::min<uint64_t>(c->dims[l], std::max<uint64_t>(nch, 1)) : c->dims[l];
    uint32_t n_chunks = (uint32_t)std::min<uint64_t>(kids, std::max<uint64_t>(1, ceil_div(target, per_chunk)));
    const uint32_t chunk_len = (uint32_t)ceil_div(kids, n_chunks);
    n_chunks = (uint32_t)ceil_div(kids, chunk_len);
    const uint64_t out_polys = rows * C * c->E * 2 * k;
    if (out_polys * n_chunks * N > c->pt_words)
      throw Fail{PIRGPU_INTERNAL, "upper-level scratch undersized"};
    if (local_rows && l != 0) throw Fail{PIRGPU_INTERNAL, "local row selectors are a d = 2 feature"};
    if (c->split_upper && sg.up_scratch) {
      // large rings: transform the re-encoded plaintexts of a block of children into scratch, multiply-accumulate
      // them elementwise, next block (upper_ntt_kernel / upper_mac_kernel)
      const uint64_t unit = (uint64_t)sg.n * rows * C * c->E * k * N;   // scratch words per child of the block
      // children per output row that exist in this shard: at the top level of a row shard only its own rows (the
      // selector buffer of the packed multi-GPU exchange holds no more than those -- reading on to dims[l] ran past it)
      const uint32_t nd = (uint32_t)kids;
      uint32_t blk = (uint32_t)std::min<uint64_t>(nd, std::max<uint64_t>(1, c->split_upper_words / unit));
      if (*sg.up_scratch_words < unit * blk) {
        HIP_TRY(hipStreamSynchronize(st));
        if (*sg.up_scratch) {
          auto it = std::find(c->allocs.begin(), c->allocs.end(), (void*)*sg.up_scratch);
          if (it != c->allocs.end()) c->allocs.erase(it);
          HIP_TRY(hipFree(*sg.up_scratch));
          *sg.up_scratch = nullptr;
        }
        *sg.up_scratch = c->dalloc<uint64_t>(unit * blk);
        *sg.up_scratch_words = unit * blk;
      }
      for (uint32_t b0 = 0; b0 < nd; b0 += blk) {
        ++c->options.counter(OPT_UPPER_PARTS);
        HIP_TRY(c->ops->upper_ntt(st, c->mode, c->dp, k, c->E, sg.lvl[l + 1], *sg.up_scratch, (uint32_t)rows, c->dims[l],
                                  (uint32_t)nch, (uint32_t)C, b0, blk, sg.n, c->lvl_cts[l + 1] * ctw, c->loop_transforms));
        if (c->mode == kNttInt)   // N = 32768
          HIP_TRY(launch_upper_mac_int(st, c->dp, *sg.up_scratch, sg.sel, sg.pt_buf, level(l), sg.n, (uint32_t)rows,
                                       (uint32_t)C, c->E, k, N, sv_first, b0, blk, nd, b0 == 0, b0 + blk >= nd, c->pt_words,
                                       c->lvl_cts[l] * ctw));
        else
          HIP_TRY(launch_upper_mac(st, c->dp, *sg.up_scratch, sg.sel, sg.pt_buf, level(l), sg.n, (uint32_t)rows, (uint32_t)C,
                                   c->E, k, N, sv_first, b0, blk, nd, b0 == 0, b0 + blk >= nd, c->pt_words,
                                   c->lvl_cts[l] * ctw));
      }
      if (l == 0 && profiled) record(c, *profiled, PH_FINAL);
    } else {
      c->options.counter(OPT_UPPER_PARTS) += n_chunks;
      HIP_TRY(c->ops->upper_fused(st, c->mode, c->dp, k, c->E, sg.lvl[l + 1], sg.sel, sg.pt_buf, (uint32_t)rows,
                                  c->dims[l], (uint32_t)nch, sv_first, (uint32_t)C, chunk_len, n_chunks, sg.n,
                                  c->lvl_cts[l + 1] * ctw, c->pt_words, sg.sel_f64));
      if (l == 0 && profiled) record(c, *profiled, PH_FINAL);
      // fold the chunk sums (wide, elementwise) and return to coefficient form (database.cpp:250-254)
      HIP_TRY(launch_reduce_splits(st, c->dp, sg.pt_buf, n_chunks, out_polys * N, level(l), sg.n, c->pt_words,
                                   c->lvl_cts[l] * ctw));
    }
    HIP_TRY(c->ops->ntt_batch(st, c->mode, c->dp, level(l), (uint64_t)sg.n * out_polys, k, 0, true));
    switch_level(l);
    C *= c->E;
  }
  if (d == 1 && profiled) record(c, *profiled, PH_FINAL);
  // packed replies: once per query or group, on the stream that produced level 0, to where the reply went before
  if (c->pack)
    HIP_TRY(launch_reply_pack(st, c->rpa, sg.last, sg.lvl[0], c->lvl_cts[0], sg.n, c->lvl_cts[0] * ctw, c->reply_cts * c->rctw));
}

// Everything after the scan for one worker's query: inverse NTT of the row sums and the upper recursion levels
// (reference database.cpp:196-254).  Leaves the reply in lvl[0].
void post_scan_on_device(pirgpu_ctx* c, Worker& w) {
  Stage sg{w.stream, w.lvl.data(), w.pt_buf, 1, MfmaPtrs{}, w.sv_rows != nullptr, &w.up_scratch, &w.up_scratch_words};
  sg.sel.p[0] = w.sv_rows ? w.sv_rows : (w.sv_cur ? w.sv_cur : w.sv_ntt);
  sg.last = w.last;
  sg.ksets[0] = w.keyset;
  post_scan_stage(c, sg, &w);
}

void multiply_on_device(pirgpu_ctx* c, Worker& w) {
  scan_on_device(c, w);
  post_scan_on_device(c, w);
}

void run_staged(pirgpu_ctx* c, Worker& w, bool profile) {
  ensure_workspace(c);
  if (w.staged_nq != c->dim_sum / c->N + 1)
    throw Fail{PIRGPU_INVALID_ARGUMENT,
               "Number of ciphertexts doesn't match number of items for oblivious expansion."};
  c->prof_cur = -1;
  w.keyset = current_keyset(c);
  w.table = c->cur_table;
  if (c->ctm && c->d >= 2) (void)relin_keys_for(c, &w.keyset, 1);   // before anything is queued
  // a batch group that borrowed this worker's selection vector (its multiply runs on a lane stream) must be done
  HIP_TRY(hipStreamWaitEvent(w.stream, w.ev_done, 0));
  if (profile) begin_profiled_run(c);
  record(c, w, PH_EXPAND);
  // expansion and selection-vector NTT are interleaved per query ciphertext; the
  // PH_SVNTT mark is taken after the last expansion level of the last ciphertext.
  expand_query_to_sv(c, w, w.d_query, w.staged_nq);
  record(c, w, PH_SVNTT);
  record(c, w, PH_SCAN);
  multiply_on_device(c, w);
  record(c, w, PH_COUNT);
  c->prof_cur = -1;
  w.reply_valid = true;
  // a batch group that borrows this worker's selection vector next (on a lane's stream, possibly queued by another
  // thread before this query has been fetched) waits for this point
  HIP_TRY(hipEventRecord(w.ev_done, w.stream));
}

}  // namespace

// =============================================================================
// C ABI
// =============================================================================

extern "C" {

// ======================================================================================================================
// [5] C ABI: create / destroy, options, database loading
// ======================================================================================================================
const char* pirgpu_create_error(void) { return g_create_error.c_str(); }

int pirgpu_create(const pirgpu_params* p, pirgpu_ctx** out) { return pirgpu_create_ex(p, 0, out); }

int pirgpu_create_ex(const pirgpu_params* p, uint32_t flags, pirgpu_ctx** out) {
  if (!p || !out) return PIRGPU_INVALID_ARGUMENT;
  *out = nullptr;
  pirgpu_ctx* c = new pirgpu_ctx();
  c->gen = ++g_ctx_generation;
  auto bail = [&](int code, const std::string& msg) {
    g_create_error = msg;
    pirgpu_destroy(c);
    return code;
  };
  try {
    if (flags & ~(PIRGPU_CREATE_STREAMED_DB | PIRGPU_CREATE_CT_MULTIPLY | PIRGPU_CREATE_CT_DEFERRED | PIRGPU_CREATE_PACKED_REPLIES |
                  PIRGPU_CREATE_CT_COMPACT_REPLY))
      return bail(PIRGPU_INVALID_ARGUMENT, "unknown pirgpu_create_ex flags " + std::to_string(flags));
    c->streamed = (flags & PIRGPU_CREATE_STREAMED_DB) != 0;
    c->ctm = (flags & PIRGPU_CREATE_CT_MULTIPLY) != 0;
    c->ctm_deferred = (flags & PIRGPU_CREATE_CT_DEFERRED) != 0;
    c->pack = (flags & PIRGPU_CREATE_PACKED_REPLIES) != 0;
    if (c->pack && c->ctm)
      return bail(PIRGPU_INVALID_ARGUMENT, "PIRGPU_CREATE_PACKED_REPLIES with PIRGPU_CREATE_CT_MULTIPLY is not supported");
    if (c->pack && (p->shard_begin || p->shard_end))
      return bail(PIRGPU_INVALID_ARGUMENT, "PIRGPU_CREATE_PACKED_REPLIES is served by one GPU: a row shard (shard_begin / "
                                           "shard_end) is not supported (packed words do not sum over shards)");
    if (c->pack && (p->slot_begin || p->slot_end))
      return bail(PIRGPU_INVALID_ARGUMENT, "PIRGPU_CREATE_PACKED_REPLIES is served by one GPU: a slot shard (slot_begin / "
                                           "slot_end) is not supported");
    if (c->ctm_deferred && !c->ctm)
      return bail(PIRGPU_INVALID_ARGUMENT, "PIRGPU_CREATE_CT_DEFERRED needs PIRGPU_CREATE_CT_MULTIPLY (it is a form of that mode)");
    // PIRGPU_CREATE_CT_COMPACT_REPLY: the finished reply of a ciphertext-multiplication context is
    // switched to result_primes primes and packed; PIRGPU_CREATE_PACKED_REPLIES itself stays refused there (above)
    c->ctm_compact = (flags & PIRGPU_CREATE_CT_COMPACT_REPLY) != 0;
    if (c->ctm_compact && !c->ctm)
      return bail(PIRGPU_INVALID_ARGUMENT, "PIRGPU_CREATE_CT_COMPACT_REPLY needs PIRGPU_CREATE_CT_MULTIPLY (it is a form of that mode)");
    if (c->ctm_compact) c->pack = true;
    c->prm = *p;
    const uint32_t N = p->poly_modulus_degree, k = p->num_data_primes;
    if (N < 2048 || N > 32768 || (N & (N - 1)))
      return bail(PIRGPU_INVALID_ARGUMENT, "poly_modulus_degree must be 2048, 4096, 8192, 16384 or 32768");
    if (k < 1 || k > PIRGPU_MAX_PRIMES) return bail(PIRGPU_INVALID_ARGUMENT, "invalid number of data primes");
    if (p->use_ciphertext_multiplication && !c->ctm)
      return bail(PIRGPU_UNIMPLEMENTED,
                  "use_ciphertext_multiplication is not supported by the MI355X path (decomposition mode only) unless the "
                  "context is created with pirgpu_create_ex and PIRGPU_CREATE_CT_MULTIPLY");
    if (c->ctm) {
      // the mode is opt-in twice: the reference's field says what the client expects, the flag that the caller accepts
      // this project's exact product (not SEAL's BEHZ approximation)
      if (!p->use_ciphertext_multiplication)
        return bail(PIRGPU_INVALID_ARGUMENT, "PIRGPU_CREATE_CT_MULTIPLY needs use_ciphertext_multiplication = 1 in the parameters");
      if (c->streamed)
        return bail(PIRGPU_INVALID_ARGUMENT, "PIRGPU_CREATE_CT_MULTIPLY with PIRGPU_CREATE_STREAMED_DB is not supported");
      if (N == 32768)
        return bail(PIRGPU_INVALID_ARGUMENT, "PIRGPU_CREATE_CT_MULTIPLY is not supported at poly_modulus_degree 32768");
      if (k > (uint32_t)kCtmMaxQ)
        return bail(PIRGPU_INVALID_ARGUMENT, "PIRGPU_CREATE_CT_MULTIPLY serves at most 6 data primes (num_data_primes; the "
                                             "auxiliary base of k + 2 primes must fit 8)");
      if (p->shard_begin || p->shard_end)
        return bail(PIRGPU_INVALID_ARGUMENT, "PIRGPU_CREATE_CT_MULTIPLY is served by one GPU: a row shard (shard_begin / "
                                             "shard_end) is not supported");
      if (p->slot_begin || p->slot_end)
        return bail(PIRGPU_INVALID_ARGUMENT, "PIRGPU_CREATE_CT_MULTIPLY is served by one GPU: a slot shard (slot_begin / "
                                             "slot_end) is not supported");
      if (p->result_primes && !c->ctm_compact)
        return bail(PIRGPU_INVALID_ARGUMENT, "PIRGPU_CREATE_CT_MULTIPLY with result_primes > 0 is not supported (without "
                                             "PIRGPU_CREATE_CT_COMPACT_REPLY)");
      if (p->tables > 1) return bail(PIRGPU_INVALID_ARGUMENT, "PIRGPU_CREATE_CT_MULTIPLY with tables > 1 is not supported");
    }
    if (p->special_prime == 0)
      return bail(PIRGPU_INVALID_ARGUMENT, "a key-switching special prime is required (SEAL: keyswitching unsupported)");
    for (uint32_t i = 0; i <= k; ++i) {
      uint64_t q = i < k ? p->coeff_modulus[i] : p->special_prime;
      if (q >> 61 || q < 2 || !hm::is_prime(q) || (q - 1) % (2ull * N))
        return bail(PIRGPU_INVALID_ARGUMENT, "coeff modulus must be a prime < 2^61 congruent to 1 mod 2N");
      for (uint32_t j = 0; j < i; ++j)
        if (p->coeff_modulus[j] == q) return bail(PIRGPU_INVALID_ARGUMENT, "coeff moduli must be distinct");
    }
    if (p->plain_modulus < 2 || p->plain_modulus >> 60)
      return bail(PIRGPU_INVALID_ARGUMENT, "invalid plain modulus");
    if (p->num_dimensions < 1 || p->num_dimensions > PIRGPU_MAX_DIMS)
      return bail(PIRGPU_INVALID_ARGUMENT, "invalid number of dimensions");
    if (c->streamed && p->num_dimensions == 1)
      return bail(PIRGPU_INVALID_ARGUMENT, "a streamed database needs d >= 2: the d = 1 scans read the u64 staging copy");
    c->N = N;
    c->k = k;
    while ((1u << c->logN) < N) ++c->logN;
    c->ctw = (size_t)2 * k * N;
    c->d = p->num_dimensions;
    c->P = p->num_pt;
    uint64_t ds = 0;
    for (uint32_t l = 0; l < c->d; ++l) {
      c->dims[l] = p->dimensions[l];
      if (c->dims[l] == 0) return bail(PIRGPU_INVALID_ARGUMENT, "dimension of size 0");
      c->sv_off[l] = (uint32_t)ds;
      ds += c->dims[l];
    }
    c->sv_off[c->d] = (uint32_t)ds;
    if (ds > (1ull << 24)) return bail(PIRGPU_INVALID_ARGUMENT, "dimension sum too large");
    c->dim_sum = (uint32_t)ds;
    c->stride[c->d] = 1;
    for (int l = (int)c->d - 1; l >= 0; --l) c->stride[l] = c->stride[l + 1] * c->dims[l];
    c->sb = p->shard_begin;
    c->se = p->shard_end;
    if (c->sb == 0 && c->se == 0) c->se = c->dims[0];
    if (c->sb > c->se || c->se > c->dims[0]) return bail(PIRGPU_INVALID_ARGUMENT, "invalid shard range");
    {
      const uint32_t kN = k * N;
      c->slot0 = p->slot_begin;
      c->nslots = (p->slot_begin == 0 && p->slot_end == 0) ? kN : p->slot_end - p->slot_begin;
      if (p->slot_end > kN || (p->slot_end && p->slot_end <= p->slot_begin) || c->slot0 % 16 || c->nslots % 16)
        return bail(PIRGPU_INVALID_ARGUMENT, "invalid slot range (multiples of 16 inside [0, k N))");
      c->slot_sharded = c->nslots != kN;
      if (c->slot_sharded && (c->d != 2 || c->sb != 0 || c->se != c->dims[0]))
        return bail(PIRGPU_INVALID_ARGUMENT, "a slot shard needs d = 2 and all rows (no row shard)");
    }
    c->pt_begin = std::min<uint64_t>((uint64_t)c->sb * c->stride[1], c->P);
    c->pt_end = std::min<uint64_t>((uint64_t)c->se * c->stride[1], c->P);
    const uint32_t bdef = hm::bits_per_coeff(p->plain_modulus);
    if (p->bits_per_coeff > bdef) return bail(PIRGPU_INVALID_ARGUMENT, "Bits per coefficient greater than max");
    c->bits = p->bits_per_coeff ? p->bits_per_coeff : bdef;
    c->planes = std::max<uint32_t>(1, p->plaintexts_per_item);
    if (c->planes > 1) {
      const uint64_t B = (uint64_t)N * c->bits / 8;   // StringEncoder::max_bytes_per_plaintext (string_encoder.cpp:29-31)
      if (p->items_per_plaintext != 1)
        return bail(PIRGPU_INVALID_ARGUMENT, "plaintexts_per_item > 1 needs items_per_plaintext == 1");
      if (p->bytes_per_item <= (c->planes - 1) * B || p->bytes_per_item > c->planes * B)
        return bail(PIRGPU_INVALID_ARGUMENT, "bytes_per_item " + std::to_string(p->bytes_per_item) + " does not need exactly " +
                                                 "plaintexts_per_item = " + std::to_string(c->planes) + " plaintexts of " +
                                                 std::to_string(B) + " bytes");
      if (c->sb != 0 || c->se != c->dims[0] || c->slot_sharded)
        return bail(PIRGPU_INVALID_ARGUMENT, "wide items (plaintexts_per_item > 1) are served by one GPU: row and slot "
                                             "shards of them are not supported");
      if (c->P > c->stride[0] || c->P == 0 || c->planes > 4096)
        return bail(PIRGPU_INVALID_ARGUMENT, "plaintexts_per_item > 1 needs 0 < num_pt <= the product of the dimensions");
      c->plane_pad = c->stride[0];
    }
    c->tables = std::max<uint32_t>(1, p->tables);
    if (c->tables > 1) {
      // one GPU, one plaintext per item at the most, a staging copy to pack every table from
      if (c->sb != 0 || c->se != c->dims[0])
        return bail(PIRGPU_INVALID_ARGUMENT, "tables > 1 is served by one GPU: a row shard (shard_begin / shard_end) of a "
                                             "context with tables is not supported");
      if (c->slot_sharded)
        return bail(PIRGPU_INVALID_ARGUMENT, "tables > 1 is served by one GPU: a slot shard (slot_begin / slot_end) of a "
                                             "context with tables is not supported");
      if (c->planes > 1)
        return bail(PIRGPU_INVALID_ARGUMENT, "tables > 1 with plaintexts_per_item > 1 is not supported (a table and a plane "
                                             "both claim the outermost rows of the stored database)");
      if (c->streamed)
        return bail(PIRGPU_INVALID_ARGUMENT, "tables > 1 with PIRGPU_CREATE_STREAMED_DB is not supported: every table is "
                                             "packed from the staging copy");
      if (c->P == 0) return bail(PIRGPU_INVALID_ARGUMENT, "tables > 1 needs num_pt > 0");
      const uint64_t cols = c->dims[c->d - 1];
      c->table_pad = c->d == 1 ? c->P : ceil_div(c->P, cols) * cols;
      // the table-major plaintext index tables * num_pt and the rows of the staging copy stay inside the 32-bit range the
      // row / unit bookkeeping of loads and updates uses
      if ((uint64_t)c->tables * c->table_pad >= (1ull << 32))
        return bail(PIRGPU_INVALID_ARGUMENT, "tables x num_pt does not fit the plaintext index range (2^32)");
      c->tbl_loaded.assign(c->tables, 0);
      c->tbl_zero.assign(c->tables, 0);
      c->tbl_packed.assign(c->tables, 0);
    }
    c->rp = p->result_primes;
    if (c->rp >= k)
      return bail(PIRGPU_INVALID_ARGUMENT, "result_primes must be below num_data_primes (0 = keep every result at the full modulus)");
    if (c->rp && (c->sb != 0 || c->se != c->dims[0] || c->slot_sharded))
      return bail(PIRGPU_INVALID_ARGUMENT, "result_primes > 0 is served by one GPU: modulus switching does not commute with "
                                           "the sum over row or slot shards");
    c->rctw = c->rp ? (size_t)2 * c->rp * N : c->ctw;
    if (c->pack) {
      c->rpa = reply_pack_args(N, p->coeff_modulus, c->rp ? c->rp : k, k);
      c->rctw = c->rpa.ct_words;
    }
    c->device = p->device;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
      return bail(PIRGPU_INTERNAL, "no HIP device available (libpirgpu has no CPU fallback)");
    if (c->device < 0 || c->device >= ndev) return bail(PIRGPU_INVALID_ARGUMENT, "invalid device ordinal");
    c->use_device();
    HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->ops = ntt_ops_for(N);
    if (!c->ops) return bail(PIRGPU_INVALID_ARGUMENT, "poly_modulus_degree must be 2048, 4096, 8192, 16384 or 32768");
    if (c->ctm) {
      // the auxiliary base and its bound, in integers, before anything is allocated for it
      if (const char* why = ctm::plan(N, k, p->coeff_modulus, p->special_prime, p->plain_modulus, c->aux_primes))
        return bail(PIRGPU_INVALID_ARGUMENT, why);
      if (c->ctm_deferred) {   // a row's sum has up to dims[l] terms
        uint64_t terms = 1;
        for (uint32_t l = 0; l + 1 < c->d; ++l) terms = std::max<uint64_t>(terms, c->dims[l]);
        if (const char* why = ctm::plan(N, k, p->coeff_modulus, p->special_prime, p->plain_modulus, c->aux_primes, terms))
          return bail(PIRGPU_INVALID_ARGUMENT, std::string("PIRGPU_CREATE_CT_DEFERRED: ") + why);
      }
      c->kb = k + 2;
    }
    build_tables(c);
    HIP_TRY(c->ops->configure(c->mode));
    if (c->ctm) {
      build_ctm_tables(c);
      c->E = 1;   // every level result is ONE ciphertext per node: nothing is re-encoded (er keeps ExpansionRatio)
    }
    c->reply_cts = c->planes;   // every plane answers with its own (2 ExpansionRatio)^(d-1) ciphertexts
    for (uint32_t l = 1; l < c->d; ++l) c->reply_cts *= c->E;
    const uint64_t shard_pts = c->pt_end - c->pt_begin;
    // rows are padded with zero plaintexts to full length so the scan kernels are branch-free
    const uint64_t cols_last = c->dims[c->d - 1];
    const uint64_t padded = c->tables > 1   ? c->tables * c->table_pad
                            : c->planes > 1 ? matrix_pts(c)
                            : c->d == 1     ? shard_pts
                                            : ceil_div(shard_pts, cols_last) * cols_last;
    if (!c->streamed) {
      c->d_db = c->dalloc<uint64_t>(padded * k * N);
      c->db_bytes = std::max<uint64_t>(padded * k * N, 1) * 8;
      note_mem(c);
      if (c->planes > 1 || c->tables > 1)   // every plane is padded to the whole box of its dimensions, every table to whole rows
        HIP_TRY(hipMemset(c->d_db, 0, padded * k * N * 8));
      else if (padded > shard_pts)
        HIP_TRY(hipMemset(c->d_db + shard_pts * k * N, 0, (padded - shard_pts) * k * N * 8));
    }
    c->loaded.assign(held_pts(c), 0);   // per ABI plaintext index - pt_begin (plane-major)
  } catch (const Fail& e) {
    return bail(e.code, e.msg);
  } catch (const std::exception& e) {
    return bail(PIRGPU_INTERNAL, e.what());
  }
  *out = c;
  return PIRGPU_OK;
}

void pirgpu_destroy(pirgpu_ctx* c) {
  if (!c) return;
  pirgpu_wire_forget(c);
  if (c->stream) {
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (BatchLane& ln : c->lanes)
      if (ln.stream) (void)hipStreamSynchronize(ln.stream);
    for (size_t i = 1; i < c->workers.size(); ++i)
      if (c->workers[i].stream) (void)hipStreamSynchronize(c->workers[i].stream);
  }
  for (KeySet& ks : c->keysets)
    for (auto& kv : ks.keys) (void)hipFree(kv.second);
  for (uint64_t* p : c->key_pool) (void)hipFree(p);
  if (c->d_seeds) (void)hipFree(c->d_seeds);
  if (c->d_cq_stage) (void)hipFree(c->d_cq_stage);
  if (c->d_cq_stats) (void)hipFree(c->d_cq_stats);
  if (c->h_cq_stats) (void)hipHostFree(c->h_cq_stats);
  if (c->h_seed_pin) (void)hipHostFree(c->h_seed_pin);
  if (c->h_seeds) (void)hipHostFree(c->h_seeds);
  for (hipEvent_t e : c->ev_seed_pin)
    if (e) (void)hipEventDestroy(e);
  for (void* p : c->allocs) (void)hipFree(p);
  for (BatchSet& b : c->sets) {
    if (b.h_query) (void)hipHostFree(b.h_query);
    if (b.h_reply) (void)hipHostFree(b.h_reply);
    for (hipEvent_t e : b.dl_events) (void)hipEventDestroy(e);
    for (hipEvent_t e : b.rd_events) (void)hipEventDestroy(e);
    for (hipEvent_t e : b.st_events) (void)hipEventDestroy(e);
  }
  for (auto& e : c->ev) (void)hipEventDestroy(e);
  for (auto& e : c->bscan_ev) (void)hipEventDestroy(e);
  for (Worker& w : c->workers) {
    if (w.ev_expanded) (void)hipEventDestroy(w.ev_expanded);
    if (w.ev_scanned) (void)hipEventDestroy(w.ev_scanned);
    if (w.ev_done) (void)hipEventDestroy(w.ev_done);
    if (w.ev_join) (void)hipEventDestroy(w.ev_join);
  }
  for (BatchLane& ln : c->lanes) {
    if (ln.ev_scanned) (void)hipEventDestroy(ln.ev_scanned);
    if (ln.ev_join) (void)hipEventDestroy(ln.ev_join);
    if (ln.stream) (void)hipStreamDestroy(ln.stream);
  }
  if (c->head_stream) {
    (void)hipStreamSynchronize(c->head_stream);
    (void)hipStreamDestroy(c->head_stream);
  }
  if (c->ev_head_tail) (void)hipEventDestroy(c->ev_head_tail);
  for (BatchLane& ln : c->lanes)
    for (HeadSlot& hs : ln.head) {
      if (hs.ev_ready) (void)hipEventDestroy(hs.ev_ready);
      if (hs.ev_free) (void)hipEventDestroy(hs.ev_free);
    }
  if (c->copy_stream) {
    (void)hipStreamSynchronize(c->copy_stream);
    (void)hipStreamDestroy(c->copy_stream);
  }
  for (hipEvent_t e : c->ev_fetch)
    if (e) (void)hipEventDestroy(e);
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_after) (void)hipEventDestroy(c->ev_after);
  if (c->ev_main_join) (void)hipEventDestroy(c->ev_main_join);
  for (size_t i = 1; i < c->workers.size(); ++i)
    if (c->workers[i].stream) (void)hipStreamDestroy(c->workers[i].stream);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

const char* pirgpu_last_error(const pirgpu_ctx* c) {
  if (!c) return "null context";
  if (t_last_error_ctx == c && t_last_error_gen == c->gen)
    return t_last_error.c_str();  // this thread's own last failure on this context
  return c->err.c_str();
}

void pirgpu_set_error(pirgpu_ctx* c, const char* message) { (void)fail(c, 0, message ? message : ""); }

void pirgpu_request_lock(pirgpu_ctx* c) {
  if (c) c->mu.lock();
}
void pirgpu_request_unlock(pirgpu_ctx* c) {
  if (c) c->mu.unlock();
}

int pirgpu_set_transparent_policy(pirgpu_ctx* c, int allow) {
  return guarded(c, [&]() -> int {
    c->allow_transparent = allow != 0;
    return PIRGPU_OK;
  });
}

// Options by name: options.h declares them, resolve_options / resolve_live_options turn them into the context's fields.
int pirgpu_set_option(pirgpu_ctx* c, const char* name, int64_t value) {
  return guarded(c, [&]() -> int {
    if (!name) return fail(c, PIRGPU_INVALID_ARGUMENT, "null option name");
    const OptId id = find_option(name);
    if (id == OPT_COUNT) return fail(c, PIRGPU_INVALID_ARGUMENT, "unknown option " + upper_case(name));
    const OptRow& row = kOptRows[id];
    if (row.kind == OptKind::Early && c->ws_ready)
      return fail(c, PIRGPU_FAILED_PRECONDITION,
                  std::string("option ") + row.name + " shapes the workspace: set it before the context is first used");
    c->options.set(id, value);
    if (row.kind == OptKind::Live) resolve_live_options(c);
    return PIRGPU_OK;
  });
}

int pirgpu_get_option(pirgpu_ctx* c, const char* name, int64_t* value) {
  return guarded(c, [&]() -> int {
    if (!name || !value) return fail(c, PIRGPU_INVALID_ARGUMENT, "null argument");
    const OptId id = find_option(name);
    if (id == OPT_COUNT) return fail(c, PIRGPU_INVALID_ARGUMENT, "unknown option " + upper_case(name));
    *value = c->options.get(id, unset_report(c, id));
    return PIRGPU_OK;
  });
}

uint64_t pirgpu_zero_plaintexts(const pirgpu_ctx* c) { return c ? c->zero_pts : 0; }

int pirgpu_set_remote_zero_plaintexts(pirgpu_ctx* c, uint64_t n) {
  return guarded(c, [&]() -> int {
    c->remote_zero_pts = n;
    return PIRGPU_OK;
  });
}

int pirgpu_check_ready(pirgpu_ctx* c) {
  return guarded(c, [&]() -> int {
    // (tables: what the next query on the table selected with pirgpu_query_use_table would fail with)
    if (!table_loaded(c, c->cur_table)) return fail(c, PIRGPU_FAILED_PRECONDITION, "database not fully loaded");
    check_transparent(c, c->cur_table);
    return PIRGPU_OK;
  });
}

int pirgpu_get_params(const pirgpu_ctx* c, pirgpu_params* out) {
  if (!c || !out) return PIRGPU_INVALID_ARGUMENT;
  *out = c->prm;
  out->shard_begin = c->sb;
  out->shard_end = c->se;
  return PIRGPU_OK;
}

uint64_t pirgpu_db_size(const pirgpu_ctx* c) { return c ? c->n_loaded : 0; }
uint32_t pirgpu_planes(const pirgpu_ctx* c) { return c ? c->planes : 0; }
uint64_t pirgpu_reply_ct_count(const pirgpu_ctx* c) { return c ? c->reply_cts : 0; }
uint64_t pirgpu_reply_ct_words(const pirgpu_ctx* c) { return c ? c->rctw : 0; }

int pirgpu_mod_switch(pirgpu_ctx* c, const uint64_t* cts, uint64_t n, uint32_t r, uint64_t* out) {
  return guarded(c, [&]() -> int {
    if ((!cts || !out) && n) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    if (r < 1 || r >= c->k) return fail(c, PIRGPU_INVALID_ARGUMENT, "r must be in [1, num_data_primes)");
    if (!n) return PIRGPU_OK;
    const size_t in_words = (size_t)n * c->ctw, out_words = (size_t)n * 2 * r * c->N;
    uint64_t* dev = nullptr;
    HIP_TRY(hipMalloc((void**)&dev, (in_words + out_words) * 8));
    try {
      HIP_TRY(hipMemcpyAsync(dev, cts, in_words * 8, hipMemcpyHostToDevice, c->stream));
      HIP_TRY(launch_mod_switch(c->stream, c->dp, dev, dev + in_words, n, c->k, r, c->N, true));
      HIP_TRY(hipMemcpyAsync(out, dev + in_words, out_words * 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
    } catch (...) {
      (void)hipFree(dev);
      throw;
    }
    HIP_TRY(hipFree(dev));
    return PIRGPU_OK;
  });
}

int pirgpu_reply_packing(const pirgpu_ctx* c) { return c && c->pack ? 1 : 0; }
uint64_t pirgpu_reply_unpacked_words(const pirgpu_ctx* c) { return c ? (uint64_t)2 * (c->rp ? c->rp : c->k) * c->N : 0; }

// Test hooks of packed replies (any context): n ciphertexts [2][r][N] over the first r data primes through the device's
// pack kernel, and back through the host's unpack (reply_pack.h -- what a client runs).
int pirgpu_reply_pack(pirgpu_ctx* c, const uint64_t* cts, uint64_t n, uint32_t r, uint64_t* out) {
  return guarded(c, [&]() -> int {
    if ((!cts || !out) && n) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    if (r < 1 || r > c->k) return fail(c, PIRGPU_INVALID_ARGUMENT, "r must be in [1, num_data_primes]");
    if (!n) return PIRGPU_OK;
    const uint32_t N = c->N;
    for (uint64_t i = 0; i < n * 2 * r; ++i) {   // the kernel packs canonical residues: a wider value would spill into its neighbour
      const uint64_t q = c->prm.coeff_modulus[i % r];
      for (uint32_t e = 0; e < N; ++e)
        if (cts[i * N + e] >= q) return fail(c, PIRGPU_INVALID_ARGUMENT, "residue out of range (not below its modulus)");
    }
    const ReplyPackArgs args = reply_pack_args(N, c->prm.coeff_modulus, r, r);
    const uint64_t step = 65535 / (2 * r);       // ciphertexts per launch (grid.y)
    const size_t in_ct = (size_t)2 * r * N, in_words = (size_t)std::min(n, step) * in_ct,
                 out_words = (size_t)std::min(n, step) * args.ct_words;
    uint64_t* dev = nullptr;
    HIP_TRY(hipMalloc((void**)&dev, (in_words + out_words) * 8));
    try {
      for (uint64_t at = 0; at < n; at += step) {
        const uint64_t m = std::min(step, n - at);
        HIP_TRY(hipMemcpyAsync(dev, cts + at * in_ct, m * in_ct * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(launch_reply_pack(c->stream, args, dev, dev + in_words, m));
        HIP_TRY(hipMemcpyAsync(out + at * args.ct_words, dev + in_words, m * args.ct_words * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
      }
    } catch (...) {
      (void)hipFree(dev);
      throw;
    }
    HIP_TRY(hipFree(dev));
    return PIRGPU_OK;
  });
}

int pirgpu_reply_unpack(pirgpu_ctx* c, const uint64_t* packed, uint64_t n, uint32_t r, uint64_t* out) {
  return guarded(c, [&]() -> int {
    if ((!packed || !out) && n) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    if (r < 1 || r > c->k) return fail(c, PIRGPU_INVALID_ARGUMENT, "r must be in [1, num_data_primes]");
    const size_t pw = rpk::ct_words(c->N, c->prm.coeff_modulus, r);
    for (uint64_t i = 0; i < n; ++i)
      if (!rpk::unpack_ct(packed + i * pw, c->N, c->prm.coeff_modulus, r, out + i * 2 * r * c->N))
        return fail(c, PIRGPU_INVALID_ARGUMENT, "packed reply holds a coefficient that is not below its modulus");
    return PIRGPU_OK;
  });
}

int pirgpu_ctmult_plan(uint32_t N, uint32_t k, const uint64_t* coeff_modulus, uint64_t special_prime, uint64_t plain_modulus,
                       uint64_t* aux_primes, uint32_t* n_aux) {
  return pirgpu_ctmult_plan_terms(N, k, coeff_modulus, special_prime, plain_modulus, 1, aux_primes, n_aux);
}

int pirgpu_ctmult_plan_terms(uint32_t N, uint32_t k, const uint64_t* coeff_modulus, uint64_t special_prime,
                             uint64_t plain_modulus, uint64_t terms, uint64_t* aux_primes, uint32_t* n_aux) {
  if (!coeff_modulus || !aux_primes) return PIRGPU_INVALID_ARGUMENT;
  if (n_aux) *n_aux = 0;
  uint64_t aux[kCtmMaxB] = {};
  if (const char* why = ctm::plan(N, k, coeff_modulus, special_prime, plain_modulus, aux, terms)) {
    g_create_error = why;
    return PIRGPU_INVALID_ARGUMENT;
  }
  for (uint32_t i = 0; i < k + 2; ++i) aux_primes[i] = aux[i];
  if (n_aux) *n_aux = k + 2;
  return PIRGPU_OK;
}

int pirgpu_ct_multiply(pirgpu_ctx* c, const uint64_t* a, const uint64_t* b, uint64_t n, uint64_t* out) {
  return guarded(c, [&]() -> int {
    if (!c->ctm) return fail(c, PIRGPU_FAILED_PRECONDITION, "not a ciphertext-multiplication context (PIRGPU_CREATE_CT_MULTIPLY)");
    if ((!a || !b || !out) && n) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    ensure_workspace(c);
    CtmScratch& ws = ctm_scratch(c, c->stream);
    const uint32_t cap = ctm_cap_pairs(c);
    const CtmRegions r = ctm_regions(c, ws.buf, cap);
    const size_t ctw = c->ctw, pw = (size_t)c->k * c->N;
    // CT_SHARED_SEL: behind a and b the block's selectors in NTT form, at Q and at B (pair p reads selector p: dim = m)
    const bool shared = c->ctm_shared_sel;
    const size_t selw = shared ? ctw + (size_t)2 * c->kb * c->N : 0;
    DevScratch in;
    uint64_t* d_in = in.get<uint64_t>((size_t)std::min<uint64_t>(cap, std::max<uint64_t>(n, 1)) * (2 * ctw + selw) * 8);
    std::vector<uint64_t> host;
    for (uint64_t p0 = 0; p0 < n; p0 += cap) {
      const uint32_t m = (uint32_t)std::min<uint64_t>(cap, n - p0);
      uint64_t* d_b = d_in + (size_t)m * ctw;
      HIP_TRY(hipMemcpyAsync(d_in, a + p0 * ctw, (size_t)m * ctw * 8, hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipMemcpyAsync(d_b, b + p0 * ctw, (size_t)m * ctw * 8, hipMemcpyHostToDevice, c->stream));
      c->options.counter(OPT_CT_LIFTS) += (uint64_t)(shared ? 2 : 4) * m;
      if (shared) {
        uint64_t* d_selq = d_b + (size_t)m * ctw;
        const CtmSel sel = ctm_hook_selectors(c, c->stream, d_b, m, d_selq, d_selq + (size_t)m * ctw);
        ctm_products_sel(c, c->stream, r, d_in, 0, sel, m, 1, 0, m);
      } else {
        ctm_products(c, c->stream, r, d_in, 0, d_b, m, 1, 0, m);
      }
      host.resize((size_t)m * 3 * pw);
      HIP_TRY(hipMemcpyAsync(host.data(), r.d, host.size() * 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      for (uint32_t p = 0; p < m; ++p) {   // the device keeps (d0, d2, d1)
        const uint64_t* src = host.data() + (size_t)p * 3 * pw;
        uint64_t* dst = out + (p0 + p) * 3 * pw;
        memcpy(dst, src, pw * 8);
        memcpy(dst + pw, src + 2 * pw, pw * 8);
        memcpy(dst + 2 * pw, src + pw, pw * 8);
      }
    }
    return PIRGPU_OK;
  });
}

int pirgpu_ct_multiply_sum(pirgpu_ctx* c, const uint64_t* a, const uint64_t* b, uint64_t n, uint64_t* out) {
  return guarded(c, [&]() -> int {
    if (!c->ctm) return fail(c, PIRGPU_FAILED_PRECONDITION, "not a ciphertext-multiplication context (PIRGPU_CREATE_CT_MULTIPLY)");
    if (!a || !b || !out) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    if (n < 1 || n > (1u << 20)) return fail(c, PIRGPU_INVALID_ARGUMENT, "n must be in [1, 2^20]");
    uint64_t aux[kCtmMaxB] = {};
    if (const char* why = ctm::plan(c->N, c->k, c->prm.coeff_modulus, c->prm.special_prime, c->prm.plain_modulus, aux, n))
      return fail(c, PIRGPU_INVALID_ARGUMENT, why);
    ensure_workspace(c);
    CtmScratch& ws = ctm_scratch(c, c->stream);
    const uint32_t cap = ctm_cap_pairs(c);
    const CtmRegions r = ctm_regions(c, ws.buf, cap);
    const size_t ctw = c->ctw, pw = (size_t)c->k * c->N;
    // one row of n children, one query: child j is a[j], its selector b[j % n]
    // CT_SHARED_SEL: behind a and b the row's n selectors in NTT form, at Q and at B, made once for all blocks
    const bool shared = c->ctm_shared_sel;
    const size_t selw = shared ? ctw + (size_t)2 * c->kb * c->N : 0;
    DevScratch in;
    uint64_t* d_a = in.get<uint64_t>((size_t)n * (2 * ctw + selw) * 8);
    uint64_t* d_b = d_a + (size_t)n * ctw;
    HIP_TRY(hipMemcpyAsync(d_a, a, (size_t)n * ctw * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_b, b, (size_t)n * ctw * 8, hipMemcpyHostToDevice, c->stream));
    CtmSel sel{};
    if (shared) {
      uint64_t* d_selq = d_b + (size_t)n * ctw;
      sel = ctm_hook_selectors(c, c->stream, d_b, n, d_selq, d_selq + (size_t)n * ctw);
    }
    uint32_t fin = 0;
    for (uint64_t j0 = 0; j0 < n; j0 += cap) {
      const uint32_t nj = (uint32_t)std::min<uint64_t>(cap, n - j0);
      c->options.counter(OPT_CT_LIFTS) += (uint64_t)(shared ? 2 : 4) * nj;
      fin += ctm_rowsum_block(c, c->stream, r, cap, d_a, 0, d_b, (uint32_t)n, 1, n, (uint32_t)j0, nj,
                              shared ? &sel : nullptr);   // (nothing to carry forward)
    }
    if (fin != 1) throw Fail{PIRGPU_INTERNAL, "the row did not finish in its last block"};
    std::vector<uint64_t> host(3 * pw);
    HIP_TRY(hipMemcpyAsync(host.data(), r.d, host.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    memcpy(out, host.data(), pw * 8);   // the device keeps (d0, d2, d1)
    memcpy(out + pw, host.data() + 2 * pw, pw * 8);
    memcpy(out + 2 * pw, host.data() + pw, pw * 8);
    return PIRGPU_OK;
  });
}

int pirgpu_relinearize(pirgpu_ctx* c, const uint64_t* in, uint64_t n, uint64_t* out) {
  return guarded(c, [&]() -> int {
    if (!c->ctm) return fail(c, PIRGPU_FAILED_PRECONDITION, "not a ciphertext-multiplication context (PIRGPU_CREATE_CT_MULTIPLY)");
    if ((!in || !out) && n) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    ensure_workspace(c);
    const uint32_t slot = current_keyset(c);
    const KeyPtrs key = relin_keys_for(c, &slot, 1);
    CtmScratch& ws = ctm_scratch(c, c->stream);
    const uint32_t cap = ctm_cap_pairs(c);
    const CtmRegions r = ctm_regions(c, ws.buf, cap);
    const size_t ctw = c->ctw, pw = (size_t)c->k * c->N;
    std::vector<uint64_t> host;
    for (uint64_t p0 = 0; p0 < n; p0 += cap) {
      const uint32_t m = (uint32_t)std::min<uint64_t>(cap, n - p0);
      host.resize((size_t)m * 3 * pw);
      for (uint32_t p = 0; p < m; ++p) {   // (d0, d1, d2) -> the device's (d0, d2, d1)
        const uint64_t* src = in + (p0 + p) * 3 * pw;
        uint64_t* dst = host.data() + (size_t)p * 3 * pw;
        memcpy(dst, src, pw * 8);
        memcpy(dst + pw, src + 2 * pw, pw * 8);
        memcpy(dst + 2 * pw, src + pw, pw * 8);
      }
      HIP_TRY(hipMemcpyAsync(r.d, host.data(), host.size() * 8, hipMemcpyHostToDevice, c->stream));
      ctm_relinearize(c, c->stream, r, m, key);
      // + d1 on component 1: the accumulation of the query path with one child per row
      HIP_TRY(launch_ctm_accumulate(c->stream, c->dp, c->k, c->N, r.yq, r.d, r.yb, 0, 1, 1, 0, m, m));
      HIP_TRY(hipMemcpyAsync(out + p0 * ctw, r.yb, (size_t)m * ctw * 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return PIRGPU_OK;
  });
}

uint32_t pirgpu_expansion_ratio(const pirgpu_ctx* c) { return c ? c->er : 0; }
uint64_t pirgpu_scan_bytes(const pirgpu_ctx* cc) {
  pirgpu_ctx* c = const_cast<pirgpu_ctx*>(cc);
  if (!c) return 0;
  try {
    c->use_device();
    ensure_workspace(c);
  } catch (...) {
    return 0;
  }
  // bytes a single-query pass over the database must read: the operand-layout copy when that pass is the MFMA scan
  // (tables: a query scans the table it names and nothing else)
  return c->mfma_on && c->mfma_single ? (uint64_t)dbp_bytes(c) : held_pts(c) / c->tables * c->k * c->N * 8;
}

int pirgpu_ntt_mode(const pirgpu_ctx* c) { return c ? c->mode : -1; }

int pirgpu_arith_info(pirgpu_ctx* c, uint32_t info[8]) {
  return guarded(c, [&]() -> int {
    if (!info) return fail(c, PIRGPU_INVALID_ARGUMENT, "null info");
    ensure_workspace(c);
    info[0] = (uint32_t)c->mode;
    info[1] = c->mode == kNttF64 ? c->hp.f64_lazy_inv : 0u;   // only the exact-fp64 flavour reads the flag (ntt_core.h)
    info[2] = c->pack40 ? (uint32_t)c->pack_bytes : 8u;
    info[3] = c->tree40 && c->pack40 ? 1u : 0u;
    info[4] = c->hp.lazy_limit;
    info[5] = (c->scan_f64_fold ? 1u : 0u) | (c->scan_f64_fold_batch ? 2u : 0u) | (c->scan_limb ? 4u : 0u);
    info[6] = info[7] = 0;
    return PIRGPU_OK;
  });
}

int pirgpu_scan_info(pirgpu_ctx* c, uint32_t info[8]) {
  return guarded(c, [&]() -> int {
    if (!info) return fail(c, PIRGPU_INVALID_ARGUMENT, "null info");
    ensure_workspace(c);
    info[0] = c->mfma_on ? 1 : 0;
    info[1] = c->mfma_on ? c->mg.L : 0;
    info[2] = c->mfma_on ? c->mg.nchunks : c->scan_nsplit;
    info[3] = c->mfma_on ? c->mg.KS : 0;
    info[4] = c->mfma_on ? c->mfma_nq : (mq_usable(c) ? std::min<uint32_t>(c->mq_nq, kMaxScanQueries) : 1);
    info[5] = c->scan_rows;
    info[6] = c->scan_cols;
    info[7] = (c->mfma_on && c->mfma_single ? 1u : 0u) | (c->mfma_on && c->mg.top4 ? 2u : 0u);
    return PIRGPU_OK;
  });
}

int pirgpu_expansion_forms(pirgpu_ctx* c, uint32_t B, uint32_t n, int head_split, uint32_t* out, uint32_t cap, uint32_t* count) {
  return guarded(c, [&]() -> int {
    if (!count || (cap && !out)) return fail(c, PIRGPU_INVALID_ARGUMENT, "null output");
    if (B == 0 || B > (uint32_t)kMaxMfmaQueries) return fail(c, PIRGPU_INVALID_ARGUMENT, "group size out of range");
    if (n == 0 || n > c->N) return fail(c, PIRGPU_INVALID_ARGUMENT, "slot count out of range");
    ensure_workspace(c);
    const ExpandOptions eo = expand_options(c);
    const bool sel_f64 = c->sel_f64;   // (what the MFMA batch path hands its groups; single queries never take it)
    // the split expand_group_on_lane takes for this context's queries when HEAD_MODE (or the staging) asks for one
    const bool use_head = head_split && expansion_uses_head(c->dim_sum / c->N + 1, B, c->head_levels, true,
                                                            expansion_depth((uint32_t)std::min<uint64_t>(c->dim_sum, c->N)));
    uint32_t w = 0;
    auto emit = [&](const ExpandPlan& p, bool on_head) {
      for (const ExpandLevel& L : p.levels) {
        if (w < cap) out[w] = pack_expand_level(L, on_head, sel_f64);
        ++w;
      }
    };
    if (use_head) {
      const ExpandPlan head = plan_expansion(c->N, c->logN, c->k, B, n, true, eo, 0, c->head_levels);
      emit(head, true);
      if (head.valid()) emit(plan_expansion(c->N, c->logN, c->k, B, n, true, eo, c->head_levels, UINT32_MAX, &head.out), false);
    } else {
      emit(plan_expansion(c->N, c->logN, c->k, B, n, true, eo), false);
    }
    *count = w;
    return PIRGPU_OK;
  });
}

// PIRDatabase::populate for one table of the context (the only one unless tables > 1): num_items == params.num_items
// items into the plaintext rows of table `table`, whose loaded[] entries start at table * num_pt.
static int load_table_items(pirgpu_ctx* c, uint32_t table, const uint8_t* items, uint64_t num_items, uint32_t bytes_per_item);

int pirgpu_db_load_items(pirgpu_ctx* c, const uint8_t* items, uint64_t num_items, uint32_t bytes_per_item) {
  return guarded(c, [&]() -> int {
    const pirgpu_params& p = c->prm;
    if (num_items != c->tables * p.num_items)  // reference database.cpp:85-90 (tables: all of them, table-major)
      return fail(c, PIRGPU_INVALID_ARGUMENT,
                  "Database size " + std::to_string(num_items) + " does not match params value " +
                      std::to_string(c->tables * p.num_items));
    for (uint32_t t = 0; t < c->tables; ++t) {
      const int rc = load_table_items(c, t, items ? items + (size_t)t * p.num_items * bytes_per_item : nullptr, p.num_items,
                                      bytes_per_item);
      if (rc) return rc;
    }
    return PIRGPU_OK;
  });
}

int pirgpu_db_load_table_items(pirgpu_ctx* c, uint32_t table, const uint8_t* items, uint64_t num_items,
                               uint32_t bytes_per_item) {
  return guarded(c, [&]() -> int {
    if (table >= c->tables)
      return fail(c, PIRGPU_INVALID_ARGUMENT, "table " + std::to_string(table) + " out of range (tables = " +
                                                  std::to_string(c->tables) + ")");
    if (num_items != c->prm.num_items)
      return fail(c, PIRGPU_INVALID_ARGUMENT,
                  "Database size " + std::to_string(num_items) + " does not match params value " +
                      std::to_string(c->prm.num_items));
    if (c->tables > 1) {   // a RELOAD overwrites rows that queued queries on this table may still read
      sync_batch_streams(c);
      HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return load_table_items(c, table, items, num_items, bytes_per_item);
  });
}

static int load_table_items(pirgpu_ctx* c, uint32_t table, const uint8_t* items, uint64_t num_items, uint32_t bytes_per_item) {
  {
    const pirgpu_params& p = c->prm;
    if (bytes_per_item != p.bytes_per_item || p.items_per_plaintext == 0 || (!items && num_items))
      return fail(c, PIRGPU_INVALID_ARGUMENT, "item size does not match parameters");
    const uint64_t ipp = p.items_per_plaintext;
    const uint64_t bytes_per_pt = ipp * bytes_per_item;
    if (c->staging_released)
      return fail(c, PIRGPU_FAILED_PRECONDITION, "database staging was released by pirgpu_db_finalize; it cannot be reloaded");
    // streamed context: a chunk is a whole number of row bands, encoded into a compact scratch and packed from there
    // (pack_range); the raw-byte upload buffer is sized to the same chunk
    const uint64_t kN = (uint64_t)c->k * c->N;
    if (!c->streamed) c->packed_valid = false;
    if (c->tables > 1) c->tbl_packed[table] = 0;
    const uint64_t row0 = (uint64_t)table * c->table_pad;   // first staging row / loaded[] entry of the table (0 without
    const uint64_t idx0 = (uint64_t)table * c->P;           // tables)
    if (c->planes > 1) {
      // wide items: item i is uploaded once and the encode kernel cuts it into its planes -- plane j reads bytes
      // [j B, min((j + 1) B, bytes_per_item)) of it and writes plaintext row j * plane_pad + i
      if (num_items > c->P) return fail(c, PIRGPU_INVALID_ARGUMENT, "more items than plaintexts");
      if (c->streamed) begin_streamed_load(c);
      const uint64_t B = (uint64_t)c->N * c->bits / 8;
      // (streamed: one item chunk becomes `planes` compact pieces [planes][n][k][N], so the bands are shared out)
      const uint64_t chunk_items = c->streamed ? stream_chunk_pts(c, c->stream_bands / c->planes, c->P)
                                               : std::max<uint64_t>(1, (64ull << 20) / bytes_per_item);
      DevScratch s_bytes, s_enc, s_units;
      const uint64_t enc_bytes = c->streamed ? c->planes * chunk_items * kN * 8 : 0;
      ScratchNote held(c, chunk_items * bytes_per_item + enc_bytes + (c->streamed ? stream_unit_bytes(c) : 0));
      uint8_t* d_bytes = s_bytes.get<uint8_t>(chunk_items * bytes_per_item);
      uint64_t* d_enc = c->streamed ? s_enc.get<uint64_t>(enc_bytes) : nullptr;
      DbUnit* d_units = c->streamed ? s_units.get<DbUnit>(stream_unit_bytes(c)) : nullptr;
      for (uint64_t it = 0; it < c->P; it += chunk_items) {
        const uint64_t n = std::min<uint64_t>(chunk_items, c->P - it);
        const uint64_t have = it < num_items ? std::min<uint64_t>(n, num_items - it) : 0;   // plaintexts past the items: zero
        if (have)
          HIP_TRY(hipMemcpyAsync(d_bytes, items + it * bytes_per_item, have * bytes_per_item, hipMemcpyHostToDevice, c->stream));
        for (uint32_t pl = 0; pl < c->planes; ++pl) {
          const uint64_t off = pl * B, len = std::min<uint64_t>(B, bytes_per_item - off);
          for (uint64_t i = 0; i < n; ++i)
            note_plaintext(c, pl * c->P + it + i,
                           it + i >= num_items || all_zero_bytes(items + (it + i) * bytes_per_item + off, len));
        }
        if (c->streamed) {
          HIP_TRY(c->ops->db_encode(c->stream, c->mode, c->dp, c->k, nullptr, d_bytes, bytes_per_item, have * bytes_per_item,
                                    c->bits, n, d_enc, c->planes, B, n));
          for (uint32_t pl = 0; pl < c->planes; ++pl)   // plane pl's rows start at pl * plane_pad: no tile boundary
            pack_range(c, d_enc + pl * n * kN, pl * c->plane_pad + it, n, d_units);
          continue;
        }
        HIP_TRY(c->ops->db_encode(c->stream, c->mode, c->dp, c->k, nullptr, d_bytes, bytes_per_item, have * bytes_per_item,
                                  c->bits, n, c->d_db + it * c->k * c->N, c->planes, B, c->plane_pad));
        HIP_TRY(hipStreamSynchronize(c->stream));
      }
      return PIRGPU_OK;
    }
    // StringEncoder::calc_num_coeff (reference string_encoder.cpp:88-95)
    if ((uint64_t)std::ceil((double)(bytes_per_pt * 8) / c->bits) > c->N)
      return fail(c, PIRGPU_INVALID_ARGUMENT, "Number of coefficients needed greater than poly modulus degree");
    if (ceil_div(num_items, ipp) > c->P) return fail(c, PIRGPU_INVALID_ARGUMENT, "more items than plaintexts");
    if (c->streamed) begin_streamed_load(c);
    const uint64_t total_bytes = num_items * bytes_per_item;
    const uint64_t chunk_pts = c->streamed ? stream_chunk_pts(c, c->stream_bands, c->pt_end - c->pt_begin)
                                           : std::max<uint64_t>(1, (64ull << 20) / std::max<uint64_t>(bytes_per_pt, 1));
    DevScratch s_enc, s_units;
    ScratchNote held(c, chunk_pts * bytes_per_pt + (c->streamed ? chunk_pts * kN * 8 + stream_unit_bytes(c) : 0));
    uint64_t* d_enc = c->streamed ? s_enc.get<uint64_t>(chunk_pts * kN * 8) : nullptr;
    DbUnit* d_units = c->streamed ? s_units.get<DbUnit>(stream_unit_bytes(c)) : nullptr;
    uint8_t* d_bytes = nullptr;
    HIP_TRY(hipMalloc((void**)&d_bytes, chunk_pts * bytes_per_pt));
    try {
      for (uint64_t pt = c->pt_begin; pt < c->pt_end; pt += chunk_pts) {
        const uint64_t n = std::min<uint64_t>(chunk_pts, c->pt_end - pt);
        const uint64_t b0 = std::min<uint64_t>(pt * bytes_per_pt, total_bytes);
        const uint64_t b1 = std::min<uint64_t>((pt + n) * bytes_per_pt, total_bytes);
        if (b1 > b0) HIP_TRY(hipMemcpyAsync(d_bytes, items + b0, b1 - b0, hipMemcpyHostToDevice, c->stream));
        for (uint64_t i = 0; i < n; ++i) {  // all-zero plaintexts (host scan while the copy is in flight)
          const uint64_t p0 = std::min<uint64_t>((pt + i) * bytes_per_pt, total_bytes);
          const uint64_t p1 = std::min<uint64_t>((pt + i + 1) * bytes_per_pt, total_bytes);
          note_plaintext(c, idx0 + pt - c->pt_begin + i, all_zero_bytes(items + p0, p1 - p0));
        }
        HIP_TRY(c->ops->db_encode(c->stream, c->mode, c->dp, c->k, nullptr, d_bytes, bytes_per_pt, b1 - b0, c->bits,
                                  n, c->streamed ? d_enc : c->d_db + (row0 + pt - c->pt_begin) * c->k * c->N, 1, 0, 0));
        if (c->streamed) pack_range(c, d_enc, pt - c->pt_begin, n, d_units);
        HIP_TRY(hipStreamSynchronize(c->stream));
      }
    } catch (...) {
      (void)hipFree(d_bytes);
      throw;
    }
    HIP_TRY(hipFree(d_bytes));
    return PIRGPU_OK;
  }
}

int pirgpu_db_load_coeffs(pirgpu_ctx* c, uint64_t first_pt, uint64_t n_pt, const uint64_t* coeffs) {
  return guarded(c, [&]() -> int {
    if (first_pt + n_pt > (uint64_t)c->tables * c->planes * c->P || (!coeffs && n_pt))
      return fail(c, PIRGPU_INVALID_ARGUMENT, "plaintext range out of bounds");
    // (wide items: pt_begin = 0, pt_end = P, and the index runs over all planes, plane-major)
    const uint64_t lo = std::max(first_pt, c->pt_begin);
    const uint64_t hi = c->planes > 1 || c->tables > 1 ? first_pt + n_pt : std::min(first_pt + n_pt, c->pt_end);
    if (lo >= hi) return PIRGPU_OK;
    if (c->staging_released)
      return fail(c, PIRGPU_FAILED_PRECONDITION, "database staging was released by pirgpu_db_finalize; it cannot be reloaded");
    if (c->streamed) begin_streamed_load(c);
    else c->packed_valid = false;
    // (streamed: chunks of whole row bands through a compact scratch and pack_range, as in pirgpu_db_load_items)
    const uint64_t kN = (uint64_t)c->k * c->N;
    const uint64_t chunk = c->streamed ? stream_chunk_pts(c, c->stream_bands, hi - lo)
                                       : std::max<uint64_t>(1, (64ull << 20) / (c->N * 8));
    DevScratch s_enc, s_units;
    ScratchNote held(c, chunk * c->N * 8 + (c->streamed ? chunk * kN * 8 + stream_unit_bytes(c) : 0));
    uint64_t* d_enc = c->streamed ? s_enc.get<uint64_t>(chunk * kN * 8) : nullptr;
    DbUnit* d_units = c->streamed ? s_units.get<DbUnit>(stream_unit_bytes(c)) : nullptr;
    uint64_t* d_coeffs = nullptr;
    HIP_TRY(hipMalloc((void**)&d_coeffs, chunk * c->N * 8));
    try {
      for (uint64_t pt = lo; pt < hi;) {
        // a piece never crosses a plane boundary: the rows of one plane are contiguous in d_db
        // (nor a table boundary: table-major indices, every table's rows contiguous)
        uint64_t n = std::min<uint64_t>(std::min<uint64_t>(chunk, hi - pt),
                                        c->planes > 1 || c->tables > 1 ? c->P - pt % c->P : chunk);
        if (c->tables > 1) c->tbl_packed[pt / c->P] = 0;
        // (streamed: the first piece ends on a chunk boundary of the matrix, so that the later ones are whole row tiles)
        if (c->streamed) n = std::min<uint64_t>(n, chunk - db_row(c, pt) % chunk);
        HIP_TRY(hipMemcpyAsync(d_coeffs, coeffs + (pt - first_pt) * c->N, n * c->N * 8, hipMemcpyHostToDevice,
                               c->stream));
        for (uint64_t i = 0; i < n; ++i)
          note_plaintext(c, pt - c->pt_begin + i,
                         all_zero_bytes(reinterpret_cast<const uint8_t*>(coeffs + (pt - first_pt + i) * c->N),
                                        (size_t)c->N * 8));
        HIP_TRY(c->ops->db_encode(c->stream, c->mode, c->dp, c->k, d_coeffs, nullptr, 0, 0, c->bits, n,
                                  c->streamed ? d_enc : c->d_db + db_row(c, pt) * c->k * c->N, 1, 0, 0));
        if (c->streamed) pack_range(c, d_enc, db_row(c, pt), n, d_units);
        HIP_TRY(hipStreamSynchronize(c->stream));
        pt += n;
      }
    } catch (...) {
      (void)hipFree(d_coeffs);
      throw;
    }
    HIP_TRY(hipFree(d_coeffs));
    return PIRGPU_OK;
  });
}

int pirgpu_db_finalize(pirgpu_ctx* c, int release_staging) {
  return guarded(c, [&]() -> int {
    ensure_workspace(c);
    if (c->n_loaded != held_pts(c)) return fail(c, PIRGPU_FAILED_PRECONDITION, "database not fully loaded");
    ensure_packed(c);
    if (release_staging && c->mfma_on && c->d_db) {
      sync_batch_streams(c);
      HIP_TRY(hipStreamSynchronize(c->stream));
      auto it = std::find(c->allocs.begin(), c->allocs.end(), (void*)c->d_db);
      if (it != c->allocs.end()) c->allocs.erase(it);
      HIP_TRY(hipFree(c->d_db));
      c->d_db = nullptr;
      c->db_bytes = 0;
      c->staging_released = true;
      c->mfma_single = true;  // the 64-bit kernels read the staging copy
    }
    return PIRGPU_OK;
  });
}

int pirgpu_db_read_plaintext(pirgpu_ctx* c, uint64_t pt_index, uint64_t* out) {
  return guarded(c, [&]() -> int {
    if (pt_index < c->pt_begin ||
        pt_index >= (c->tables > 1 ? c->tables * c->P : c->planes > 1 ? c->planes * c->P : c->pt_end) || !out)
      return fail(c, PIRGPU_INVALID_ARGUMENT, "plaintext index outside this shard");
    uint64_t* stage = nullptr;
    HIP_TRY(hipMalloc((void**)&stage, (size_t)2 * c->k * c->N * 8));
    try {
      const uint64_t* src = c->d_db ? c->d_db + db_row(c, pt_index) * c->k * c->N : nullptr;
      if (!src) {  // staging released: gather the digits of this plaintext from the operand layout
        refuse_slot_shard(c);   // ... which a slot shard holds only 1 / G of
        if (!c->d_dbp)          // (a streamed context before its first load)
          throw Fail{PIRGPU_FAILED_PRECONDITION, "database not loaded: the operand-layout copy does not exist yet"};
        // (tables: the position inside the table's own layout)
        const uint64_t local = c->tables > 1 ? pt_index % c->P : db_row(c, pt_index);
        uint64_t* tmp = stage + (size_t)c->k * c->N;
        HIP_TRY(launch_db_unpack(c->stream, c->dp, c->mg, table_dbp(c, c->tables > 1 ? (uint32_t)(pt_index / c->P) : 0), tmp,
                                 (uint32_t)(local / c->scan_cols),
                                 (uint32_t)(local % c->scan_cols), c->k * c->N));
        src = tmp;
      }
      HIP_TRY(launch_ntt_reorder(c->stream, c->N, src, stage, c->k, false, false));
      HIP_TRY(hipMemcpyAsync(out, stage, (size_t)c->k * c->N * 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
    } catch (...) {
      (void)hipFree(stage);
      throw;
    }
    HIP_TRY(hipFree(stage));
    return PIRGPU_OK;
  });
}

int pirgpu_db_memory(const pirgpu_ctx* cc, uint64_t out[4]) {
  pirgpu_ctx* c = const_cast<pirgpu_ctx*>(cc);
  return guarded(c, [&]() -> int {
    if (!out) return fail(c, PIRGPU_INVALID_ARGUMENT, "null argument");
    ensure_workspace(c);   // a streamed context's operand copy and band size exist once the geometry is fixed
    out[0] = c->dbp_alloc;
    out[1] = c->db_bytes;
    out[2] = c->mem_peak;
    out[3] = c->streamed && c->mfma_on ? stream_band_bytes(c) : 0;
    return PIRGPU_OK;
  });
}

int pirgpu_db_read_operand(pirgpu_ctx* c, uint64_t offset, uint64_t n, uint8_t* out) {
  return guarded(c, [&]() -> int {
    if (!c->d_dbp) return fail(c, PIRGPU_FAILED_PRECONDITION, "the operand-layout copy does not exist yet");
    if (offset > c->dbp_alloc || n > c->dbp_alloc - offset || (!out && n))
      return fail(c, PIRGPU_INVALID_ARGUMENT, "byte range outside the operand-layout copy");
    if (!n) return PIRGPU_OK;
    sync_batch_streams(c);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, c->d_dbp + offset, n, hipMemcpyDeviceToHost));
    return PIRGPU_OK;
  });
}

// In-place updates (pirgpu_db_update_items / _plaintexts).  The touched plaintexts (sorted by local index) go through
// the device in chunks: [fetch residue 0 of the old NTT form (staging row, or db_gather from the operand layout) ->
// inverse NTT -> db_splice] (item updates only) -> lift + forward NTT (db_encode) into a compact [n][k][N] buffer ->
// staging rows and the touched columns of the operand layout (db_pack_update).  No repack: packed_valid is kept.
}  // extern "C"

namespace {

struct PtUpdate {
  uint64_t local;                                     // ABI plaintext index - pt_begin (plane-major for wide items)
  const uint64_t* coeffs = nullptr;                   // update_plaintexts: its new coefficient row
  std::vector<std::pair<uint32_t, uint64_t>> items;   // update_items: (item slot in the plaintext, row of `items`)
};

// Waits for every queued use of the database (as pirgpu_db_finalize does before it frees the staging copy).
void quiesce(pirgpu_ctx* c) {
  sync_batch_streams(c);
  HIP_TRY(hipStreamSynchronize(c->stream));
}

void require_loaded(pirgpu_ctx* c) {
  if (c->n_loaded != held_pts(c) || c->pt_end == c->pt_begin)
    throw Fail{PIRGPU_FAILED_PRECONDITION, "database not fully loaded (the first load is pirgpu_db_load_items / _coeffs)"};
}

// Tables: `pts` lie in ONE table (apply_update_tables cuts the sorted list), whose operand layout the units index.
void apply_update(pirgpu_ctx* c, const std::vector<PtUpdate>& pts, const uint8_t* items, uint32_t item_bytes,
                  uint32_t table = 0) {
  const uint32_t N = c->N, kN = c->k * c->N;
  uint8_t* const dbp = table_dbp(c, table);
  const uint64_t table_row0 = (uint64_t)table * c->table_pad;   // 0 without tables
  // wide items: a touched plaintext is one whole plane of ONE item (items_per_plaintext = 1), nothing of the old
  // plaintext survives -- no fetch, no inverse transform, no splice: the plane's bytes are encoded like a first load
  const bool wide = items != nullptr && c->planes > 1;
  const bool splice = items != nullptr && !wide;
  const uint64_t plane_bytes = (uint64_t)N * c->bits / 8;
  const uint64_t ipp = splice ? c->prm.items_per_plaintext : 0, bpp = wide ? plane_bytes : ipp * item_bytes;
  const bool to_packed = c->mfma_on && c->packed_valid && c->d_dbp;
  if (c->tables > 1 && !to_packed) c->tbl_packed[table] = 0;   // the next ensure_packed packs this table again
  // chunks of at most 64 MB of device scratch (pirgpu_db_load_items' upload size) and 65535 units (grid.y)
  const uint64_t per_pt = (uint64_t)N * 8 + (uint64_t)kN * 8 + bpp + ipp + 8 + 4 + sizeof(DbUnit);
  const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>((64ull << 20) / per_pt, 65535));
  const uint64_t cap = std::min<uint64_t>(chunk, pts.size());
  DevScratch s_coef, s_enc, s_loc, s_units, s_img, s_upd, s_nz;
  ScratchNote held(c, cap * ((uint64_t)N * 8 + (uint64_t)kN * 8 + 8 + sizeof(DbUnit) +
                             (splice || wide ? bpp : 0) + (splice ? ipp + 4 : 0)));
  uint64_t* d_coef = s_coef.get<uint64_t>(cap * N * 8);
  uint64_t* d_enc = s_enc.get<uint64_t>(cap * kN * 8);
  uint64_t* d_loc = s_loc.get<uint64_t>(cap * 8);
  DbUnit* d_units = s_units.get<DbUnit>(cap * sizeof(DbUnit));
  uint8_t* d_img = splice || wide ? s_img.get<uint8_t>(cap * bpp) : nullptr;
  uint8_t* d_upd = splice ? s_upd.get<uint8_t>(cap * ipp) : nullptr;
  uint32_t* d_nz = splice ? s_nz.get<uint32_t>(cap * 4) : nullptr;
  std::vector<uint64_t> loc, coef_rows;
  std::vector<DbUnit> units;
  std::vector<uint8_t> img, upd;
  std::vector<uint32_t> nz;
  for (uint64_t b = 0; b < pts.size(); b += chunk) {
    const uint64_t n = std::min<uint64_t>(chunk, pts.size() - b);
    loc.resize(n);
    units.clear();
    for (uint64_t i = 0; i < n; ++i) {
      const uint64_t l = db_row(c, pts[b + i].local + c->pt_begin);   // row of d_db = position in the scanned matrix
      loc[i] = l;                                                      // (tables: table_row0 + the position in the table's)
      if (!to_packed) continue;
      const uint64_t lt = l - table_row0;
      const uint32_t r = (uint32_t)(lt / c->scan_cols), col = (uint32_t)(lt % c->scan_cols), kg = col / 16;
      if (units.empty() || units.back().r != r || units.back().kg != kg) units.push_back(DbUnit{r, kg, 0u, (uint32_t)i});
      units.back().mask |= 1u << (col % 16);
    }
    HIP_TRY(hipMemcpyAsync(d_loc, loc.data(), n * 8, hipMemcpyHostToDevice, c->stream));
    if (!units.empty())
      HIP_TRY(hipMemcpyAsync(d_units, units.data(), units.size() * sizeof(DbUnit), hipMemcpyHostToDevice, c->stream));
    std::vector<uint8_t> zero_pt;
    if (wide) {
      img.assign(n * bpp, 0);
      zero_pt.resize(n);
      for (uint64_t i = 0; i < n; ++i) {
        const uint64_t off = pts[b + i].local / c->P * plane_bytes, len = std::min<uint64_t>(plane_bytes, item_bytes - off);
        memcpy(&img[i * bpp], items + pts[b + i].items[0].second * item_bytes + off, len);
        zero_pt[i] = all_zero_bytes(&img[i * bpp], len);
      }
      HIP_TRY(hipMemcpyAsync(d_img, img.data(), n * bpp, hipMemcpyHostToDevice, c->stream));
    } else if (splice) {
      img.assign(n * bpp, 0);
      upd.assign(n * ipp, 0);
      for (uint64_t i = 0; i < n; ++i)
        for (const auto& it : pts[b + i].items) {
          memcpy(&img[i * bpp + (uint64_t)it.first * item_bytes], items + it.second * item_bytes, item_bytes);
          upd[i * ipp + it.first] = 1;
        }
      HIP_TRY(hipMemcpyAsync(d_img, img.data(), n * bpp, hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipMemcpyAsync(d_upd, upd.data(), n * ipp, hipMemcpyHostToDevice, c->stream));
      // (1) residue 0 of the old NTT form
      if (c->d_db)
        HIP_TRY(launch_copy_rows(c->stream, c->d_db, d_coef, d_loc, nullptr, n, N, kN, N));
      else
        HIP_TRY(launch_db_gather(c->stream, c->dp, c->mg, dbp, d_units, (uint32_t)units.size(), d_coef, N));
      // (2) back to coefficients (residues < t < q_0 carry the plaintext exactly), (3) splice
      HIP_TRY(c->ops->ntt_batch(c->stream, c->mode, c->dp, d_coef, n, 1, 0, true));
      HIP_TRY(launch_db_splice(c->stream, c->dp, d_coef, N, d_img, d_upd, n, bpp, item_bytes, c->bits, d_nz));
    } else {
      coef_rows.resize(n * N);
      for (uint64_t i = 0; i < n; ++i) memcpy(&coef_rows[i * N], pts[b + i].coeffs, (size_t)N * 8);
      HIP_TRY(hipMemcpyAsync(d_coef, coef_rows.data(), n * N * 8, hipMemcpyHostToDevice, c->stream));
    }
    // (4) lift + forward NTT, (5) write back
    if (wide)
      HIP_TRY(c->ops->db_encode(c->stream, c->mode, c->dp, c->k, nullptr, d_img, bpp, n * bpp, c->bits, n, d_enc, 1, 0, 0));
    else
      HIP_TRY(c->ops->db_encode(c->stream, c->mode, c->dp, c->k, d_coef, nullptr, 0, 0, c->bits, n, d_enc, 1, 0, 0));
    if (c->d_db) HIP_TRY(launch_copy_rows(c->stream, d_enc, c->d_db, nullptr, d_loc, n, kN, kN, kN));
    if (to_packed)
      HIP_TRY(launch_db_pack_update(c->stream, c->dp, c->mg, d_enc, d_units, (uint32_t)units.size(), dbp, kN,
                                    c->slot0, c->nslots));
    if (splice) {
      nz.resize(n);
      HIP_TRY(hipMemcpyAsync(nz.data(), d_nz, n * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint64_t i = 0; i < n; ++i)
      note_plaintext(c, pts[b + i].local,
                     wide ? zero_pt[i] != 0 : splice ? nz[i] == 0
                            : all_zero_bytes(reinterpret_cast<const uint8_t*>(pts[b + i].coeffs), (size_t)N * 8));
  }
}

// The sorted touched plaintexts of an update, table by table (without tables: one call).
void apply_update_tables(pirgpu_ctx* c, const std::vector<PtUpdate>& pts, const uint8_t* items, uint32_t item_bytes) {
  if (c->tables <= 1) return apply_update(c, pts, items, item_bytes);
  for (size_t b = 0; b < pts.size();) {
    const uint64_t t = pts[b].local / c->P;
    size_t e = b;
    while (e < pts.size() && pts[e].local / c->P == t) ++e;
    apply_update(c, std::vector<PtUpdate>(pts.begin() + b, pts.begin() + e), items, item_bytes, (uint32_t)t);
    b = e;
  }
}

}  // namespace

extern "C" {

int pirgpu_db_update_items(pirgpu_ctx* c, uint64_t n, const uint64_t* item_indices, const uint8_t* items,
                           uint32_t bytes_per_item) {
  return guarded(c, [&]() -> int {
    const pirgpu_params& p = c->prm;
    require_loaded(c);
    if (bytes_per_item != p.bytes_per_item || p.items_per_plaintext == 0)
      return fail(c, PIRGPU_INVALID_ARGUMENT, "item size does not match parameters");
    if (!n) return PIRGPU_OK;
    if (!item_indices || !items) return fail(c, PIRGPU_INVALID_ARGUMENT, "null item indices or items");
    for (uint64_t i = 0; i < n; ++i)
      if (item_indices[i] >= c->tables * p.num_items)
        return fail(c, PIRGPU_INVALID_ARGUMENT, "item index " + std::to_string(item_indices[i]) + " out of range (" +
                                                    std::to_string(c->tables * p.num_items) + " items)");
    if (c->slot_sharded && !c->d_db)
      return fail(c, PIRGPU_FAILED_PRECONDITION,
                  "this slot shard released its staging copy: it holds too little of each plaintext to keep the items "
                  "an update does not replace (pirgpu_db_update_plaintexts still works)");
    const uint64_t ipp = p.items_per_plaintext;
    std::map<uint64_t, uint64_t> last;   // item -> row of `items` (a later entry wins)
    // (tables: item index = table * num_items + i -- ascending item indices are ascending (table, plaintext) pairs)
    const uint64_t ni = c->tables > 1 ? p.num_items : UINT64_MAX;
    for (uint64_t i = 0; i < n; ++i) {
      const uint64_t pt = item_indices[i] % ni / ipp;
      if (pt >= c->pt_begin && pt < c->pt_end) last[item_indices[i]] = i;   // other row shards' items are skipped
    }
    std::vector<PtUpdate> pts;
    if (c->planes > 1) {   // every plane of every touched item, plane-major (= ascending rows of the scanned matrix)
      for (uint32_t pl = 0; pl < c->planes; ++pl)
        for (const auto& e : last) {
          pts.push_back(PtUpdate{pl * c->P + e.first});
          pts.back().items.emplace_back(0u, e.second);
        }
      last.clear();
    }
    for (const auto& e : last) {
      const uint64_t in_table = e.first % ni;
      const uint64_t local = (c->tables > 1 ? e.first / ni * c->P : 0) + in_table / ipp - c->pt_begin;
      if (pts.empty() || pts.back().local != local) pts.push_back(PtUpdate{local});
      pts.back().items.emplace_back((uint32_t)(in_table % ipp), e.second);
    }
    if (pts.empty()) return PIRGPU_OK;
    quiesce(c);
    apply_update_tables(c, pts, items, bytes_per_item);
    return PIRGPU_OK;
  });
}

int pirgpu_db_update_plaintexts(pirgpu_ctx* c, uint64_t n, const uint64_t* pt_indices, const uint64_t* coeffs) {
  return guarded(c, [&]() -> int {
    require_loaded(c);
    if (!n) return PIRGPU_OK;
    if (!pt_indices || !coeffs) return fail(c, PIRGPU_INVALID_ARGUMENT, "null plaintext indices or coefficients");
    const uint64_t t = c->prm.plain_modulus;
    for (uint64_t i = 0; i < n; ++i) {
      if (pt_indices[i] >= (uint64_t)c->tables * c->planes * c->P)
        return fail(c, PIRGPU_INVALID_ARGUMENT, "plaintext index " + std::to_string(pt_indices[i]) + " out of range (" +
                                                    std::to_string((uint64_t)c->tables * c->planes * c->P) + " plaintexts)");
      const uint64_t* row = coeffs + i * c->N;
      for (uint32_t x = 0; x < c->N; ++x)
        if (row[x] >= t) return fail(c, PIRGPU_INVALID_ARGUMENT, "coefficient not below the plain modulus");
    }
    std::map<uint64_t, uint64_t> last;   // local plaintext -> row of `coeffs` (a later entry wins)
    for (uint64_t i = 0; i < n; ++i)
      if (c->planes > 1 || c->tables > 1 || (pt_indices[i] >= c->pt_begin && pt_indices[i] < c->pt_end))
        last[pt_indices[i] - c->pt_begin] = i;
    std::vector<PtUpdate> pts;
    for (const auto& e : last) {
      pts.push_back(PtUpdate{e.first});
      pts.back().coeffs = coeffs + e.second * c->N;
    }
    if (pts.empty()) return PIRGPU_OK;
    quiesce(c);
    apply_update_tables(c, pts, nullptr, 0);
    return PIRGPU_OK;
  });
}

// ======================================================================================================================
// [6] C ABI: Galois keys and per-client key sets
// ======================================================================================================================
// The device buffer of key g in a slot: the one it has, a recycled one or a new one.
static uint64_t* key_buffer(pirgpu_ctx* c, uint32_t slot, uint32_t g) {
  const size_t words = (size_t)c->k * 2 * (c->k + 1) * c->N;
  auto& keys = c->keysets[slot].keys;
  uint64_t* dev = nullptr;
  auto it = keys.find(g);
  if (it != keys.end()) {
    // overwriting a key that queued work may still read: wait for it (never happens on the request path, where a
    // slot is emptied -- after a drain -- before it is refilled)
    HIP_TRY(hipStreamSynchronize(c->stream));
    sync_batch_streams(c);
    dev = it->second;
  } else {
    if (!c->key_pool.empty()) {
      dev = c->key_pool.back();
      c->key_pool.pop_back();
    } else {
      HIP_TRY(hipMalloc((void**)&dev, words * 8));
    }
    keys[g] = dev;
  }
  return dev;
}

// Uploads one Galois key into a key set slot (SEAL's NTT order at the boundary, device order in HBM).  A new client's
// first request pays for 12 of these (N = 4096): the staging buffer is allocated once per context and the key buffers
// of emptied sets are recycled, so the steady state of a server whose clients come and go allocates nothing.
static void upload_key(pirgpu_ctx* c, uint32_t slot, uint32_t g, const uint64_t* key, bool wait = true) {
  if (slot >= c->keysets.size()) throw Fail{PIRGPU_INVALID_ARGUMENT, "key set slot out of range"};
  if (!key || !(g & 1) || g >= 2 * c->N) throw Fail{PIRGPU_INVALID_ARGUMENT, "invalid Galois element"};
  const size_t words = (size_t)c->k * 2 * (c->k + 1) * c->N;
  uint64_t* dev = key_buffer(c, slot, g);
  if (!c->d_key_stage) c->d_key_stage = c->dalloc<uint64_t>(words);
  // stream order on the main stream covers the reuse of the staging buffer by the next key
  HIP_TRY(hipMemcpyAsync(c->d_key_stage, key, words * 8, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(launch_ntt_reorder(c->stream, c->N, c->d_key_stage, dev, (uint64_t)c->k * 2 * (c->k + 1), true,
                             c->mode != kNttInt));
  // the lanes / workers that will read the key do not follow this stream: the caller (or this call) waits once
  if (wait) HIP_TRY(hipStreamSynchronize(c->stream));
  ++c->key_uploads;
}

// Empties a slot; waits for everything in flight first (queued kernels may still read its keys).
static void clear_keyset(pirgpu_ctx* c, uint32_t slot) {
  KeySet& ks = c->keysets[slot];
  if (!ks.keys.empty()) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    sync_batch_streams(c);
    for (auto& kv : ks.keys) c->key_pool.push_back(kv.second);   // recycled by the next upload
    ks.keys.clear();
  }
  ks.blob.clear();
  ks.fingerprint = 0;
  if (slot) ks.gen = (ks.gen + 1) & ((1u << (32 - kSlotBits)) - 1);   // handles of the previous tenant go stale
}

static uint32_t slot_handle(const pirgpu_ctx* c, uint32_t index) { return index ? (c->keysets[index].gen << kSlotBits) | index : 0; }

// Handle -> slot index; FailedPrecondition for a handle whose set was evicted or released since it was handed out.
static uint32_t resolve_slot(pirgpu_ctx* c, uint32_t handle) {
  const uint32_t index = handle & kSlotMask;
  if (index >= c->keysets.size()) throw Fail{PIRGPU_INVALID_ARGUMENT, "key set slot out of range"};
  if (index && c->keysets[index].gen != handle >> kSlotBits)
    throw Fail{PIRGPU_FAILED_PRECONDITION, "stale key set handle: the set was evicted or released (claim it again)"};
  if (!index && handle) throw Fail{PIRGPU_INVALID_ARGUMENT, "key set slot out of range"};
  return index;
}

// cheap candidate filter before the byte-for-byte compare: length + 64 words sampled across the blob
static uint64_t blob_fingerprint(const uint8_t* blob, size_t len) {
  uint64_t h = 0xcbf29ce484222325ull ^ len;
  const size_t words = len / 8, step = std::max<size_t>(1, words / 64);
  for (size_t i = 0; i < words; i += step) {
    uint64_t w;
    memcpy(&w, blob + i * 8, 8);
    h = (h ^ w) * 0x100000001b3ull;
    h ^= h >> 29;
  }
  return h | 1;   // never 0 (0 = no blob)
}

int pirgpu_set_galois_key(pirgpu_ctx* c, uint32_t g, const uint64_t* key) {
  return guarded(c, [&]() -> int {
    c->keysets[0].blob.clear();
    c->keysets[0].fingerprint = 0;
    upload_key(c, 0, g, key);
    return PIRGPU_OK;
  });
}

int pirgpu_clear_galois_keys(pirgpu_ctx* c) {
  return guarded(c, [&]() -> int {
    clear_keyset(c, 0);
    return PIRGPU_OK;
  });
}

int pirgpu_set_keyset_capacity(pirgpu_ctx* c, uint32_t slots) {
  return guarded(c, [&]() -> int {
    if (slots < 1 || slots > 1024) return fail(c, PIRGPU_INVALID_ARGUMENT, "key set capacity must be in [1, 1024]");
    for (size_t i = (size_t)slots + 1; i < c->keysets.size(); ++i)
      if (c->keysets[i].pins) return fail(c, PIRGPU_FAILED_PRECONDITION, "a key set beyond the new capacity is in use by requests in flight");
    while (c->keysets.size() > (size_t)slots + 1) {   // shrinking drops the highest slots
      clear_keyset(c, (uint32_t)c->keysets.size() - 1);
      c->keysets.pop_back();
    }
    c->keyset_cap = slots;   // (a staged batch / selection that named a dropped slot fails its next run: stale handle)
    return PIRGPU_OK;
  });
}

int pirgpu_keyset_lookup(pirgpu_ctx* c, const uint8_t* blob, size_t len, int verify, uint32_t* slot) {
  return guarded(c, [&]() -> int {
    if (!slot || (!blob && len)) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    *slot = 0;
    if (!len) return PIRGPU_OK;
    const uint64_t fp = blob_fingerprint(blob, len);
    for (uint32_t i = 1; i < c->keysets.size(); ++i) {
      KeySet& ks = c->keysets[i];
      if (ks.fingerprint == fp && ks.blob.size() == len && (!verify || memcmp(ks.blob.data(), blob, len) == 0)) {
        ks.last_use = ++c->keyset_clock;
        *slot = slot_handle(c, i);
        break;
      }
    }
    return PIRGPU_OK;
  });
}

int pirgpu_keyset_verify(pirgpu_ctx* c, uint32_t slot, const uint8_t* blob, size_t len) {
  if (!c || !blob) return 0;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  const uint32_t index = slot & kSlotMask;
  if (index == 0 || index >= c->keysets.size() || c->keysets[index].gen != slot >> kSlotBits) return 0;
  const KeySet& ks = c->keysets[index];
  return ks.blob.size() == len && memcmp(ks.blob.data(), blob, len) == 0 ? 1 : 0;
}

size_t pirgpu_keyset_blob(pirgpu_ctx* c, uint32_t slot, const uint8_t** blob) {
  if (blob) *blob = nullptr;
  if (!c || !blob) return 0;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  const uint32_t index = slot & kSlotMask;
  if (index == 0 || index >= c->keysets.size() || c->keysets[index].gen != slot >> kSlotBits) return 0;
  *blob = c->keysets[index].blob.data();
  return c->keysets[index].blob.size();
}

int pirgpu_keyset_claim(pirgpu_ctx* c, const uint8_t* blob, size_t len, uint32_t* slot) {
  return guarded(c, [&]() -> int {
    if (!slot || (!blob && len)) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    uint32_t pick = 0;
    for (uint32_t i = 1; i < c->keysets.size() && !pick; ++i)
      if (c->keysets[i].keys.empty() && c->keysets[i].blob.empty() && !c->keysets[i].pins) pick = i;
    if (!pick && c->keysets.size() < (size_t)c->keyset_cap + 1) {
      c->keysets.emplace_back();
      pick = (uint32_t)c->keysets.size() - 1;
    }
    if (!pick) {   // least recently used -- never a set that requests in flight are pinned to.  (A staged batch or the
                   // single-query selection that still names the evicted set notices at its next run: its handle is stale.)
      uint64_t best = UINT64_MAX;
      for (uint32_t i = 1; i < c->keysets.size(); ++i)
        if (c->keysets[i].last_use < best && !c->keysets[i].pins) {
          best = c->keysets[i].last_use;
          pick = i;
        }
      if (!pick)
        return fail(c, PIRGPU_FAILED_PRECONDITION,
                    "every key set slot is in use by the requests being processed (pirgpu_set_keyset_capacity)");
      clear_keyset(c, pick);
      ++c->keyset_evictions;
    }
    KeySet& ks = c->keysets[pick];
    if (len) {
      ks.blob.assign(blob, blob + len);
      ks.fingerprint = blob_fingerprint(blob, len);
    }
    ks.last_use = ++c->keyset_clock;
    *slot = slot_handle(c, pick);
    return PIRGPU_OK;
  });
}

int pirgpu_keyset_release(pirgpu_ctx* c, uint32_t slot) {
  return guarded(c, [&]() -> int {
    const uint32_t index = resolve_slot(c, slot);
    if (index == 0) return fail(c, PIRGPU_INVALID_ARGUMENT, "key set slot out of range");
    if (c->keysets[index].pins) return fail(c, PIRGPU_FAILED_PRECONDITION, "the key set is in use by requests in flight");
    clear_keyset(c, index);
    return PIRGPU_OK;
  });
}

int pirgpu_keyset_set_key(pirgpu_ctx* c, uint32_t slot, uint32_t g, const uint64_t* key) {
  return guarded(c, [&]() -> int {
    upload_key(c, resolve_slot(c, slot), g, key);
    return PIRGPU_OK;
  });
}

int pirgpu_keyset_set_keys(pirgpu_ctx* c, uint32_t slot, uint32_t n, const uint32_t* galois_elts, const uint64_t* const* keys) {
  return guarded(c, [&]() -> int {
    if (n && (!galois_elts || !keys)) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    const uint32_t index = resolve_slot(c, slot);
    // one wait for the whole set (a new client's 12 keys: 12 stream synchronisations used to be a quarter of its
    // first request); the staging buffer's reuse from key to key is covered by stream order
    for (uint32_t i = 0; i < n; ++i) upload_key(c, index, galois_elts[i], keys[i], false);
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PIRGPU_OK;
  });
}

// ---- seed-compressed keys
constexpr size_t kSeedBytes = 64;
constexpr size_t kSeedStatWords = 2;
constexpr size_t kSeedStageBytes = 128u << 20;   // the stage holds as many keys as fit in this, at least 1, at most 16

// n_mod = k + 1: the key level; n_mod = k: the data level (compact queries, section 6.9), a prefix of the same walk
static SeedExpandArgs seed_expand_args(const pirgpu_ctx* c, bool key_level = true) {
  SeedExpandArgs a{};
  a.n_mod = key_level ? c->k + 1 : c->k;
  a.N = c->N;
  const uint64_t max_random = 0x7FFFFFFFFFFFFFFFull;
  for (uint32_t j = 0; j < a.n_mod; ++j) {
    a.mod[j] = c->hp.mod[j];
    a.max_multiple[j] = max_random - max_random % a.mod[j].q - 1;
  }
  // a prime below 2^61 accepts more than 7 draws of 8: four times the stream without rejections is never reached
  a.max_refills = 4 * ((uint64_t)a.n_mod * c->N / 512 + 1) + kSeedThreads / 64;
  return a;
}

static void ensure_seed_buffers(pirgpu_ctx* c, size_t n_seeds) {
  const size_t km = c->k + 1, key_words = (size_t)c->k * 2 * km * c->N;
  if (!c->d_seed_stats) {
    c->d_seed_stats = c->dalloc<uint64_t>(kSeedStatWords);
    HIP_TRY(hipMemsetAsync(c->d_seed_stats, 0, kSeedStatWords * 8, c->stream));
  }
  if (!c->d_seed_stage) {
    c->seed_stage_keys = std::min<size_t>(16, std::max<size_t>(1, kSeedStageBytes / (key_words * 8)));
    c->d_seed_stage = c->dalloc<uint64_t>(c->seed_stage_keys * key_words);
  }
  if (!c->h_seed_pin)
    HIP_TRY(hipHostMalloc((void**)&c->h_seed_pin, (key_words + kSeedStatWords) * 8, hipHostMallocDefault));   // 2 c0 halves = 1 key
  for (hipEvent_t& e : c->ev_seed_pin)
    if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  const size_t bytes = std::max<size_t>(n_seeds, 64) * kSeedBytes;
  if (bytes > c->d_seeds_cap) {     // nothing of an earlier call is in flight: every call ends with a wait
    if (c->d_seeds) HIP_TRY(hipFree(c->d_seeds));
    c->d_seeds = nullptr;
    c->d_seeds_cap = 0;
    HIP_TRY(hipMalloc((void**)&c->d_seeds, bytes));
    c->d_seeds_cap = bytes;
  }
  if (bytes > c->h_seeds_cap) {
    if (c->h_seeds) HIP_TRY(hipHostFree(c->h_seeds));
    c->h_seeds = nullptr;
    c->h_seeds_cap = 0;
    HIP_TRY(hipHostMalloc((void**)&c->h_seeds, bytes, hipHostMallocDefault));
    c->h_seeds_cap = bytes;
  }
}

// the kernel's counters after the stream has been waited for: an overrun is an error (and is cleared)
static void check_seed_overrun(pirgpu_ctx* c) {
  const uint64_t* st = c->h_seed_pin + (size_t)c->k * 2 * (c->k + 1) * c->N;
  if (st[1]) {
    HIP_TRY(hipMemsetAsync(c->d_seed_stats + 1, 0, 8, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    throw Fail{PIRGPU_INTERNAL, "seed expansion ran past its stream bound"};
  }
}

int pirgpu_keyset_set_keys_seeded(pirgpu_ctx* c, uint32_t slot, uint32_t n, const uint32_t* galois_elts,
                                  const void* const* c0, const uint8_t* const* seeds) {
  return guarded(c, [&]() -> int {
    if (n && (!galois_elts || !c0 || !seeds)) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    const uint32_t index = resolve_slot(c, slot);
    for (uint32_t i = 0; i < n; ++i)
      if (!c0[i] || !seeds[i] || !(galois_elts[i] & 1) || galois_elts[i] >= 2 * c->N)
        return fail(c, PIRGPU_INVALID_ARGUMENT, "invalid Galois element");
    if (!n) return PIRGPU_OK;
    const uint32_t k = c->k, km = k + 1;
    const size_t poly_words = (size_t)km * c->N, half_words = (size_t)k * poly_words, key_words = 2 * half_words;
    ensure_seed_buffers(c, (size_t)n * k);
    const SeedExpandArgs args = seed_expand_args(c);
    for (uint32_t i = 0; i < n; ++i) memcpy(c->h_seeds + (size_t)i * k * kSeedBytes, seeds[i], k * kSeedBytes);
    HIP_TRY(hipMemcpyAsync(c->d_seeds, c->h_seeds, (size_t)n * k * kSeedBytes, hipMemcpyHostToDevice, c->stream));
    bool pin_used[2] = {false, false};
    for (uint32_t g0 = 0; g0 < n; g0 += (uint32_t)c->seed_stage_keys) {
      const uint32_t ng = std::min<uint32_t>((uint32_t)c->seed_stage_keys, n - g0);
      // component 1 of every object of the group: object (key i, digit j) -> stage[i][j][1]; the stage's reuse from
      // group to group is covered by stream order
      HIP_TRY(launch_seed_expand(c->stream, args, c->d_seeds + (size_t)g0 * k * kSeedBytes, ng * k,
                                 c->d_seed_stage + poly_words, 2 * poly_words, c->d_seed_stats));
      for (uint32_t i = g0; i < g0 + ng; ++i) {
        const uint32_t h = i & 1;
        uint64_t* pin = c->h_seed_pin + h * half_words;
        if (pin_used[h]) HIP_TRY(hipEventSynchronize(c->ev_seed_pin[h]));   // the copy of key i - 2 has left this half
        memcpy(pin, c0[i], half_words * 8);
        uint64_t* stage = c->d_seed_stage + (size_t)(i - g0) * key_words;
        // c0 [k][km][N] -> component 0 of [k][2][km][N]
        HIP_TRY(hipMemcpy2DAsync(stage, 2 * poly_words * 8, pin, poly_words * 8, poly_words * 8, k, hipMemcpyHostToDevice,
                                 c->stream));
        HIP_TRY(hipEventRecord(c->ev_seed_pin[h], c->stream));
        pin_used[h] = true;
        uint64_t* dev = key_buffer(c, index, galois_elts[i]);
        HIP_TRY(launch_ntt_reorder(c->stream, c->N, stage, dev, (uint64_t)k * 2 * km, true, c->mode != kNttInt));
        ++c->key_uploads;
      }
    }
    c->seed_objects += (uint64_t)n * k;
    HIP_TRY(hipMemcpyAsync(c->h_seed_pin + key_words, c->d_seed_stats, kSeedStatWords * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));   // the one wait of the call
    check_seed_overrun(c);
    return PIRGPU_OK;
  });
}

int pirgpu_expand_seeds(pirgpu_ctx* c, const uint8_t* seeds, uint32_t n, uint64_t* out) {
  return guarded(c, [&]() -> int {
    if (n && (!seeds || !out)) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    if (!n) return PIRGPU_OK;
    const size_t poly_words = (size_t)(c->k + 1) * c->N;
    ensure_seed_buffers(c, n);
    DevScratch buf;
    uint64_t* d_out = buf.get<uint64_t>((size_t)n * poly_words * 8);
    HIP_TRY(hipMemcpyAsync(c->d_seeds, seeds, (size_t)n * kSeedBytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_seed_expand(c->stream, seed_expand_args(c), c->d_seeds, n, d_out, poly_words, c->d_seed_stats));
    c->seed_objects += n;
    HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)n * poly_words * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_seed_pin + (size_t)c->k * 2 * poly_words, c->d_seed_stats, kSeedStatWords * 8,
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    check_seed_overrun(c);
    return PIRGPU_OK;
  });
}

int pirgpu_keyset_seed_stats(pirgpu_ctx* c, uint64_t stats[2]) {
  return guarded(c, [&]() -> int {
    if (!stats) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    stats[0] = c->seed_objects;
    stats[1] = 0;
    if (c->d_seed_stats) {
      HIP_TRY(hipStreamSynchronize(c->stream));
      HIP_TRY(hipMemcpy(&stats[1], c->d_seed_stats, 8, hipMemcpyDeviceToHost));
    }
    return PIRGPU_OK;
  });
}

int pirgpu_keyset_pin(pirgpu_ctx* c, uint32_t slot) {
  return guarded(c, [&]() -> int {
    const uint32_t index = resolve_slot(c, slot);
    if (index) ++c->keysets[index].pins;
    return PIRGPU_OK;
  });
}

int pirgpu_keyset_unpin(pirgpu_ctx* c, uint32_t slot) {
  if (!c) return PIRGPU_INVALID_ARGUMENT;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  const uint32_t index = slot & kSlotMask;   // a pinned set cannot have changed generation
  if (index && index < c->keysets.size() && c->keysets[index].pins) --c->keysets[index].pins;
  return PIRGPU_OK;
}

// The single-query selection as a handle: the generation it was SELECTED with (not the slot's current one -- a selection
// that went stale must stay stale), 0 for the default set.
uint32_t pirgpu_current_keyset(pirgpu_ctx* c) {
  if (!c) return 0;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  return c->cur_keyset ? (c->cur_keyset_gen << kSlotBits) | (c->cur_keyset & kSlotMask) : 0;
}

// wire layer: the selection saved and put back exactly as it was (index, generation), valid or not
void pirgpu_keyset_selection_get(pirgpu_ctx* c, uint32_t sel[2]) {
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  sel[0] = c->cur_keyset;
  sel[1] = c->cur_keyset_gen;
}
void pirgpu_keyset_selection_set(pirgpu_ctx* c, const uint32_t sel[2]) {
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  c->cur_keyset = sel[0];
  c->cur_keyset_gen = sel[1];
}

int pirgpu_query_use_keyset(pirgpu_ctx* c, uint32_t slot) {
  return guarded(c, [&]() -> int {
    const uint32_t index = resolve_slot(c, slot);
    c->cur_keyset = index;
    c->cur_keyset_gen = c->keysets[index].gen;
    c->keysets[index].last_use = ++c->keyset_clock;
    return PIRGPU_OK;
  });
}

int pirgpu_batch_set_keysets(pirgpu_ctx* c, const uint32_t* slots, uint32_t count) {
  return guarded(c, [&]() -> int {
    if (!slots || count != c->bs().staged_count) return fail(c, PIRGPU_INVALID_ARGUMENT, "one key set slot per staged query");
    std::vector<uint32_t> idx(count);
    for (uint32_t i = 0; i < count; ++i) idx[i] = resolve_slot(c, slots[i]);
    ++c->keyset_clock;
    std::vector<uint32_t> gens(count);
    for (uint32_t i = 0; i < count; ++i) {
      c->keysets[idx[i]].last_use = c->keyset_clock;
      gens[i] = c->keysets[idx[i]].gen;
    }
    c->bs().batch_keysets = std::move(idx);
    c->bs().batch_keyset_gens = std::move(gens);
    return PIRGPU_OK;
  });
}

uint32_t pirgpu_tables(const pirgpu_ctx* c) { return c ? c->tables : 0; }

uint64_t pirgpu_table_zero_plaintexts(const pirgpu_ctx* cc, uint32_t table) {
  pirgpu_ctx* c = const_cast<pirgpu_ctx*>(cc);
  if (!c) return 0;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  if (table >= c->tables) return 0;
  return c->tables > 1 ? c->tbl_zero[table] : c->zero_pts;
}

int pirgpu_query_use_table(pirgpu_ctx* c, uint32_t table) {
  return guarded(c, [&]() -> int {
    if (table >= c->tables)
      return fail(c, PIRGPU_INVALID_ARGUMENT, "table " + std::to_string(table) + " out of range (tables = " +
                                                  std::to_string(c->tables) + ")");
    c->cur_table = table;
    return PIRGPU_OK;
  });
}

// wire layer: the selection read and put back around a request (like pirgpu_keyset_selection_get / _set)
uint32_t pirgpu_current_table(pirgpu_ctx* c) {
  if (!c) return 0;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  return c->cur_table;
}

int pirgpu_batch_set_tables(pirgpu_ctx* c, const uint32_t* tables, uint32_t count) {
  return guarded(c, [&]() -> int {
    if (!tables || count != c->bs().staged_count) return fail(c, PIRGPU_INVALID_ARGUMENT, "one table per staged query");
    for (uint32_t i = 0; i < count; ++i)
      if (tables[i] >= c->tables)
        return fail(c, PIRGPU_INVALID_ARGUMENT, "table " + std::to_string(tables[i]) + " of query " + std::to_string(i) +
                                                    " out of range (tables = " + std::to_string(c->tables) + ")");
    c->bs().batch_tables.assign(tables, tables + count);
    return PIRGPU_OK;
  });
}

// Test hook, no context and no device: the order and the runs the batch pipeline forms for these tables with groups of
// `group` queries (plan_table_runs).  order[count]; run_begin[count + 1], of which *n_runs + 1 entries are written.
int pirgpu_plan_table_runs(const uint32_t* tables, uint32_t count, uint32_t group, uint32_t* order, uint32_t* run_begin,
                           uint32_t* n_runs) {
  if ((!tables && count) || !order || !run_begin || !n_runs || group == 0) return PIRGPU_INVALID_ARGUMENT;
  const TablePlan tp = plan_table_runs(tables, count, group);
  std::copy(tp.order.begin(), tp.order.end(), order);
  std::copy(tp.run_begin.begin(), tp.run_begin.end(), run_begin);
  *n_runs = (uint32_t)tp.run_begin.size() - 1;
  return PIRGPU_OK;
}

int pirgpu_keyset_stats(pirgpu_ctx* c, uint64_t stats[4]) {
  return guarded(c, [&]() -> int {
    if (!stats) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    uint64_t resident = 0;
    for (uint32_t i = 1; i < c->keysets.size(); ++i) resident += c->keysets[i].keys.empty() ? 0 : 1;
    stats[0] = resident;
    stats[1] = c->key_uploads;
    stats[2] = c->keyset_evictions;
    stats[3] = c->keyset_cap;
    return PIRGPU_OK;
  });
}

int pirgpu_batch_select(pirgpu_ctx* c, uint32_t which) {
  if (!c || which >= (uint32_t)kBatchSets) return PIRGPU_INVALID_ARGUMENT;
  t_batch_set = (int)which;
  return PIRGPU_OK;
}

// Pinned host staging owned by the context (the wire layer parses queries straight into it and serialises replies
// straight out of it: H2D / D2H then run at link speed and asynchronously instead of through pageable bounce buffers).
static uint64_t* host_buffer(pirgpu_ctx* c, uint64_t*& buf, size_t& cap, size_t words) {
  if (words > cap) {
    if (buf) {
      HIP_TRY(hipStreamSynchronize(c->stream));
      HIP_TRY(hipHostFree(buf));
      buf = nullptr;
      cap = 0;
    }
    HIP_TRY(hipHostMalloc((void**)&buf, words * 8, hipHostMallocDefault));
    cap = words;
  }
  return buf;
}

uint64_t* pirgpu_host_query_buffer(pirgpu_ctx* c, uint32_t count) {
  uint64_t* out = nullptr;
  (void)guarded(c, [&]() -> int {
    out = host_buffer(c, c->bs().h_query, c->bs().h_query_words, (size_t)std::max<uint32_t>(count, 1) * (c->dim_sum / c->N + 1) * c->ctw);
    return PIRGPU_OK;
  });
  return out;
}

uint64_t* pirgpu_host_reply_buffer(pirgpu_ctx* c, uint32_t count) {
  uint64_t* out = nullptr;
  (void)guarded(c, [&]() -> int {
    out = host_buffer(c, c->bs().h_reply, c->bs().h_reply_words, (size_t)std::max<uint32_t>(count, 1) * c->reply_cts * c->rctw);
    return PIRGPU_OK;
  });
  return out;
}

// ======================================================================================================================
// [7] C ABI: single query (stage / run / fetch), stream ordering hooks (join / fork), test hooks (expand, substitute, multiply)
// ======================================================================================================================
static int query_stage_impl(pirgpu_ctx* c, const uint64_t* query, uint32_t nq, bool wait) {
  return guarded(c, [&]() -> int {
    ensure_workspace(c);
    Worker& w = c->workers[0];
    if (!query || nq != c->dim_sum / c->N + 1)  // reference server.cpp:154-158
      return fail(c, PIRGPU_INVALID_ARGUMENT,
                  "Number of ciphertexts doesn't match number of items for oblivious expansion.");
    HIP_TRY(hipStreamWaitEvent(c->stream, w.ev_done, 0));
    HIP_TRY(hipMemcpyAsync(w.d_query, query, (size_t)nq * c->ctw * 8, hipMemcpyHostToDevice, c->stream));
    if (wait) HIP_TRY(hipStreamSynchronize(c->stream));   // the caller may reuse `query` at once
    w.staged_nq = nq;
    return PIRGPU_OK;
  });
}

int pirgpu_query_stage(pirgpu_ctx* c, const uint64_t* query, uint32_t nq) { return query_stage_impl(c, query, nq, true); }

int pirgpu_query_stage_async(pirgpu_ctx* c, const uint64_t* pinned_query, uint32_t nq) {
  return query_stage_impl(c, pinned_query, nq, false);
}

int pirgpu_query_run(pirgpu_ctx* c) {
  return guarded(c, [&]() -> int {
    ensure_workspace(c);
    run_staged(c, c->workers[0], true);
    return PIRGPU_OK;
  });
}

int pirgpu_sync(pirgpu_ctx* c) {
  return guarded(c, [&]() -> int {
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (BatchLane& ln : c->lanes)
      if (ln.stream) HIP_TRY(hipStreamSynchronize(ln.stream));
    for (Worker& w : c->workers)
      if (w.stream) HIP_TRY(hipStreamSynchronize(w.stream));
    if (c->copy_stream) HIP_TRY(hipStreamSynchronize(c->copy_stream));
    return PIRGPU_OK;
  });
}

// ---- device-side ordering with the caller's streams (pipelined multi-GPU step) ----
//
// The library queues its work on its own HIP streams (one main stream, the batch lanes, the workers).  A caller that
// runs collectives on ITS streams orders them against that work without stopping the host: pirgpu_join makes the main
// stream wait -- on the device -- for everything queued on the lanes and workers so far, so the main stream (handed
// out by pirgpu_stream_handle, e.g. for torch.cuda.ExternalStream) becomes the completion point an event can be
// recorded on; pirgpu_fork makes the lanes and workers wait for everything the main stream has been made to wait for
// (e.g. an event of the caller's collective), so work queued afterwards starts behind it.

void* pirgpu_stream_handle(pirgpu_ctx* c) { return c ? (void*)c->stream : nullptr; }

int pirgpu_join(pirgpu_ctx* c) { return pirgpu_join_stream(c, nullptr); }

int pirgpu_device_synchronize(pirgpu_ctx* c) {
  return guarded(c, [&]() -> int {
    c->use_device();
    HIP_TRY(hipDeviceSynchronize());
    return PIRGPU_OK;
  });
}

int pirgpu_join_stream(pirgpu_ctx* c, void* stream) {
  return guarded(c, [&]() -> int {
    hipStream_t target = stream ? (hipStream_t)stream : c->stream;
    for (BatchLane& ln : c->lanes) {
      if (!ln.stream) continue;
      if (!ln.ev_join) HIP_TRY(hipEventCreateWithFlags(&ln.ev_join, hipEventDisableTiming));
      HIP_TRY(hipEventRecord(ln.ev_join, ln.stream));
      HIP_TRY(hipStreamWaitEvent(target, ln.ev_join, 0));
    }
    for (Worker& w : c->workers) {
      if (!w.stream || w.stream == c->stream) continue;
      if (!w.ev_join) HIP_TRY(hipEventCreateWithFlags(&w.ev_join, hipEventDisableTiming));
      HIP_TRY(hipEventRecord(w.ev_join, w.stream));
      HIP_TRY(hipStreamWaitEvent(target, w.ev_join, 0));
    }
    if (target != c->stream) {   // the main stream carries work too (worker 0, copies): the target follows it as well
      if (!c->ev_main_join) HIP_TRY(hipEventCreateWithFlags(&c->ev_main_join, hipEventDisableTiming));
      HIP_TRY(hipEventRecord(c->ev_main_join, c->stream));
      HIP_TRY(hipStreamWaitEvent(target, c->ev_main_join, 0));
    }
    return PIRGPU_OK;
  });
}

int pirgpu_batch_set_reply_buffer(pirgpu_ctx* c, uint64_t* device_buf, uint64_t cap) {
  return guarded(c, [&]() -> int {
    if (c->in_batch) return fail(c, PIRGPU_FAILED_PRECONDITION, "a batch is being queued");
    if (device_buf && cap == 0) return fail(c, PIRGPU_INVALID_ARGUMENT, "empty reply buffer");
    c->bs().ext_reply = device_buf;
    c->bs().ext_reply_cts = device_buf ? cap : 0;
    c->bs().batch_valid = false;   // replies of an earlier batch live in the other buffer
    return PIRGPU_OK;
  });
}

int pirgpu_batch_set_host_replies(pirgpu_ctx* c, uint64_t* pinned_host, uint64_t cap) {
  return guarded(c, [&]() -> int {
    if (c->in_batch) return fail(c, PIRGPU_FAILED_PRECONDITION, "a batch is being queued");
    c->bs().host_reply = pinned_host;
    c->bs().host_reply_cts = pinned_host ? cap : 0;
    c->bs().host_reply_done = false;
    return PIRGPU_OK;
  });
}

int pirgpu_batch_next_host_replies(pirgpu_ctx* c, uint32_t* ready) {
  if (!c || !ready) return PIRGPU_INVALID_ARGUMENT;
  // the wait itself happens WITHOUT the context's lock held by this call (the caller may hold it recursively anyway)
  hipEvent_t ev = nullptr;
  uint32_t end = 0;
  int rc = guarded(c, [&]() -> int {
    if (!c->bs().host_reply_done) return fail(c, PIRGPU_FAILED_PRECONDITION, "the last batch did not download its replies group by group");
    if (c->bs().dl_next >= c->bs().dl_end.size()) {
      *ready = c->bs().dl_end.empty() ? 0 : c->bs().dl_end.back();
      return PIRGPU_OK;
    }
    ev = c->bs().dl_events[c->bs().dl_next];
    end = c->bs().dl_end[c->bs().dl_next];
    ++c->bs().dl_next;
    return PIRGPU_OK;
  });
  if (rc || !ev) return rc;
  if (hipEventSynchronize(ev) != hipSuccess) return fail(c, PIRGPU_INTERNAL, "waiting for a group's replies failed");
  *ready = end;
  return PIRGPU_OK;
}

int pirgpu_fork(pirgpu_ctx* c) {
  return guarded(c, [&]() -> int {
    if (!c->ev_fork) HIP_TRY(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(c->ev_fork, c->stream));
    for (BatchLane& ln : c->lanes)
      if (ln.stream) HIP_TRY(hipStreamWaitEvent(ln.stream, c->ev_fork, 0));
    if (c->head_stream) HIP_TRY(hipStreamWaitEvent(c->head_stream, c->ev_fork, 0));
    for (Worker& w : c->workers)
      if (w.stream && w.stream != c->stream) HIP_TRY(hipStreamWaitEvent(w.stream, c->ev_fork, 0));
    return PIRGPU_OK;
  });
}

int pirgpu_query_fetch(pirgpu_ctx* c, uint64_t* reply, uint64_t cap, uint64_t* count) {
  return guarded(c, [&]() -> int {
    if (c->workers.empty()) return fail(c, PIRGPU_FAILED_PRECONDITION, "no query has been run");
    Worker& w = c->workers[0];
    if (!w.reply_valid) return fail(c, PIRGPU_FAILED_PRECONDITION, "no query has been run");
    if (!reply || cap < c->reply_cts) return fail(c, PIRGPU_INVALID_ARGUMENT, "reply buffer too small");
    HIP_TRY(hipMemcpyAsync(reply, w.lvl[0], c->reply_cts * c->rctw * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (count) *count = c->reply_cts;
    return PIRGPU_OK;
  });
}

// pirgpu_query_fetch in two halves: both downloads are queued at once, the caller serialises the first half of the
// reply while the second is still crossing PCIe (a megabyte of memcpy against 20 us of transfer: the tail of a lone
// request).  fetch_begin returns the number of ciphertexts in the first part; fetch_wait(part) blocks until that part has
// landed in `reply` (pinned host memory).
int pirgpu_query_fetch_begin(pirgpu_ctx* c, uint64_t* reply, uint64_t cap, uint64_t* count, uint64_t* first_part) {
  return guarded(c, [&]() -> int {
    if (c->workers.empty()) return fail(c, PIRGPU_FAILED_PRECONDITION, "no query has been run");
    Worker& w = c->workers[0];
    if (!w.reply_valid) return fail(c, PIRGPU_FAILED_PRECONDITION, "no query has been run");
    if (!reply || cap < c->reply_cts) return fail(c, PIRGPU_INVALID_ARGUMENT, "reply buffer too small");
    for (hipEvent_t& e : c->ev_fetch)
      if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    const uint64_t a = (c->reply_cts + 1) / 2;
    HIP_TRY(hipMemcpyAsync(reply, w.lvl[0], a * c->rctw * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipEventRecord(c->ev_fetch[0], c->stream));
    if (c->reply_cts > a)
      HIP_TRY(hipMemcpyAsync(reply + a * c->rctw, w.lvl[0] + a * c->rctw, (c->reply_cts - a) * c->rctw * 8, hipMemcpyDeviceToHost,
                             c->stream));
    HIP_TRY(hipEventRecord(c->ev_fetch[1], c->stream));
    if (count) *count = c->reply_cts;
    if (first_part) *first_part = a;
    return PIRGPU_OK;
  });
}

int pirgpu_query_fetch_wait(pirgpu_ctx* c, int part) {
  if (!c || part < 0 || part > 1 || !c->ev_fetch[part]) return PIRGPU_INVALID_ARGUMENT;
  if (hipEventSynchronize(c->ev_fetch[part]) != hipSuccess) return fail(c, PIRGPU_INTERNAL, "waiting for the reply failed");
  return PIRGPU_OK;
}

int pirgpu_process_query(pirgpu_ctx* c, const uint64_t* query, uint32_t nq, uint64_t* reply, uint64_t cap,
                         uint64_t* count) {
  int rc = pirgpu_query_stage(c, query, nq);
  if (rc) return rc;
  rc = pirgpu_query_run(c);
  if (rc) return rc;
  return pirgpu_query_fetch(c, reply, cap, count);
}

uint64_t* pirgpu_reply_device_ptr(pirgpu_ctx* c) { return (c && c->ws_ready) ? c->workers[0].lvl[0] : nullptr; }

int pirgpu_reply_copy_to_device(pirgpu_ctx* c, uint64_t* dst, uint64_t cap) {
  return guarded(c, [&]() -> int {
    refuse_switched(c);
    refuse_packed(c);
    refuse_ctm(c);
    if (c->workers.empty()) return fail(c, PIRGPU_FAILED_PRECONDITION, "no query has been run");
    Worker& w = c->workers[0];
    if (!w.reply_valid) return fail(c, PIRGPU_FAILED_PRECONDITION, "no query has been run");
    if (!dst || cap < c->reply_cts) return fail(c, PIRGPU_INVALID_ARGUMENT, "reply buffer too small");
    HIP_TRY(hipMemcpyAsync(dst, w.lvl[0], c->reply_cts * c->rctw * 8, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PIRGPU_OK;
  });
}

int pirgpu_expand(pirgpu_ctx* c, const uint64_t* ct, uint32_t num_items, uint64_t* out) {
  return guarded(c, [&]() -> int {
    ensure_workspace(c);
    Worker& w = c->workers[0];
    if (!ct || (!out && num_items)) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    if (num_items > c->N)
      return fail(c, PIRGPU_INVALID_ARGUMENT, "Cannot expand more items from a CT than poly modulus degree");
    // the shared workspace is sized for this context's dim_sum
    const uint64_t m_max = std::min<uint64_t>(c->N, hm::next_power_two(std::max<uint32_t>(c->dim_sum, 1)));
    if (hm::next_power_two(num_items) > m_max)
      return fail(c, PIRGPU_INVALID_ARGUMENT, "num_items exceeds this context's expansion workspace");
    w.keyset = current_keyset(c);
    HIP_TRY(hipMemcpyAsync(w.res_b, ct, c->ctw * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_tree_convert(c->stream, c->dp, c->mode, w.res_b, w.res_a, c->ctw, true));
    uint64_t* res = expand_on_device(c, w, num_items);
    if (num_items) {  // tree element type -> canonical residues (in place), then out
      HIP_TRY(launch_tree_convert(c->stream, c->dp, c->mode, res, res, (uint64_t)num_items * c->ctw, false));
      HIP_TRY(hipMemcpyAsync(out, res, (size_t)num_items * c->ctw * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PIRGPU_OK;
  });
}

int pirgpu_expand_multi(pirgpu_ctx* c, const uint64_t* cts, uint32_t num_cts, uint64_t total_items, uint64_t* out) {
  return guarded(c, [&]() -> int {
    ensure_workspace(c);
    Worker& w = c->workers[0];
    if (!cts || !out) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    if (num_cts != total_items / c->N + 1)  // reference server.cpp:154-158
      return fail(c, PIRGPU_INVALID_ARGUMENT,
                  "Number of ciphertexts doesn't match number of items for oblivious expansion.");
    const uint64_t m_max = std::min<uint64_t>(c->N, hm::next_power_two(std::max<uint32_t>(c->dim_sum, 1)));
    uint64_t remaining = total_items, produced = 0;
    w.keyset = current_keyset(c);
    for (uint32_t q = 0; q < num_cts && remaining; ++q) {
      uint32_t n = (uint32_t)std::min<uint64_t>(remaining, c->N);
      if (hm::next_power_two(n) > m_max)
        return fail(c, PIRGPU_INVALID_ARGUMENT, "total_items exceeds this context's expansion workspace");
      HIP_TRY(hipMemcpyAsync(w.res_b, cts + (size_t)q * c->ctw, c->ctw * 8, hipMemcpyHostToDevice, c->stream));
      HIP_TRY(launch_tree_convert(c->stream, c->dp, c->mode, w.res_b, w.res_a, c->ctw, true));
      uint64_t* res = expand_on_device(c, w, n);
      HIP_TRY(launch_tree_convert(c->stream, c->dp, c->mode, res, res, (uint64_t)n * c->ctw, false));
      HIP_TRY(hipMemcpyAsync(out + produced * c->ctw, res, (size_t)n * c->ctw * 8, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      produced += n;
      remaining -= n;
    }
    return PIRGPU_OK;
  });
}

int pirgpu_substitute_power_x(pirgpu_ctx* c, uint64_t* ct, uint32_t power) {
  return guarded(c, [&]() -> int {
    ensure_workspace(c);
    Worker& w = c->workers[0];
    if (!ct) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    if (!(power & 1) || power >= 2 * c->N)  // SEAL: "Galois element is not valid" -> InternalError
      return fail(c, PIRGPU_INTERNAL, "Galois element is not valid");
    KeyPtrs key{};
    key.p[0] = find_key(c, current_keyset(c), power);
    key.B = 1;
    HIP_TRY(hipMemcpyAsync(w.res_b, ct, c->ctw * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_tree_convert(c->stream, c->dp, c->mode, w.res_b, w.res_a, c->ctw, true));
    HIP_TRY(c->ops->ks_digit(c->stream, c->mode, c->dp, c->k, w.res_a, power, 1, w.dig, c->pack40, nullptr, false, false));
    HIP_TRY(c->ops->ks_mac_intt(c->stream, c->mode, c->dp, c->k, w.dig, key, 1, w.prod, c->pack40, 0, c->k + 1));
    HIP_TRY(launch_ks_combine(c->stream, c->dp, c->mode, c->N, c->k, w.res_a, w.prod, galois_inverse(power, c->N), 1, 0,
                              false, /*hi_limit: unused without the expand step*/ 0, c->pack40, w.res_b, c->pack_bytes));
    HIP_TRY(launch_tree_convert(c->stream, c->dp, c->mode, w.res_b, w.res_b, c->ctw, false));
    HIP_TRY(hipMemcpyAsync(ct, w.res_b, c->ctw * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PIRGPU_OK;
  });
}

int pirgpu_multiply_inverse_power_of_x(pirgpu_ctx* c, const uint64_t* ct, uint32_t kpow, uint64_t* out) {
  return guarded(c, [&]() -> int {
    ensure_workspace(c);
    Worker& w = c->workers[0];
    if (!ct || !out) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    const uint32_t twoN = 2 * c->N;
    const uint32_t index = (twoN - (kpow % twoN)) % twoN;  // reference server.cpp:87-88
    HIP_TRY(hipMemcpyAsync(w.res_a, ct, c->ctw * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_monomial_shift(c->stream, c->dp, c->N, c->k, w.res_a, index, 1, w.res_b));
    HIP_TRY(hipMemcpyAsync(out, w.res_b, c->ctw * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PIRGPU_OK;
  });
}

int pirgpu_multiply(pirgpu_ctx* c, const uint64_t* sv, uint64_t sv_count, uint64_t* reply, uint64_t cap,
                    uint64_t* count) {
  return guarded(c, [&]() -> int {
    ensure_workspace(c);
    Worker& w = c->workers[0];
    if (sv_count != c->dim_sum)  // reference database.cpp:297-300
      return fail(c, PIRGPU_INVALID_ARGUMENT, "Selection vector size does not match dimensions");
    if (!sv || !reply || cap < c->reply_cts) return fail(c, PIRGPU_INVALID_ARGUMENT, "reply buffer too small");
    // stage the coefficient-form selectors through res_a in workspace-sized pieces
    const uint64_t m_max = std::min<uint64_t>(c->N, hm::next_power_two(std::max<uint32_t>(c->dim_sum, 1)));
    for (uint64_t s = 0; s < sv_count; s += m_max) {
      const uint64_t n = std::min<uint64_t>(m_max, sv_count - s);
      HIP_TRY(hipMemcpyAsync(w.res_a, sv + s * c->ctw, n * c->ctw * 8, hipMemcpyHostToDevice, c->stream));
      HIP_TRY(c->ops->ct_ntt_fwd_oop(c->stream, c->mode, c->dp, c->k, w.res_a, w.sv_ntt + s * c->ctw, n, false));
      HIP_TRY(hipStreamSynchronize(c->stream));
    }
    c->prof_cur = -1;
    w.sv_cur = nullptr;
    w.sv_rows = nullptr;
    w.table = c->cur_table;
    w.keyset = current_keyset(c);
    multiply_on_device(c, w);
    HIP_TRY(hipMemcpyAsync(reply, w.lvl[0], c->reply_cts * c->rctw * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (count) *count = c->reply_cts;
    return PIRGPU_OK;
  });
}

// ======================================================================================================================
// [8] BATCH PIPELINE (server.cpp:60-63): staging, lanes, grouped expansion, batch_run_mfma
// ======================================================================================================================
// ---- batch mode: `count` independent queries, spread round-robin over the workers ----

int pirgpu_set_concurrency(pirgpu_ctx* c, uint32_t n_workers) {
  return guarded(c, [&]() -> int {
    if (n_workers < 1 || n_workers > 32) return fail(c, PIRGPU_INVALID_ARGUMENT, "workers must be in [1, 32]");
    ensure_workspace(c);
    while (c->workers.size() < n_workers) {
      c->workers.emplace_back();
      alloc_worker(c, c->workers.back());
    }
    c->n_active = n_workers;
    return PIRGPU_OK;
  });
}

static void ensure_batch_capacity(pirgpu_ctx* c, uint32_t count);
// Where a batch's replies are written and read: the context's own buffer, or the caller's (pirgpu_batch_set_reply_buffer).
static inline uint64_t* reply_base(pirgpu_ctx* c) { return c->bs().ext_reply ? c->bs().ext_reply : c->bs().d_breply; }
static void check_reply_target(pirgpu_ctx* c, uint64_t count) {
  if (c->bs().ext_reply && count * c->reply_cts > c->bs().ext_reply_cts)
    throw Fail{PIRGPU_INVALID_ARGUMENT, "the caller's reply buffer (pirgpu_batch_set_reply_buffer) is too small for this batch"};
}

static int batch_stage_impl(pirgpu_ctx* c, const uint64_t* queries, uint32_t nq, uint32_t count, bool async) {
  return guarded(c, [&]() -> int {
    ensure_workspace(c);
    if (!queries || nq != c->dim_sum / c->N + 1)  // reference server.cpp:154-158
      return fail(c, PIRGPU_INVALID_ARGUMENT,
                  "Number of ciphertexts doesn't match number of items for oblivious expansion.");
    if (count == 0 || count > 4096) return fail(c, PIRGPU_INVALID_ARGUMENT, "batch size must be in [1, 4096]");
    ensure_batch_capacity(c, count);
    BatchSet& b = c->bs();
    const size_t qwords = (size_t)nq * c->ctw;
    // head-stream work queued earlier may still import queries of this set's previous batch: uploads go behind it
    if (c->ev_head_tail) HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_head_tail, 0));
    if (async) {
      // pieces of kStagePiece queries, one event each: the first group starts as soon as ITS queries are on the device
      const uint32_t pieces = (count + kStagePiece - 1) / kStagePiece;
      while (b.st_events.size() < pieces) {
        hipEvent_t e;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        b.st_events.push_back(e);
      }
      for (uint32_t p = 0; p < pieces; ++p) {
        const uint32_t q0 = p * kStagePiece, n = std::min<uint32_t>(kStagePiece, count - q0);
        HIP_TRY(hipMemcpyAsync(b.d_bquery + (size_t)q0 * qwords, queries + (size_t)q0 * qwords, (size_t)n * qwords * 8,
                               hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipEventRecord(b.st_events[p], c->stream));
      }
      b.st_pieces = pieces;
    } else {
      HIP_TRY(hipMemcpyAsync(b.d_bquery, queries, (size_t)count * qwords * 8, hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      b.st_pieces = 0;
    }
    b.batch_count = count;
    b.staged_count = count;
    b.batch_keysets.assign(count, 0);   // pirgpu_batch_set_keysets assigns other clients' key sets
    b.batch_keyset_gens.assign(count, 0);
    b.batch_tables.clear();             // pirgpu_batch_set_tables names other tables than the selected one
    b.batch_valid = false;
    return PIRGPU_OK;
  });
}

int pirgpu_batch_stage(pirgpu_ctx* c, const uint64_t* queries, uint32_t nq, uint32_t count) {
  return batch_stage_impl(c, queries, nq, count, false);
}

int pirgpu_batch_stage_async(pirgpu_ctx* c, const uint64_t* pinned_queries, uint32_t nq, uint32_t count) {
  return batch_stage_impl(c, pinned_queries, nq, count, true);
}

int pirgpu_batch_unstage(pirgpu_ctx* c) {
  return guarded(c, [&]() -> int {
    BatchSet& b = c->bs();
    b.staged_count = 0;
    b.batch_keysets.clear();
    b.batch_keyset_gens.clear();
    b.batch_tables.clear();
    b.st_pieces = 0;
    return PIRGPU_OK;
  });
}

// ---- compact queries: c0 (plain or packed words) + the 64-byte seed of c1 per ciphertext ----
static QueryUnpackArgs cq_args(const pirgpu_ctx* c, bool packed) {
  return query_unpack_args(c->N, c->prm.coeff_modulus, c->k, packed);
}

uint64_t pirgpu_query_compact_words(const pirgpu_ctx* c, int packed) { return c ? cq_args(c, packed != 0).obj_words : 0; }

// every c0 coefficient below its modulus (a packed value may be anywhere in [q, 2^w)); c1 needs no check
static bool cq_in_range(const pirgpu_ctx* c, const QueryUnpackArgs& a, const uint64_t* compact, size_t n_cts) {
  bool ok = true;
  for (size_t i = 0; i < n_cts; ++i)
    for (uint32_t j = 0; j < c->k; ++j)
      ok &= rpk::check_poly(compact + i * a.obj_words + a.off[j], c->N, a.w[j], c->prm.coeff_modulus[j]);
  return ok;
}

static void refuse_compact(const pirgpu_ctx* c) {
  if (c->slot_sharded || c->sb != 0 || c->se != c->dims[0])
    throw Fail{PIRGPU_FAILED_PRECONDITION, "compact queries are staged on one GPU: this context is a row or slot shard"};
}

// the stage for `count` queries of nq ciphertexts: plain-form words (the larger form), then the gathered seeds.  Grows
// by the rule of ensure_batch_capacity.
static void ensure_cq_stage(pirgpu_ctx* c, uint32_t count) {
  if (!c->d_cq_stats) {
    HIP_TRY(hipMalloc((void**)&c->d_cq_stats, 2 * 8));
    HIP_TRY(hipMemsetAsync(c->d_cq_stats, 0, 2 * 8, c->stream));
  }
  if (!c->h_cq_stats) HIP_TRY(hipHostMalloc((void**)&c->h_cq_stats, 2 * 8, hipHostMallocDefault));
  if (count <= c->cq_cap) return;
  const uint32_t nq = c->dim_sum / c->N + 1;
  if (c->d_cq_stage) {
    HIP_TRY(hipStreamSynchronize(c->stream));   // its only reader and writer
    HIP_TRY(hipFree(c->d_cq_stage));
    c->d_cq_stage = nullptr;
  }
  const uint32_t cap = std::max<uint32_t>(count, std::min<uint32_t>(4096, 2 * c->cq_cap));
  c->cq_cap = 0;
  HIP_TRY(hipMalloc((void**)&c->d_cq_stage, (size_t)cap * nq * ((size_t)c->k * c->N + 8 + 8) * 8));
  c->cq_cap = cap;
}
static uint64_t* cq_seed_area(const pirgpu_ctx* c) {
  return c->d_cq_stage + (size_t)c->cq_cap * (c->dim_sum / c->N + 1) * ((size_t)c->k * c->N + 8);
}

// queries [q0, q0 + n) of a call, nq ciphertexts each: upload their compact words to the stage, unpack c0 and re-sample
// c1 into dst, one array of ciphertexts [query][nq][2][k][N], all on the main stream
static void cq_expand_queue(pirgpu_ctx* c, const QueryUnpackArgs& a, const uint64_t* compact, uint32_t nq, uint32_t q0,
                            uint32_t n, uint64_t* dst) {
  const size_t at = (size_t)q0 * nq, cts = (size_t)n * nq, dst_qstride = (size_t)nq * c->ctw;
  uint64_t* stage = c->d_cq_stage + at * a.obj_words;
  uint64_t* seeds = cq_seed_area(c) + at * 8;
  HIP_TRY(hipMemcpyAsync(stage, compact + at * a.obj_words, cts * a.obj_words * 8, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(launch_query_unpack(c->stream, a, stage, dst + (size_t)q0 * dst_qstride, seeds, nq, c->ctw, n, dst_qstride));
  const SeedExpandArgs sa = seed_expand_args(c, false);
  const size_t half = (size_t)c->k * c->N;
  HIP_TRY(launch_seed_expand(c->stream, sa, reinterpret_cast<const uint8_t*>(seeds), (uint32_t)cts,
                             dst + (size_t)q0 * dst_qstride + half, c->ctw, c->d_cq_stats));
  c->cq_objects += cts;
}

// The one wait of a synchronous call: the kernel's counters come back in stream order behind the expansion, as the key
// path's do; an overrun of the kernel's stream bound is an error (and is cleared).  The asynchronous entry points do
// not look at the flag: it cannot be set for a modulus a context accepts -- a prime below 2^61 accepts more than 7 draws
// of 8, and max_refills allows four times the stream an object needs without a rejection -- so the check is a guard for
// the kernel's own arithmetic, which the synchronous calls and the hook exercise on the same code.
static void cq_wait_checked(pirgpu_ctx* c) {
  HIP_TRY(hipMemcpyAsync(c->h_cq_stats, c->d_cq_stats, 2 * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->h_cq_stats[1]) {
    HIP_TRY(hipMemsetAsync(c->d_cq_stats + 1, 0, 8, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    throw Fail{PIRGPU_INTERNAL, "seed expansion ran past its stream bound"};
  }
}

static int query_stage_compact_impl(pirgpu_ctx* c, const uint64_t* compact, uint32_t nq, int packed, bool wait) {
  return guarded(c, [&]() -> int {
    refuse_compact(c);
    ensure_workspace(c);
    Worker& w = c->workers[0];
    if (!compact || nq != c->dim_sum / c->N + 1)  // reference server.cpp:154-158
      return fail(c, PIRGPU_INVALID_ARGUMENT,
                  "Number of ciphertexts doesn't match number of items for oblivious expansion.");
    const QueryUnpackArgs a = cq_args(c, packed != 0);
    if (!cq_in_range(c, a, compact, nq))
      return fail(c, PIRGPU_INVALID_ARGUMENT, "ciphertext data is invalid (coefficient out of range)");
    ensure_cq_stage(c, 1);
    HIP_TRY(hipStreamWaitEvent(c->stream, w.ev_done, 0));
    cq_expand_queue(c, a, compact, nq, 0, 1, w.d_query);
    if (wait) cq_wait_checked(c);   // the caller may reuse `compact` at once
    w.staged_nq = nq;
    return PIRGPU_OK;
  });
}

int pirgpu_query_stage_compact(pirgpu_ctx* c, const uint64_t* compact, uint32_t nq, int packed) {
  return query_stage_compact_impl(c, compact, nq, packed, true);
}

int pirgpu_query_stage_compact_async(pirgpu_ctx* c, const uint64_t* pinned_compact, uint32_t nq, int packed) {
  return query_stage_compact_impl(c, pinned_compact, nq, packed, false);
}

static int batch_stage_compact_impl(pirgpu_ctx* c, const uint64_t* compact, uint32_t nq, uint32_t count, int packed,
                                    bool async) {
  return guarded(c, [&]() -> int {
    refuse_compact(c);
    ensure_workspace(c);
    if (!compact || nq != c->dim_sum / c->N + 1)  // reference server.cpp:154-158
      return fail(c, PIRGPU_INVALID_ARGUMENT,
                  "Number of ciphertexts doesn't match number of items for oblivious expansion.");
    if (count == 0 || count > 4096) return fail(c, PIRGPU_INVALID_ARGUMENT, "batch size must be in [1, 4096]");
    const QueryUnpackArgs a = cq_args(c, packed != 0);
    if (!cq_in_range(c, a, compact, (size_t)count * nq))
      return fail(c, PIRGPU_INVALID_ARGUMENT, "ciphertext data is invalid (coefficient out of range)");
    ensure_batch_capacity(c, count);
    ensure_cq_stage(c, count);
    BatchSet& b = c->bs();
    // head-stream work queued earlier may still import queries of this set's previous batch: uploads go behind it
    if (c->ev_head_tail) HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_head_tail, 0));
    if (async) {
      // as pirgpu_batch_stage_async: a piece's event is recorded behind its expansion, so a group still waits for
      // exactly the pieces that hold its queries
      const uint32_t pieces = (count + kStagePiece - 1) / kStagePiece;
      while (b.st_events.size() < pieces) {
        hipEvent_t e;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        b.st_events.push_back(e);
      }
      for (uint32_t p = 0; p < pieces; ++p) {
        const uint32_t q0 = p * kStagePiece, n = std::min<uint32_t>(kStagePiece, count - q0);
        cq_expand_queue(c, a, compact, nq, q0, n, b.d_bquery);
        HIP_TRY(hipEventRecord(b.st_events[p], c->stream));
      }
      b.st_pieces = pieces;
    } else {
      for (uint32_t q0 = 0; q0 < count; q0 += 1024)   // the launch bounds of the two kernels (65535 objects)
        cq_expand_queue(c, a, compact, nq, q0, std::min<uint32_t>(1024, count - q0), b.d_bquery);
      cq_wait_checked(c);
      b.st_pieces = 0;
    }
    b.batch_count = count;
    b.staged_count = count;
    b.batch_keysets.assign(count, 0);
    b.batch_keyset_gens.assign(count, 0);
    b.batch_tables.clear();
    b.batch_valid = false;
    return PIRGPU_OK;
  });
}

int pirgpu_batch_stage_compact(pirgpu_ctx* c, const uint64_t* compact, uint32_t nq, uint32_t count, int packed) {
  return batch_stage_compact_impl(c, compact, nq, count, packed, false);
}

int pirgpu_batch_stage_compact_async(pirgpu_ctx* c, const uint64_t* pinned_compact, uint32_t nq, uint32_t count, int packed) {
  return batch_stage_compact_impl(c, pinned_compact, nq, count, packed, true);
}

int pirgpu_query_expand(pirgpu_ctx* c, const uint64_t* compact, uint32_t n, int packed, uint64_t* out) {
  return guarded(c, [&]() -> int {
    if (n && (!compact || !out)) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    if (!n) return PIRGPU_OK;
    const QueryUnpackArgs a = cq_args(c, packed != 0);
    if (!cq_in_range(c, a, compact, n))
      return fail(c, PIRGPU_INVALID_ARGUMENT, "ciphertext data is invalid (coefficient out of range)");
    // the staging path itself, one ciphertext per "query": pieces of kStagePiece, each uploaded, unpacked and expanded
    const uint32_t nq = c->dim_sum / c->N + 1;
    ensure_cq_stage(c, (n + nq - 1) / nq);
    DevScratch buf;
    uint64_t* d_out = buf.get<uint64_t>((size_t)n * c->ctw * 8);
    for (uint32_t q0 = 0; q0 < n; q0 += kStagePiece)
      cq_expand_queue(c, a, compact, 1, q0, std::min<uint32_t>(kStagePiece, n - q0), d_out);
    HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)n * c->ctw * 8, hipMemcpyDeviceToHost, c->stream));
    cq_wait_checked(c);
    return PIRGPU_OK;
  });
}

int pirgpu_query_expand_stats(pirgpu_ctx* c, uint64_t stats[2]) {
  return guarded(c, [&]() -> int {
    if (!stats) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    stats[0] = c->cq_objects;
    stats[1] = 0;
    if (c->d_cq_stats) {
      HIP_TRY(hipStreamSynchronize(c->stream));
      HIP_TRY(hipMemcpy(&stats[1], c->d_cq_stats, 8, hipMemcpyDeviceToHost));
    }
    return PIRGPU_OK;
  });
}

// `stream` waits for the upload of the staged queries [first, first + n) (asynchronously staged batches only)
static void wait_staged(pirgpu_ctx* c, hipStream_t stream, uint32_t first, uint32_t n) {
  BatchSet& b = c->bs();
  if (!b.st_pieces || !n) return;
  const uint32_t p0 = first / kStagePiece, p1 = std::min<uint32_t>(b.st_pieces - 1, (first + n - 1) / kStagePiece);
  for (uint32_t p = p0; p <= p1; ++p) HIP_TRY(hipStreamWaitEvent(stream, b.st_events[p], 0));
}

// Batch staging (queries + replies, device resident) for at least `count` queries.  Growth frees the old pair
// (after every stream that may still touch it has drained) and at least doubles, so a peer that sends ever
// larger requests cannot accumulate stale buffers.
static void ensure_batch_capacity(pirgpu_ctx* c, uint32_t count) {
  if (count <= c->bs().batch_cap) return;
  const uint32_t nq = c->dim_sum / c->N + 1;
  const uint32_t old_cap = c->bs().batch_cap;
  if (c->bs().d_bquery || c->bs().d_breply) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (BatchLane& ln : c->lanes)
      if (ln.stream) HIP_TRY(hipStreamSynchronize(ln.stream));
    for (Worker& w : c->workers)
      if (w.stream) HIP_TRY(hipStreamSynchronize(w.stream));
    for (uint64_t* p : {c->bs().d_bquery, c->bs().d_breply}) {
      if (!p) continue;
      auto it = std::find(c->allocs.begin(), c->allocs.end(), (void*)p);
      if (it != c->allocs.end()) c->allocs.erase(it);
      HIP_TRY(hipFree(p));
    }
    c->bs().d_bquery = c->bs().d_breply = nullptr;
    c->bs().batch_cap = 0;
    c->bs().batch_valid = false;
    c->bs().staged_count = 0;   // the staged queries went with the old buffer
  }
  const uint32_t cap = std::max<uint32_t>(count, std::min<uint32_t>(4096, 2 * old_cap));
  c->bs().d_bquery = c->dalloc<uint64_t>((size_t)cap * nq * c->ctw);
  c->bs().d_breply = c->dalloc<uint64_t>((size_t)cap * c->reply_cts * c->rctw);
  c->bs().batch_cap = cap;
}

// Lanes (stream + expansion buffers for up to 8 interleaved queries), created on the first batch.
static void ensure_lanes(pirgpu_ctx* c, bool with_expansion_buffers) {
  const uint32_t N = c->N, k = c->k;
  if (c->lanes.empty()) {
    // groups in flight (each lane = one stream + one set of group buffers): two -- one, three and four lanes were measured
    // in rounds 2 and 4 (3 857 / 4 114 / 4 090 against 4 165; 5 304 against 5 427 queries/s), a constant since round 5
    const uint32_t n_lanes = 2;
    c->lanes.resize(n_lanes);
    for (BatchLane& ln : c->lanes) {
      HIP_TRY(hipStreamCreateWithFlags(&ln.stream, hipStreamNonBlocking));
      HIP_TRY(hipEventCreateWithFlags(&ln.ev_scanned, hipEventDisableTiming));
    }
  }
  if (with_expansion_buffers && !c->lanes[0].res_a) {
    const uint64_t half = std::max<uint64_t>(c->m_max / 2, 1);
    for (BatchLane& ln : c->lanes) {
      ln.res_a = c->dalloc<uint64_t>((size_t)kMaxMfmaQueries * c->m_max * c->ctw);
      ln.res_b = c->dalloc<uint64_t>((size_t)kMaxMfmaQueries * c->m_max * c->ctw);
      ln.prod = c->dalloc<uint64_t>((size_t)kMaxMfmaQueries * half * 2 * (k + 1) * N);
      ln.dig = c->dalloc<uint64_t>((size_t)kMaxMfmaQueries * half * (k + 1) * k * N);
    }
  }
  if (c->mfma_on && c->lanes[0].lvl.empty()) {  // the group's multiply runs in lane-owned, query-major buffers
    for (BatchLane& ln : c->lanes) {
      ln.lvl.assign(c->d, nullptr);
      for (uint32_t l = 0; l < c->d; ++l) ln.lvl[l] = c->dalloc<uint64_t>((size_t)kMaxMfmaQueries * c->lvl_cts[l] * c->ctw);
      if (c->rp || c->pack) ln.last = c->dalloc<uint64_t>((size_t)kMaxMfmaQueries * c->lvl_cts[0] * c->ctw);
      if (c->pt_words) ln.pt_buf = c->dalloc<uint64_t>((size_t)kMaxMfmaQueries * c->pt_words);
      if (c->mg.nchunks > 1)
        ln.scan_part = c->dalloc<uint64_t>((size_t)kMaxMfmaQueries * c->mg.nchunks * std::max<uint32_t>(c->scan_rows, 1) * c->ctw);
    }
  }
}

// The second group of a paired database pass: its selection vectors, packed column selectors and row sums, lane-owned
// (the lane's workers hold the first group's; stream order on the lane covers the reuse from pair to pair and call to call)
static void ensure_pair_buffers(pirgpu_ctx* c, BatchLane& ln, bool expands) {
  if (expands && !ln.sv2) ln.sv2 = c->dalloc<uint64_t>((size_t)kMaxMfmaQueries * c->dim_sum * c->ctw);
  if (ln.selp2) return;
  ln.selp2 = c->dalloc<uint8_t>(c->mg.sel_bytes);
  ln.rows2 = c->dalloc<uint64_t>((size_t)kMaxMfmaQueries * c->lvl_cts[c->d - 1] * c->ctw);
}

static void ensure_head_slot(pirgpu_ctx* c, HeadSlot& hs) {
  if (hs.res_a) return;
  const uint32_t N = c->N, k = c->k;
  const uint64_t cts = ((uint64_t)1 << c->head_levels) * kMaxMfmaQueries;   // tree ciphertexts after the last head level
  hs.res_a = c->dalloc<uint64_t>(cts * c->ctw);
  hs.res_b = c->dalloc<uint64_t>(cts * c->ctw);
  hs.prod = c->dalloc<uint64_t>(std::max<uint64_t>(cts / 2, 1) * 2 * (k + 1) * N);
  hs.dig = c->dalloc<uint64_t>(std::max<uint64_t>(cts / 2, 1) * (k + 1) * k * N);
  HIP_TRY(hipEventCreateWithFlags(&hs.ev_ready, hipEventDisableTiming));
  HIP_TRY(hipEventCreateWithFlags(&hs.ev_free, hipEventDisableTiming));
  if (!c->head_stream) {
    HIP_TRY(hipStreamCreateWithFlags(&c->head_stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&c->ev_head_tail, hipEventDisableTiming));
  }
}

// ---- what every walk over groups shares (batch_run_mfma, the 64-bit rounds, the packed and the slot-sharded steps) ----

static uint32_t active_workers(const pirgpu_ctx* c) { return active_workers(c->n_active, (uint32_t)c->workers.size()); }
static uint32_t lanes_in_use(const pirgpu_ctx* c, uint32_t G) { return lanes_in_use(active_workers(c), G, (uint32_t)c->lanes.size()); }

// `after` / `then` (a stream of the caller's, may be null): the lane waits for what is queued on `after` so far, `then`
// for what is queued on the lane so far.
static void lane_after(pirgpu_ctx* c, hipStream_t lane, void* after) {
  if (!after) return;
  if (!c->ev_after) HIP_TRY(hipEventCreateWithFlags(&c->ev_after, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(c->ev_after, (hipStream_t)after));
  HIP_TRY(hipStreamWaitEvent(lane, c->ev_after, 0));
}
static void lane_then(BatchLane& ln, void* then) {
  if (!then) return;
  if (!ln.ev_join) HIP_TRY(hipEventCreateWithFlags(&ln.ev_join, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(ln.ev_join, ln.stream));
  HIP_TRY(hipStreamWaitEvent((hipStream_t)then, ln.ev_join, 0));
}

// The next lane of `nl` in turn, with n workers bound to it as the members of its group (they lend their selection-vector
// buffers): member q is worker (lane * per_lane + base + q) mod W -- lane-bound with per_lane = G, so that stream order
// on the lane covers their reuse -- and the lane waits until whoever used a member's buffers last is done.
struct LaneClaim {
  BatchLane& ln;
  uint32_t n;
  Worker* members[kMaxMfmaQueries];
};
static LaneClaim claim_lane(pirgpu_ctx* c, uint32_t nl, uint32_t n, uint32_t per_lane, uint32_t base = 0, void* after = nullptr) {
  const uint32_t li = (uint32_t)(c->groups_run++ % nl), W = active_workers(c);
  LaneClaim cl{c->lanes[li], n, {}};
  lane_after(c, cl.ln.stream, after);
  for (uint32_t q = 0; q < n; ++q) {
    cl.members[q] = &c->workers[(li * per_lane + base + q) % W];
    HIP_TRY(hipStreamWaitEvent(cl.ln.stream, cl.members[q]->ev_done, 0));
  }
  return cl;
}
// The members' buffers are free once the lane got here (replies_elsewhere: in the lane / batch buffers, not the workers').
static void release_lane(const LaneClaim& cl, bool replies_elsewhere) {
  for (uint32_t q = 0; q < cl.n; ++q) {
    HIP_TRY(hipEventRecord(cl.members[q]->ev_done, cl.ln.stream));
    if (replies_elsewhere) cl.members[q]->reply_valid = false;
  }
}

// The multiply of a group of n queries in a lane's query-major buffers -- except the row sums (level d - 1) at `rows` and
// level 0 at `lvl0` where given: the replies' own place, so that the last fold and the final inverse transform write them
// where they are read (no device-to-device copy per group).
struct LaneStage {
  uint64_t* lvl[PIRGPU_MAX_DIMS];
  Stage sg;
  LaneStage(const pirgpu_ctx* c, BatchLane& ln, uint32_t n, uint64_t* lvl0, uint64_t* rows)
      : sg{ln.stream, lvl, ln.pt_buf, n, MfmaPtrs{}, false, &ln.up_scratch, &ln.up_scratch_words} {
    for (uint32_t l = 0; l < c->d; ++l) lvl[l] = ln.lvl[l];
    if (rows) lvl[c->d - 1] = rows;
    if (lvl0) lvl[0] = lvl0;
    sg.last = ln.last;   // result_primes: level 0 lands there, the compact switch writes the replies to lvl[0]
  }
  LaneStage(const LaneStage&) = delete;
};

// Set while the batch pipeline enqueues work (pirgpu_ctx::in_batch), on every way out.
struct InBatch {
  bool& f;
  explicit InBatch(pirgpu_ctx* c) : f(c->in_batch) { f = true; }
  ~InBatch() { f = false; }
};

// pirgpu_batch_set_host_replies: a group's replies start their way to the host while the next groups are computed -- on
// the context's COPY stream, behind an event of the lane: the lane itself goes straight on to its next group (round 3
// queued the copy on the lane, which then idled for 8 MB of PCIe per group: 5-6 % of a lane's time at cfg 3).  The n
// replies from `first` on in one copy, or -- a permuted group -- those at scattered[q], one copy each; `report` = how many
// LEADING queries of the batch are complete with this group (the copy stream runs the groups' copies in order).
static void queue_download(pirgpu_ctx* c, BatchLane& ln, uint32_t first, uint32_t n, const uint32_t* scattered, uint32_t report) {
  BatchSet& b = c->bs();
  const size_t rwords = (size_t)c->reply_cts * c->rctw, gi = b.dl_end.size();
  while (gi >= b.dl_events.size()) {
    hipEvent_t e;
    HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    b.dl_events.push_back(e);
    HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    b.rd_events.push_back(e);
  }
  if (!c->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
  HIP_TRY(hipEventRecord(b.rd_events[gi], ln.stream));
  HIP_TRY(hipStreamWaitEvent(c->copy_stream, b.rd_events[gi], 0));
  for (uint32_t q = 0; q < (scattered ? n : 1); ++q) {
    const size_t at = (size_t)(scattered ? scattered[q] : first) * rwords;
    HIP_TRY(hipMemcpyAsync(b.host_reply + at, reply_base(c) + at, (scattered ? 1 : n) * rwords * 8, hipMemcpyDeviceToHost,
                           c->copy_stream));
  }
  HIP_TRY(hipEventRecord(b.dl_events[gi], c->copy_stream));
  b.dl_end.push_back(report);
}

// Batched oblivious expansion of the staged queries first .. first+B-1 on lane `ln`, B queries interleaved
// (ciphertext index = node * B + query), into the members' own selection vectors (NTT form).
// sv_dst (optional): the selection vector of query q goes to sv_dst + q * dim_sum ciphertexts (caller-owned memory that
// outlives the members' buffers: the slot-sharded step keeps its row selectors there for two steps) instead of the
// members' own buffers.
// qidx (optional; batches ordered by table): the staged query each member answers -- member q is query qidx[q] of the
// batch instead of first + q, and the roots are imported one query at a time.
static void expand_group_on_lane(pirgpu_ctx* c, BatchLane& ln, Worker* const* members, uint32_t B, uint32_t first,
                                 bool sel_f64 = false, uint64_t* sv_dst = nullptr, const uint32_t* qidx = nullptr) {
  const uint32_t N = c->N, k = c->k;
  const uint32_t nq = c->dim_sum / N + 1;
  const size_t ctw = c->ctw, qwords = (size_t)nq * ctw;
  uint64_t remaining = c->dim_sum, produced = 0;
  // the narrow first levels on the head stream (HeadSlot): one query ciphertext per query (the usual case), a real group,
  // and at least two levels left for the lane
  // -- for batches that were staged asynchronously (request windows queued behind one another: +6 % through the wire,
  // 12.0 against 12.9 ms per window of 64 with two callers) or always (head_mode 2); a back-to-back loop over one staged
  // batch gains nothing from it (5 325-5 408 against 5 379-5 433 queries/s, same box) and keeps the plain path
  const bool use_head = expansion_uses_head(nq, B, c->head_levels, c->head_mode == 2 || (c->head_mode == 1 && c->bs().st_pieces > 0),
                                            expansion_depth((uint32_t)std::min<uint64_t>(c->dim_sum, N)));
  // (a permuted group's queries may lie in any piece of the upload: it waits for all of them)
  const uint32_t ws_first = qidx ? 0 : first, ws_n = qidx ? c->bs().staged_count : B;
  if (!use_head) wait_staged(c, ln.stream, ws_first, ws_n);
  // the B query ciphertexts, gathered side by side out of the staged batch, become the roots of the B interleaved trees:
  // one strided import launch for consecutive queries (no separate 2-D copy), one launch per query for permuted ones
  auto import_roots = [&](hipStream_t st, uint64_t* dst, uint32_t qc) {
    if (!qidx) {
      HIP_TRY(launch_tree_convert(st, c->dp, c->mode, c->bs().d_bquery + (size_t)first * qwords + (size_t)qc * ctw, dst,
                                  (uint64_t)B * ctw, true, ctw, qwords));
      return;
    }
    for (uint32_t q = 0; q < B; ++q)
      HIP_TRY(launch_tree_convert(st, c->dp, c->mode, c->bs().d_bquery + (size_t)qidx[q] * qwords + (size_t)qc * ctw,
                                  dst + (size_t)q * ctw, ctw, true));
  };
  for (uint32_t qc = 0; qc < nq && remaining; ++qc) {
    const uint32_t slots = (uint32_t)std::min<uint64_t>(remaining, N);
    MfmaPtrs dst{};
    uint32_t ksets[kMaxMfmaQueries];   // every query of the group is switched with its own client's keys
    for (uint32_t q = 0; q < B; ++q) {
      dst.p[q] = (sv_dst ? sv_dst + (size_t)q * c->dim_sum * ctw : members[q]->sv_ntt) + produced * ctw;
      ksets[q] = keyset_of(c, qidx ? qidx[q] : first + q);
    }
    uint64_t* res;
    if (use_head) {
      HeadSlot& hs = ln.head[ln.head_next++ & 1];
      ensure_head_slot(c, hs);
      hipStream_t hst = c->head_stream;
      if (hs.in_use) HIP_TRY(hipStreamWaitEvent(hst, hs.ev_free, 0));   // the lane is done with the slot's previous tree
      wait_staged(c, hst, ws_first, ws_n);
      import_roots(hst, hs.res_a, qc);
      TreeState at;
      (void)expand_core(c, hst, hs.res_a, hs.res_b, hs.dig, hs.prod, slots, B, &dst, sel_f64, ksets, 0, c->head_levels, nullptr, &at);
      HIP_TRY(hipEventRecord(hs.ev_ready, hst));
      HIP_TRY(hipEventRecord(c->ev_head_tail, hst));
      HIP_TRY(hipStreamWaitEvent(ln.stream, hs.ev_ready, 0));
      res = expand_core(c, ln.stream, ln.res_a, ln.res_b, ln.dig, ln.prod, slots, B, &dst, sel_f64, ksets, c->head_levels,
                        UINT32_MAX, &at, nullptr, [&]() {
                          HIP_TRY(hipEventRecord(hs.ev_free, ln.stream));
                          hs.in_use = true;
                        });
    } else {
      import_roots(ln.stream, ln.res_a, qc);
      res = expand_core(c, ln.stream, ln.res_a, ln.res_b, ln.dig, ln.prod, slots, B, &dst, sel_f64, ksets);
    }
    if (res) HIP_TRY(c->ops->ct_ntt_fwd_split(ln.stream, c->mode, c->dp, k, res, dst, B, (uint64_t)slots * B));
    produced += slots;
    remaining -= slots;
  }
  for (uint32_t q = 0; q < B; ++q) {
    members[q]->sv_cur = nullptr;
    members[q]->sv_rows = nullptr;
  }
}

// Batch mode with the MFMA scan (see BatchLane): groups of up to mfma_nq queries share one batched
// expansion and one database pass; consecutive groups alternate between two lanes.
struct PackedInput {            // multi-GPU packed exchange (pirgpu_batch_run_packed)
  const uint8_t* packed;       // [src rank][group] digit-packed column selectors, mg.sel_bytes each
  const uint64_t* rows;        // [query][this shard's rows][2][k][N] dimension-0 selectors
  uint32_t per_rank;           // queries per source rank (groups never span two source ranks)
};

// The database pass of a group whose members named more than one table: run r = members [rb[r], rb[r + 1]) multiplies its
// column selectors with table tabs[r].  One launch for all runs (scan_mfma_runs_kernel; option TABLES_ONE_LAUNCH, default
// 1, geometries of the 8-wave kernels), else one launch of the usual pass per run.  Row sums land query-major in the
// lane's buffers exactly as a single-table group leaves them.
static void scan_group_runs(pirgpu_ctx* c, BatchLane& ln, const MfmaPtrs& col, uint32_t B, const uint32_t* rb, uint32_t nr,
                            const uint32_t* tabs, bool sel_f64, bool share_chip) {
  const uint32_t kN = c->k * c->N;
  const uint64_t words = (uint64_t)c->scan_rows * c->ctw;
  const uint32_t nch = c->mg.nchunks;
  ensure_packed(c);
  uint64_t* const out_base = ln.lvl[c->d - 1];
  if (!c->tables_one_launch || !scan_mfma_runs_supported(c->mg)) {
    for (uint32_t r = 0; r < nr; ++r) {
      MfmaPtrs cr{};
      for (uint32_t q = rb[r]; q < rb[r + 1]; ++q) cr.p[q - rb[r]] = col.p[q];
      // (stream order on the lane covers the reuse of the one selector buffer by the next run)
      scan_group_mfma(c, ln.stream, ln.selp, cr, rb[r + 1] - rb[r], out_base + rb[r] * words,
                      ln.scan_part ? ln.scan_part + (uint64_t)rb[r] * nch * words : nullptr, nullptr, nullptr, sel_f64,
                      share_chip, tabs[r]);
    }
    return;
  }
  if (!ln.selp_runs) ln.selp_runs = c->dalloc<uint8_t>((size_t)kMaxMfmaQueries * c->mg.sel_bytes);
  uint64_t* const out = nch > 1 ? ln.scan_part : out_base;
  const uint64_t out_qstride = nch > 1 ? (uint64_t)nch * words : words;
  ScanGroupsDb grp{};
  grp.n = nr;
  for (uint32_t r = 0; r < nr; ++r) {
    MfmaPtrs cr{};
    for (uint32_t q = rb[r]; q < rb[r + 1]; ++q) cr.p[q - rb[r]] = col.p[q];
    uint8_t* selp = ln.selp_runs + (size_t)r * c->mg.sel_bytes;
    HIP_TRY(launch_sel_pack(ln.stream, c->dp, c->mg, cr, rb[r + 1] - rb[r], selp, c->scan_cols, kN, sel_f64));
    grp.sel[r] = selp;
    grp.out[r] = out + rb[r] * out_qstride;
    grp.nq[r] = (uint8_t)(rb[r + 1] - rb[r]);
    grp.db[r] = table_dbp(c, tabs[r]);
  }
  const uint32_t wgs = share_chip && c->scan_wgs_batch ? c->scan_wgs_batch : 0;
  timed_scan_launch(c, ln.stream, wgs, B, [&] {
    HIP_TRY(launch_scan_mfma_runs(ln.stream, c->dp, c->mg, grp, c->scan_rows, kN, words, wgs,
                                  c->scan_f64_fold || c->scan_f64_fold_batch, out_qstride));
  });
  if (nch > 1)
    HIP_TRY(launch_reduce_splits(ln.stream, c->dp, ln.scan_part, nch, words, out_base, B, (uint64_t)nch * words, words));
}

// qtab (contexts with tables): the table of every query of the batch, by submission index.  The groups are then formed
// over the batch sorted by table (plan_table_runs); replies, key sets and downloads keep the submission index.
static void batch_run_mfma(pirgpu_ctx* c, uint32_t count, const uint64_t* ext_sv, const PackedInput* pk = nullptr,
                           const uint32_t* qtab = nullptr) {
  const size_t rwords = (size_t)c->reply_cts * c->rctw, svwords = (size_t)c->dim_sum * c->ctw;
  const uint32_t W = active_workers(c);
  const uint32_t G = std::min<uint32_t>(c->mfma_nq, W);
  TablePlan tp;
  if (qtab) tp = plan_table_runs(qtab, count, G);
  const uint32_t* order = qtab && !tp.identity ? tp.order.data() : nullptr;   // position in the served order -> staged query
  auto oq = [&](uint32_t pos) { return order ? order[pos] : pos; };
  auto tab = [&](uint32_t pos) { return qtab ? qtab[oq(pos)] : 0u; };
  LeadingReplies lead(order ? count : 0);   // permuted batch: what its groups report as downloaded
  const uint32_t my_rows = c->se - c->sb;
  ensure_lanes(c, !ext_sv && !pk);
  const uint32_t nl = lanes_in_use(c, G);
  // groups: runs of up to G consecutive queries; with packed input a group is what ONE source rank packed together
  // (its queries in runs of kMaxMfmaQueries), so the walk restarts at every source-rank boundary
  const uint32_t span = pk ? pk->per_rank : count, step = pk ? (uint32_t)kMaxMfmaQueries : G;
  // groups this call queues: with two or more (and two lanes) every pass runs on half the chip
  const uint32_t n_groups = count_groups(count, span, step);
  const bool share_chip = n_groups >= 2 && nl >= 2;
  // pirgpu_batch_set_host_replies: every group downloads its replies as soon as they exist (queue_download)
  const bool host_dl = c->bs().host_reply && (uint64_t)count * c->reply_cts <= c->bs().host_reply_cts;
  c->bs().host_reply_done = host_dl;
  c->bs().dl_end.clear();
  c->bs().dl_next = 0;
  // Two groups per database read (PIRGPU_SCAN_MFMA_PAIR, scan_mfma_pair.hip): a lane expands group a (into its workers'
  // selection vectors) and group b (into its own second buffer), packs both, scans the database ONCE for both, then
  // finishes a and b one after the other.  The plain case only: the context's own expansion of one database in one
  // column chunk (or caller-owned selection vectors), re-encoding upper levels at every prime, replies written in place.
  // Everything else -- an odd last group, short calls under value 1, tables, packed / slot-sharded input, result_primes,
  // wide items, ciphertext-multiplication mode -- keeps one pass per group.
  const bool may_pair = !pk && !qtab && c->d >= 2 && !c->ctm && !c->rp && c->planes <= 1 &&
                        G == (uint32_t)kMaxMfmaQueries && scan_mfma_pair_supported(c->mg) &&
                        pair_by_count(c->scan_pair, n_groups, nl);
  const bool sel_f64 = !pk && !ext_sv && c->sel_f64;   // a lane's own selectors, read on that lane only: exact doubles
  // (d = 1 would make the scan itself write to the replies, a permuted group's replies are not neighbours: the lane buffer)
  const bool direct_reply = c->d >= 2 && !order;
  for (const GroupStep& st : plan_group_walk(count, span, step, may_pair).steps) {
    const uint32_t nh = st.n[1] ? 2 : 1;
    if (st.n[0] > W) throw Fail{PIRGPU_FAILED_PRECONDITION, "packed groups need min(queries per rank, 8) workers (pirgpu_set_concurrency)"};
    const LaneClaim cl = claim_lane(c, nl, st.n[0], G);
    BatchLane& ln = cl.ln;
    if (nh == 2) ensure_pair_buffers(c, ln, !ext_sv);
    GroupHalf hv[2] = {{st.first[0], st.n[0], nullptr, ln.lvl[c->d - 1], {}, {}}, {st.first[1], st.n[1], ln.sv2, ln.rows2, {}, {}}};
    if (!pk && !ext_sv)
      for (uint32_t h = 0; h < nh; ++h)
        expand_group_on_lane(c, ln, cl.members, hv[h].n, hv[h].first, sel_f64, hv[h].sv, order ? order + hv[h].first : nullptr);
    for (uint32_t h = 0; h < nh; ++h)
      for (uint32_t q = 0; q < hv[h].n; ++q) {
        const uint64_t* own = hv[h].sv ? hv[h].sv + (size_t)q * svwords : cl.members[q]->sv_ntt;
        const uint64_t* sv = ext_sv ? ext_sv + (size_t)oq(hv[h].first + q) * svwords : own;
        // (packed input: the column selectors arrive packed, the row selectors are this shard's alone)
        hv[h].sel.p[q] = pk ? pk->rows + (size_t)(hv[h].first + q) * my_rows * c->ctw : sv;
        if (!pk) hv[h].col.p[q] = sv + (size_t)c->sv_off[c->d - 1] * c->ctw;
      }
    if (nh == 2) {
      scan_pair_mfma(c, ln, hv, sel_f64, share_chip);
    } else {
      const uint32_t first = hv[0].first, B = hv[0].n;
      const uint32_t groups_per_rank = pk ? (pk->per_rank + kMaxMfmaQueries - 1) / kMaxMfmaQueries : 0;
      const uint8_t* packed = !pk ? nullptr : pk->packed + ((size_t)(first / pk->per_rank) * groups_per_rank +
                                                             first % pk->per_rank / kMaxMfmaQueries) * c->mg.sel_bytes;
      // runs of equal tables among the members (one run without tables)
      uint32_t rb[kMaxMfmaQueries + 1], tabs[kMaxMfmaQueries], nr = 0;
      for (uint32_t q = 0; q < B; ++q)
        if (q == 0 || tab(first + q) != tab(first + q - 1)) {
          rb[nr] = q;
          tabs[nr++] = tab(first + q);
        }
      rb[nr] = B;
      if (nr == 1)
        scan_group_mfma(c, ln.stream, ln.selp, hv[0].col, B, hv[0].rows, ln.scan_part, nullptr, packed, sel_f64, share_chip, tabs[0]);
      else
        scan_group_runs(c, ln, hv[0].col, B, rb, nr, tabs, sel_f64, share_chip);
    }
    for (uint32_t h = 0; h < nh; ++h) {
      const uint32_t first = hv[h].first, B = hv[h].n;
      LaneStage ls(c, ln, B, direct_reply ? reply_base(c) + (size_t)first * rwords : nullptr, hv[h].rows);
      ls.sg.sel = hv[h].sel;
      ls.sg.local_rows = pk != nullptr;
      ls.sg.sel_f64 = sel_f64;
      for (uint32_t q = 0; q < B; ++q) ls.sg.ksets[q] = keyset_of(c, oq(first + q));
      post_scan_stage(c, ls.sg, nullptr);
      if (order) {   // every reply to its query's own place
        for (uint32_t q = 0; q < B; ++q)
          HIP_TRY(hipMemcpyAsync(reply_base(c) + (size_t)oq(first + q) * rwords, ln.lvl[0] + (size_t)q * rwords, rwords * 8,
                                 hipMemcpyDeviceToDevice, ln.stream));
      } else if (!direct_reply)
        HIP_TRY(hipMemcpyAsync(reply_base(c) + (size_t)first * rwords, ln.lvl[0], (size_t)B * rwords * 8,
                               hipMemcpyDeviceToDevice, ln.stream));
      if (host_dl) queue_download(c, ln, first, B, order ? order + first : nullptr, order ? lead.mark(order + first, B) : first + B);
    }
    release_lane(cl, true);
  }
}

// Shared body of pirgpu_batch_run / pirgpu_batch_run_selectors: `count` queries in rounds of W (one worker
// per query).  Expansion is batched per group of up to 8 queries on a lane; with the MFMA scan the group
// also shares the database pass (batch_run_mfma), otherwise groups of up to 4 workers share one pass of
// scan_mq_kernel (d = 1 / few rows), hand-offs between streams through events.  With ext_sv the expansion
// is skipped and query i reads its NTT-form selection vector at ext_sv + i*dim_sum.
static void batch_run_impl(pirgpu_ctx* c, uint32_t count, const uint64_t* ext_sv) {
  InBatch in_batch(c);
  refuse_slot_shard(c);
  c->bs().host_reply_done = false;   // set again by the path that queues per-group downloads (batch_run_mfma)
  const size_t rwords = (size_t)c->reply_cts * c->rctw;
  const size_t svwords = (size_t)c->dim_sum * c->ctw;
  const uint32_t W = active_workers(c);
  const uint32_t G = mq_usable(c) && c->pt_end > c->pt_begin ? std::min<uint32_t>(c->mq_nq, kMaxScanQueries) : 1;
  // contexts with tables: the table of every query -- what pirgpu_batch_set_tables left for this many queries, else the
  // table selected with pirgpu_query_use_table for all of them.  Every named table must be complete and free of zero
  // plaintexts before anything is queued (the batch fails as a whole, like a batch on one database)
  std::vector<uint32_t> qtab_v;
  if (c->tables > 1) {
    qtab_v = c->bs().batch_tables.size() == count ? c->bs().batch_tables : std::vector<uint32_t>(count, c->cur_table);
    for (uint32_t t : qtab_v) {
      if (!table_loaded(c, t)) throw Fail{PIRGPU_FAILED_PRECONDITION, "table " + std::to_string(t) + " not fully loaded"};
      check_transparent(c, t);
    }
  } else {
    if (c->n_loaded != held_pts(c))
      throw Fail{PIRGPU_FAILED_PRECONDITION, "database not fully loaded"};
    check_transparent(c);
  }
  const uint32_t* qtab = qtab_v.empty() ? nullptr : qtab_v.data();
  check_reply_target(c, count);
  if (!ext_sv) check_staged_keysets(c);
  if (c->ctm && c->d >= 2)   // every query's relinearisation key, before anything is queued
    for (uint32_t i = 0; i < count; ++i) {
      const uint32_t slot = keyset_of(c, i);
      (void)relin_keys_for(c, &slot, 1);
    }
  ensure_packed(c);
  c->prof_cur = -1;
  if (c->mfma_on) {
    batch_run_mfma(c, count, ext_sv, nullptr, qtab);
    c->bs().batch_valid = true;
    return;
  }
  // 64-bit scans: the same order by table, so that the queries one pass of scan_mq_kernel serves share their table
  TablePlan tp;
  if (qtab) tp = plan_table_runs(qtab, count, kMaxMfmaQueries);
  const uint32_t* order = qtab && !tp.identity ? tp.order.data() : nullptr;
  auto oq = [&](uint32_t pos) { return order ? order[pos] : pos; };
  if (!ext_sv) ensure_lanes(c, true);
  for (uint32_t base = 0; base < count; base += W) {
    const uint32_t n = std::min<uint32_t>(W, count - base);
    for (uint32_t j = 0; j < n; ++j) c->workers[j].table = qtab ? qtab[oq(base + j)] : 0;
    if (ext_sv) {
      for (uint32_t j = 0; j < n; ++j) {
        Worker& w = c->workers[j];
        w.sv_cur = ext_sv + (size_t)oq(base + j) * svwords;
        HIP_TRY(hipEventRecord(w.ev_expanded, w.stream));
      }
    } else {
      for (uint32_t j0 = 0; j0 < n; j0 += kMaxMfmaQueries) {
        const uint32_t B = std::min<uint32_t>(kMaxMfmaQueries, n - j0);
        // every lane, and worker j0 + q itself as member q: it goes on with its own query on its own stream
        const LaneClaim cl = claim_lane(c, (uint32_t)c->lanes.size(), B, 0, j0);
        expand_group_on_lane(c, cl.ln, cl.members, B, base + j0, false, nullptr, order ? order + base + j0 : nullptr);
        for (uint32_t q = 0; q < B; ++q) {
          HIP_TRY(hipEventRecord(cl.members[q]->ev_expanded, cl.ln.stream));
          HIP_TRY(hipStreamWaitEvent(cl.members[q]->stream, cl.members[q]->ev_expanded, 0));
        }
      }
    }
    for (uint32_t j0 = 0; j0 < n; j0 += G) {
      const uint32_t g = std::min<uint32_t>(G, n - j0);
      uint32_t done = 0;
      while (done < g) {  // group sizes the kernel is instantiated for: 4, 2, 1
        uint32_t take = g - done >= 4 && G >= 4 ? 4 : (g - done >= 2 && G >= 2 ? 2 : 1);
        Worker& lead = c->workers[j0 + done];
        while (take > 1) {   // (tables: one pass reads one table)
          bool same = true;
          for (uint32_t q = 1; q < take; ++q) same = same && c->workers[j0 + done + q].table == lead.table;
          if (same) break;
          take /= 2;
        }
        if (take == 1) {
          scan_on_device(c, lead);
        } else {
          const uint64_t* svp[kMaxScanQueries];
          uint64_t* outp[kMaxScanQueries];
          for (uint32_t q = 0; q < take; ++q) {
            Worker& m = c->workers[j0 + done + q];
            if (q) HIP_TRY(hipStreamWaitEvent(lead.stream, m.ev_expanded, 0));
            svp[q] = scan_selectors(c, m);
            outp[q] = scan_out(c, m);
          }
          const uint32_t rpw = take == 4 ? (c->mq_rows > 2 ? 1 : c->mq_rows) : (c->mq_rows > 2 ? 2 : c->mq_rows);
          HIP_TRY(launch_scan_mq(lead.stream, c->dp, c->N, c->k, table_db(c, lead.table), svp, outp, take, c->scan_rows,
                                 c->scan_cols, rpw, c->scan_limb));
          HIP_TRY(hipEventRecord(lead.ev_scanned, lead.stream));
          for (uint32_t q = 1; q < take; ++q)
            HIP_TRY(hipStreamWaitEvent(c->workers[j0 + done + q].stream, lead.ev_scanned, 0));
        }
        done += take;
      }
    }
    for (uint32_t j = 0; j < n; ++j) {
      Worker& w = c->workers[j];
      w.keyset = keyset_of(c, oq(base + j));
      post_scan_on_device(c, w);
      HIP_TRY(hipMemcpyAsync(reply_base(c) + (size_t)oq(base + j) * rwords, w.lvl[0], rwords * 8, hipMemcpyDeviceToDevice,
                             w.stream));
      HIP_TRY(hipEventRecord(w.ev_done, w.stream));
      w.reply_valid = true;
    }
  }
  c->bs().batch_valid = true;
}

int pirgpu_batch_run(pirgpu_ctx* c) {
  return guarded(c, [&]() -> int {
    if (!c->bs().staged_count) return fail(c, PIRGPU_FAILED_PRECONDITION, "no batch has been staged");
    batch_run_impl(c, c->bs().staged_count, nullptr);
    c->bs().batch_count = c->bs().staged_count;
    return PIRGPU_OK;
  });
}

// ======================================================================================================================
// [9] MULTI-GPU entry points: u64 selector exchange, packed row-shard exchange, slot shards, reply copies, fix-up, pack40
// ======================================================================================================================
// ---- query-parallel expansion for multi-GPU ----

int pirgpu_batch_expand(pirgpu_ctx* c, uint32_t first, uint32_t count, uint64_t* device_dst) {
  return guarded(c, [&]() -> int {
    if (!c->bs().staged_count || (uint64_t)first + count > c->bs().staged_count)
      return fail(c, PIRGPU_INVALID_ARGUMENT, "query range outside the staged batch");
    if (!device_dst && count) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    const uint32_t nq = c->dim_sum / c->N + 1;
    const size_t qwords = (size_t)nq * c->ctw, svwords = (size_t)c->dim_sum * c->ctw;
    const uint32_t W = active_workers(c);
    c->prof_cur = -1;
    check_staged_keysets(c);
    for (uint32_t i = 0; i < count; ++i) {
      Worker& w = c->workers[i % W];
      HIP_TRY(hipStreamWaitEvent(w.stream, w.ev_done, 0));   // a lane's group may still be reading its buffers
      wait_staged(c, w.stream, first + i, 1);
      HIP_TRY(hipMemcpyAsync(w.d_query, c->bs().d_bquery + (size_t)(first + i) * qwords, qwords * 8,
                             hipMemcpyDeviceToDevice, w.stream));
      w.staged_nq = nq;
      w.keyset = keyset_of(c, first + i);
      expand_query_to_sv(c, w, w.d_query, nq);
      HIP_TRY(hipMemcpyAsync(device_dst + (size_t)i * svwords, w.sv_ntt, svwords * 8, hipMemcpyDeviceToDevice,
                             w.stream));
    }
    for (Worker& w : c->workers) HIP_TRY(hipStreamSynchronize(w.stream));
    return PIRGPU_OK;
  });
}

int pirgpu_batch_run_selectors(pirgpu_ctx* c, const uint64_t* device_sv, uint32_t count) {
  return guarded(c, [&]() -> int {
    ensure_workspace(c);
    if (!device_sv || count == 0 || count > 4096) return fail(c, PIRGPU_INVALID_ARGUMENT, "invalid batch");
    ensure_batch_capacity(c, count);
    batch_run_impl(c, count, device_sv);
    c->bs().batch_count = count;
    return PIRGPU_OK;
  });
}

// ---- packed selector exchange for row-sharded multi-GPU runs ----

uint64_t pirgpu_packed_selector_bytes(pirgpu_ctx* c) {
  uint64_t bytes = 0;
  (void)guarded(c, [&]() -> int {
    ensure_workspace(c);
    // d = 2 only (dimension 0 = rows, dimension 1 = the scanned columns) and the shard scanned by the MFMA kernel
    if (c->d == 2 && c->mfma_on && c->planes == 1) bytes = c->mg.sel_bytes;
    return PIRGPU_OK;
  });
  return bytes;
}

static int batch_expand_packed_impl(pirgpu_ctx* c, uint32_t first_query, uint32_t count, uint8_t* device_packed,
                                    uint64_t* device_rows, const uint32_t* row_cuts, uint32_t n_ranks, bool wait) {
  return guarded(c, [&]() -> int {
    refuse_wide(c);
    refuse_tables(c);
    refuse_switched(c);
    refuse_packed(c);
    refuse_ctm(c);
    ensure_workspace(c);
    if (c->d != 2 || !c->mfma_on)
      return fail(c, PIRGPU_FAILED_PRECONDITION, "packed selector exchange needs d = 2 and the int8-MFMA scan");
    if (!c->bs().staged_count || (uint64_t)first_query + count > c->bs().staged_count)
      return fail(c, PIRGPU_INVALID_ARGUMENT, "query range outside the staged batch");
    if (!device_packed || !device_rows || !row_cuts || n_ranks == 0 || row_cuts[0] != 0 || row_cuts[n_ranks] != c->dims[0])
      return fail(c, PIRGPU_INVALID_ARGUMENT, "invalid packed-exchange buffers or row cuts");
    for (uint32_t s = 0; s < n_ranks; ++s)
      if (row_cuts[s] > row_cuts[s + 1]) return fail(c, PIRGPU_INVALID_ARGUMENT, "row cuts must be non-decreasing");
    const uint32_t W = active_workers(c);
    if (W < std::min<uint32_t>(count, kMaxMfmaQueries))
      return fail(c, PIRGPU_FAILED_PRECONDITION, "packed groups need min(count, 8) workers (pirgpu_set_concurrency)");
    ensure_lanes(c, true);
    c->prof_cur = -1;
    check_staged_keysets(c);
    const size_t ctw = c->ctw;
    const uint32_t kN = c->k * c->N;
    const uint32_t first = first_query;
    const uint32_t G = std::min<uint32_t>(kMaxMfmaQueries, W), nl = lanes_in_use(c, G);
    uint32_t g = 0;
    for (uint32_t j0 = 0; j0 < count; j0 += kMaxMfmaQueries, ++g) {
      const uint32_t B = std::min<uint32_t>(kMaxMfmaQueries, count - j0);
      const LaneClaim cl = claim_lane(c, nl, B, G);
      BatchLane& ln = cl.ln;
      Worker* const* members = cl.members;
      expand_group_on_lane(c, ln, members, B, first + j0);
      // column selectors (dimension 1) of the whole group -> one B-operand buffer
      MfmaPtrs sv{};
      for (uint32_t q = 0; q < B; ++q) sv.p[q] = members[q]->sv_ntt + (size_t)c->sv_off[1] * ctw;
      HIP_TRY(launch_sel_pack(ln.stream, c->dp, c->mg, sv, B, device_packed + (size_t)g * c->mg.sel_bytes, c->scan_cols, kN));
      // row selectors (dimension 0): block of destination rank s = [query][rows of s][2][k][N]
      for (uint32_t s2 = 0; s2 < n_ranks; ++s2) {
        const uint32_t r0 = row_cuts[s2], nr = row_cuts[s2 + 1] - r0;
        if (!nr) continue;
        for (uint32_t q = 0; q < B; ++q)
          HIP_TRY(hipMemcpyAsync(device_rows + ((size_t)count * r0 + (size_t)(j0 + q) * nr) * ctw,
                                 members[q]->sv_ntt + (size_t)(c->sv_off[0] + r0) * ctw, (size_t)nr * ctw * 8,
                                 hipMemcpyDeviceToDevice, ln.stream));
      }
      release_lane(cl, false);
    }
    if (wait)
      for (BatchLane& ln : c->lanes) HIP_TRY(hipStreamSynchronize(ln.stream));
    return PIRGPU_OK;
  });
}

int pirgpu_batch_expand_packed(pirgpu_ctx* c, uint32_t first_query, uint32_t count, uint8_t* device_packed,
                               uint64_t* device_rows, const uint32_t* row_cuts, uint32_t n_ranks) {
  return batch_expand_packed_impl(c, first_query, count, device_packed, device_rows, row_cuts, n_ranks, true);
}

int pirgpu_batch_expand_packed_async(pirgpu_ctx* c, uint32_t first_query, uint32_t count, uint8_t* device_packed,
                                     uint64_t* device_rows, const uint32_t* row_cuts, uint32_t n_ranks) {
  return batch_expand_packed_impl(c, first_query, count, device_packed, device_rows, row_cuts, n_ranks, false);
}

int pirgpu_batch_run_packed(pirgpu_ctx* c, const uint8_t* device_packed, uint32_t n_ranks, uint32_t per_rank,
                            const uint64_t* device_rows) {
  return guarded(c, [&]() -> int {
    refuse_wide(c);
    refuse_tables(c);
    refuse_switched(c);
    refuse_packed(c);
    refuse_ctm(c);
    ensure_workspace(c);
    if (c->d != 2 || !c->mfma_on)
      return fail(c, PIRGPU_FAILED_PRECONDITION, "packed selector exchange needs d = 2 and the int8-MFMA scan");
    refuse_slot_shard(c);
    const uint64_t count = (uint64_t)n_ranks * per_rank;
    if (!device_packed || !device_rows || count == 0 || count > 4096) return fail(c, PIRGPU_INVALID_ARGUMENT, "invalid batch");
    if (c->n_loaded != held_pts(c)) return fail(c, PIRGPU_FAILED_PRECONDITION, "database not fully loaded");
    check_transparent(c);
    check_reply_target(c, count);
    ensure_packed(c);
    ensure_batch_capacity(c, (uint32_t)count);
    c->prof_cur = -1;
    PackedInput pk{device_packed, device_rows, per_rank};
    {
      InBatch in_batch(c);
      batch_run_mfma(c, (uint32_t)count, nullptr, &pk);
    }
    c->bs().batch_count = (uint32_t)count;
    c->bs().batch_valid = true;
    return PIRGPU_OK;
  });
}

// ---- slot-sharded multi-GPU step ----
//
// The base case of PIRDatabase::multiply (reference database.cpp:185-194) is a dyadic product in NTT form: independent
// per NTT slot.  G ranks therefore each hold the slots [cut[g], cut[g+1]) of EVERY plaintext (1 / G of the bytes; the
// operand layout has the slot outermost) and a step of B queries runs as
//   E  rank g expands its own B / G queries (groups of 8) and packs their column selectors, cut by destination rank;
//   X1 all-to-all: rank h receives ITS slots of every group's packed column selectors (1 / G of each);
//   S  rank h scans its slots for all B queries in one launch: full row tiles, row sums [query][row, comp][its slots];
//   X2 all-to-all: the row sums go back to the rank that expanded the query;
//   U  that rank puts the slot pieces together and runs inverse NTT + upper level for its own queries on ALL rows with
//      the row selectors it kept: reply i ends on the rank that owns query i.  No row-selector exchange, no reduce.
// The three entry points queue E, S and U on the lanes without waiting for the device.  `after` / `then` (hipStream_t
// of the caller, may be NULL) order them against the caller's collectives: every lane the call uses first waits for what
// is queued on `after` so far, and `then` waits for what the call queued.

namespace {

void check_cuts(pirgpu_ctx* c, const uint32_t* cuts, uint32_t n_ranks, SliceMap& map) {
  const uint32_t kN = c->k * c->N;
  if (!cuts || n_ranks == 0 || n_ranks > (uint32_t)kMaxSlices || cuts[0] != 0 || cuts[n_ranks] != kN)
    throw Fail{PIRGPU_INVALID_ARGUMENT, "slot cuts must run from 0 to k N over at most 16 ranks"};
  map = SliceMap{};
  map.n = n_ranks;
  for (uint32_t r = 0; r <= n_ranks; ++r) {
    if (cuts[r] % 16 || (r && cuts[r] < cuts[r - 1])) throw Fail{PIRGPU_INVALID_ARGUMENT, "slot cuts must be non-decreasing multiples of 16"};
    map.cut[r] = cuts[r];
  }
}

void check_slots_ctx(pirgpu_ctx* c) {
  refuse_wide(c);
  refuse_tables(c);
  refuse_switched(c);
  refuse_packed(c);
  refuse_ctm(c);
  ensure_workspace(c);
  if (c->d != 2 || !c->mfma_on || c->mg.nchunks != 1 || c->sb != 0 || c->se != c->dims[0])
    throw Fail{PIRGPU_FAILED_PRECONDITION, "the slot-sharded step needs d = 2, all rows and the int8-MFMA scan in one column chunk"};
}

}  // namespace

uint64_t pirgpu_slots_packed_bytes(pirgpu_ctx* c, uint32_t slots) {
  uint64_t bytes = 0;
  (void)guarded(c, [&]() -> int {
    ensure_workspace(c);
    if (c->d == 2 && c->mfma_on && c->mg.nchunks == 1 && c->planes == 1) bytes = (uint64_t)slots * c->mg.KG * c->mg.tile_bytes;
    return PIRGPU_OK;
  });
  return bytes;
}

int pirgpu_slots_expand_async(pirgpu_ctx* c, uint32_t first, uint32_t count, uint8_t* device_packed, uint64_t* device_sv,
                              const uint32_t* slot_cuts, uint32_t n_ranks, void* after, void* then) {
  return guarded(c, [&]() -> int {
    check_slots_ctx(c);
    SliceMap map;
    check_cuts(c, slot_cuts, n_ranks, map);
    if (!c->bs().staged_count || (uint64_t)first + count > c->bs().staged_count)
      return fail(c, PIRGPU_INVALID_ARGUMENT, "query range outside the staged batch");
    if (!device_packed || !device_sv || count == 0) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    const uint32_t W = active_workers(c);
    if (W < std::min<uint32_t>(count, kMaxMfmaQueries))
      return fail(c, PIRGPU_FAILED_PRECONDITION, "groups need min(count, 8) workers (pirgpu_set_concurrency)");
    ensure_lanes(c, true);
    c->prof_cur = -1;
    check_staged_keysets(c);
    const size_t ctw = c->ctw, svwords = (size_t)c->dim_sum * ctw;
    const uint32_t kN = c->k * c->N;
    const uint32_t G = std::min<uint32_t>(kMaxMfmaQueries, W), nl = lanes_in_use(c, G);
    const uint32_t groups = (count + kMaxMfmaQueries - 1) / kMaxMfmaQueries;
    const uint64_t slot_bytes = (uint64_t)c->mg.KG * c->mg.tile_bytes;
    if (after && c->head_stream) lane_after(c, c->head_stream, after);
    uint32_t g = 0;
    for (uint32_t j0 = 0; j0 < count; j0 += kMaxMfmaQueries, ++g) {
      const uint32_t B = std::min<uint32_t>(kMaxMfmaQueries, count - j0);
      const LaneClaim cl = claim_lane(c, nl, B, G, 0, after);
      BatchLane& ln = cl.ln;
      uint64_t* sv_dst = device_sv + (size_t)j0 * svwords;
      expand_group_on_lane(c, ln, cl.members, B, first + j0, c->sel_f64, sv_dst);
      // the group's column selectors -> B-operand tiles, rank r's slots as piece [r][group g] of the send buffer
      MfmaPtrs sv{};
      for (uint32_t q = 0; q < B; ++q) sv.p[q] = sv_dst + (size_t)q * svwords + (size_t)c->sv_off[1] * ctw;
      for (uint32_t r = 0; r < n_ranks; ++r)
        map.off[r] = ((uint64_t)groups * map.cut[r] + (uint64_t)g * (map.cut[r + 1] - map.cut[r])) * slot_bytes;
      HIP_TRY(launch_sel_pack(ln.stream, c->dp, c->mg, sv, B, device_packed, c->scan_cols, kN, c->sel_f64, &map));
      release_lane(cl, false);
      lane_then(ln, then);
    }
    return PIRGPU_OK;
  });
}

int pirgpu_slots_scan_async(pirgpu_ctx* c, const uint8_t* device_packed, uint32_t n_ranks, uint32_t per_rank,
                            uint64_t* device_rowsums, void* after, void* then) {
  return guarded(c, [&]() -> int {
    check_slots_ctx(c);
    const uint64_t count = (uint64_t)n_ranks * per_rank;
    if (!device_packed || !device_rowsums || count == 0 || count > 4096) return fail(c, PIRGPU_INVALID_ARGUMENT, "invalid batch");
    if (c->n_loaded != held_pts(c)) return fail(c, PIRGPU_FAILED_PRECONDITION, "database not fully loaded");
    check_transparent(c);
    ensure_packed(c);
    ensure_lanes(c, true);
    c->prof_cur = -1;
    const uint32_t nl = lanes_in_use(c, std::min<uint32_t>(kMaxMfmaQueries, active_workers(c)));
    BatchLane& ln = claim_lane(c, nl, 0, 0, 0, after).ln;
    const uint32_t groups = (per_rank + kMaxMfmaQueries - 1) / kMaxMfmaQueries;
    const uint64_t piece = (uint64_t)c->nslots * c->mg.KG * c->mg.tile_bytes;      // my slots of one packed group
    const uint64_t qwords = (uint64_t)c->scan_rows * 2 * c->nslots;                // row sums of one query on my slots
    // workgroups: the pass shares the chip with the other lane's expansion like the single-GPU batch pass (option
    // SLOTS_SCAN_WGS; unset: as many as that pass).  Units in (slot block, group) order: option SLOTS_SCAN_BLK_MAJOR
    const uint32_t wgs = c->slots_scan_wgs < 0 ? c->scan_wgs_batch : (uint32_t)c->slots_scan_wgs;
    ScanGroups grp{};
    auto flush = [&]() {
      if (!grp.n) return;
      HIP_TRY(launch_scan_mfma_groups(ln.stream, c->dp, c->mg, c->d_dbp, grp, c->scan_rows, 0, wgs,
                                      c->scan_f64_fold || c->scan_f64_fold_batch, c->slot0,
                                      c->nslots, qwords, c->nslots, c->slots_blk_major));
      grp = ScanGroups{};
    };
    for (uint32_t r = 0; r < n_ranks; ++r)
      for (uint32_t g = 0; g < groups; ++g) {
        grp.sel[grp.n] = device_packed + ((uint64_t)r * groups + g) * piece;
        grp.out[grp.n] = device_rowsums + ((uint64_t)r * per_rank + (uint64_t)g * kMaxMfmaQueries) * qwords;
        grp.nq[grp.n] = (uint8_t)std::min<uint32_t>(kMaxMfmaQueries, per_rank - g * kMaxMfmaQueries);
        if (++grp.n == (uint32_t)kMaxScanGroups) flush();
      }
    flush();
    lane_then(ln, then);
    return PIRGPU_OK;
  });
}

int pirgpu_slots_finish_async(pirgpu_ctx* c, const uint64_t* device_rowsums, uint32_t count, const uint64_t* device_sv,
                              const uint32_t* slot_cuts, uint32_t n_ranks, uint64_t* device_replies, void* after,
                              void* then) {
  return guarded(c, [&]() -> int {
    check_slots_ctx(c);
    SliceMap map;
    check_cuts(c, slot_cuts, n_ranks, map);
    if (!device_rowsums || !device_sv || !device_replies || count == 0 || count > 4096)
      return fail(c, PIRGPU_INVALID_ARGUMENT, "invalid batch");
    ensure_lanes(c, true);
    c->prof_cur = -1;
    const uint32_t nl = lanes_in_use(c, std::min<uint32_t>(kMaxMfmaQueries, active_workers(c)));
    const size_t ctw = c->ctw, svwords = (size_t)c->dim_sum * ctw, rwords = (size_t)c->reply_cts * ctw;
    const uint32_t kN = c->k * c->N, RC = c->scan_rows * 2;
    const uint64_t words = (uint64_t)c->scan_rows * ctw;
    InBatch in_batch(c);
    for (uint32_t j0 = 0; j0 < count; j0 += kMaxMfmaQueries) {
      const uint32_t B = std::min<uint32_t>(kMaxMfmaQueries, count - j0);
      BatchLane& ln = claim_lane(c, nl, 0, 0, 0, after).ln;
      // rank h's block of the receive buffer holds [count][RC][slots of h]: the group's queries are rows j0 .. j0 + B of
      // it; the inverse transform of the row sums (database.cpp:250-254) gathers them from there (option
      // SLOTS_GATHER_NTT = 0: a separate assembly pass, then the plain in-place transform)
      bool gather = c->slots_gather_ntt;
      const uint32_t nt = c->N >> ntt_log_ept((int)c->logN);    // threads of a transform workgroup
      for (uint32_t r = 0; r <= n_ranks; ++r) gather = gather && map.cut[r] % nt == 0;
      if (gather)
        HIP_TRY(c->ops->ntt_inv_gather(ln.stream, c->mode, c->dp, c->k, device_rowsums, ln.lvl[c->d - 1], map, RC, B, count, j0));
      else
        HIP_TRY(launch_slots_assemble(ln.stream, device_rowsums, ln.lvl[c->d - 1], map, RC, kN, B, words, count, j0));
      LaneStage ls(c, ln, B, device_replies + (size_t)j0 * rwords, nullptr);
      for (uint32_t q = 0; q < B; ++q) ls.sg.sel.p[q] = device_sv + (size_t)(j0 + q) * svwords;
      ls.sg.sel_f64 = c->sel_f64;
      ls.sg.rows_inverted = gather;
      post_scan_stage(c, ls.sg, nullptr);
      lane_then(ln, then);
    }
    return PIRGPU_OK;
  });
}

int pirgpu_batch_reply_copy_to_device(pirgpu_ctx* c, uint64_t* dst, uint64_t cap) {
  return guarded(c, [&]() -> int {
    refuse_switched(c);
    refuse_packed(c);
    refuse_ctm(c);
    if (!c->bs().batch_valid) return fail(c, PIRGPU_FAILED_PRECONDITION, "no batch has been run");
    const uint64_t total = (uint64_t)c->bs().batch_count * c->reply_cts;
    if (!dst || cap < total) return fail(c, PIRGPU_INVALID_ARGUMENT, "reply buffer too small");
    sync_batch_streams(c);
    // a device-to-device hipMemcpy on the null stream may return before the copy has run, and the context's
    // streams are non-blocking (not ordered with the null stream): copy on the context's stream and wait
    HIP_TRY(hipMemcpyAsync(dst, reply_base(c), total * c->rctw * 8, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PIRGPU_OK;
  });
}

int pirgpu_batch_reply_copy_to_device_async(pirgpu_ctx* c, uint64_t* dst, uint64_t cap) {
  int rc = guarded(c, [&]() -> int {
    refuse_switched(c);
    refuse_packed(c);
    refuse_ctm(c);
    return PIRGPU_OK;
  });
  if (rc) return rc;
  rc = pirgpu_join(c);   // the main stream now follows every lane: the copy below sees the finished batch
  if (rc) return rc;
  return guarded(c, [&]() -> int {
    if (!c->bs().batch_valid) return fail(c, PIRGPU_FAILED_PRECONDITION, "no batch has been run");
    const uint64_t total = (uint64_t)c->bs().batch_count * c->reply_cts;
    if (!dst || cap < total) return fail(c, PIRGPU_INVALID_ARGUMENT, "reply buffer too small");
    HIP_TRY(hipMemcpyAsync(dst, reply_base(c), total * c->rctw * 8, hipMemcpyDeviceToDevice, c->stream));
    return PIRGPU_OK;
  });
}

int pirgpu_batch_fetch(pirgpu_ctx* c, uint64_t* replies, uint64_t cap, uint64_t* count) {
  return guarded(c, [&]() -> int {
    if (!c->bs().batch_valid) return fail(c, PIRGPU_FAILED_PRECONDITION, "no batch has been run");
    const uint64_t total = (uint64_t)c->bs().batch_count * c->reply_cts;
    if (!replies || cap < total) return fail(c, PIRGPU_INVALID_ARGUMENT, "reply buffer too small");
    sync_batch_streams(c);
    if (!(c->bs().host_reply_done && replies == c->bs().host_reply))   // else: the groups downloaded their replies themselves
      HIP_TRY(hipMemcpy(replies, reply_base(c), total * c->rctw * 8, hipMemcpyDeviceToHost));
    if (count) *count = total;
    return PIRGPU_OK;
  });
}

static int ntt_hook(pirgpu_ctx* c, uint64_t* polys, uint64_t count, int key_level, bool inverse) {
  return guarded(c, [&]() -> int {
    if (!polys && count) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    const uint32_t per = key_level ? c->k + 1 : c->k;
    const uint64_t npoly = key_level ? count * per : count * 2 * per;
    // the hook speaks SEAL's NTT order at the boundary; the kernels use device order
    uint64_t* dev = nullptr;
    HIP_TRY(hipMalloc((void**)&dev, 2 * std::max<uint64_t>(npoly, 1) * c->N * 8));
    uint64_t* tmp = dev + std::max<uint64_t>(npoly, 1) * c->N;
    try {
      if (inverse) {
        HIP_TRY(hipMemcpyAsync(tmp, polys, npoly * c->N * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(launch_ntt_reorder(c->stream, c->N, tmp, dev, npoly, true, false));
        HIP_TRY(c->ops->ntt_batch(c->stream, c->mode, c->dp, dev, npoly, per, 0, true));
        HIP_TRY(hipMemcpyAsync(polys, dev, npoly * c->N * 8, hipMemcpyDeviceToHost, c->stream));
      } else {
        HIP_TRY(hipMemcpyAsync(dev, polys, npoly * c->N * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c->ops->ntt_batch(c->stream, c->mode, c->dp, dev, npoly, per, 0, false));
        HIP_TRY(launch_ntt_reorder(c->stream, c->N, dev, tmp, npoly, false, false));
        HIP_TRY(hipMemcpyAsync(polys, tmp, npoly * c->N * 8, hipMemcpyDeviceToHost, c->stream));
      }
      HIP_TRY(hipStreamSynchronize(c->stream));
    } catch (...) {
      (void)hipFree(dev);
      throw;
    }
    HIP_TRY(hipFree(dev));
    return PIRGPU_OK;
  });
}

int pirgpu_ntt_forward(pirgpu_ctx* c, uint64_t* polys, uint64_t count, int key_level) {
  return ntt_hook(c, polys, count, key_level, false);
}
int pirgpu_ntt_inverse(pirgpu_ctx* c, uint64_t* polys, uint64_t count, int key_level) {
  return ntt_hook(c, polys, count, key_level, true);
}

int pirgpu_reduce_fixup_device(pirgpu_ctx* c, uint64_t* device_ptr, uint64_t count) {
  return guarded(c, [&]() -> int {
    refuse_switched(c);
    refuse_packed(c);
    refuse_ctm(c);
    if (!device_ptr) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    HIP_TRY(launch_reduce_splits(c->stream, c->dp, device_ptr, 1, count * c->ctw, device_ptr));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return PIRGPU_OK;
  });
}

int pirgpu_reduce_fixup_device_async(pirgpu_ctx* c, uint64_t* device_ptr, uint64_t count, void* stream) {
  return guarded(c, [&]() -> int {
    refuse_switched(c);
    refuse_packed(c);
    refuse_ctm(c);
    if (!device_ptr) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    HIP_TRY(launch_reduce_splits(st, c->dp, device_ptr, 1, count * c->ctw, device_ptr));
    return PIRGPU_OK;
  });
}

// Row selectors of the multi-GPU exchange in 5 bytes per residue (moduli below 2^40): pack before the all-to-all,
// unpack behind it.  words: multiple of 4; `packed` holds words * 5 / 4 dwords.  stream NULL: the main stream.
static bool moduli_fit_40_bits(const pirgpu_ctx* c) {
  for (uint32_t j = 0; j < c->k; ++j)
    if (c->hp.mod[j].q >> 40) return false;
  return true;
}
int pirgpu_pack40_supported(pirgpu_ctx* c) { return c && moduli_fit_40_bits(c) ? 1 : 0; }

int pirgpu_pack40_device_async(pirgpu_ctx* c, const uint64_t* words_in, uint32_t* packed, uint64_t words, void* stream) {
  return guarded(c, [&]() -> int {
    if (!words_in || !packed || words % 4) return fail(c, PIRGPU_INVALID_ARGUMENT, "invalid buffers for the 5-byte form");
    if (!moduli_fit_40_bits(c)) return fail(c, PIRGPU_FAILED_PRECONDITION, "the 5-byte form needs moduli below 2^40");
    HIP_TRY(launch_pack40x4(stream ? (hipStream_t)stream : c->stream, words_in, packed, words));
    return PIRGPU_OK;
  });
}

int pirgpu_unpack40_device_async(pirgpu_ctx* c, const uint32_t* packed, uint64_t* words_out, uint64_t words, void* stream) {
  return guarded(c, [&]() -> int {
    if (!words_out || !packed || words % 4) return fail(c, PIRGPU_INVALID_ARGUMENT, "invalid buffers for the 5-byte form");
    if (!moduli_fit_40_bits(c)) return fail(c, PIRGPU_FAILED_PRECONDITION, "the 5-byte form needs moduli below 2^40");
    HIP_TRY(launch_unpack40x4(stream ? (hipStream_t)stream : c->stream, packed, words_out, words));
    return PIRGPU_OK;
  });
}

// ======================================================================================================================
// [10] MEASUREMENT: phase timings, batch scan timings
// ======================================================================================================================
int pirgpu_set_profiling(pirgpu_ctx* c, int enabled) {
  return guarded(c, [&]() -> int {
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->prof = enabled != 0;
    c->prof_runs = 0;
    c->bscan_n = 0;
    return PIRGPU_OK;
  });
}

int pirgpu_last_timings(pirgpu_ctx* c, float ms[6], uint32_t* runs) {
  return guarded(c, [&]() -> int {
    if (!ms) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    if (c->prof_runs > 0) {
      HIP_TRY(hipStreamSynchronize(c->stream));
      // events per run: [EXPAND] start, [SVNTT] end of expansion + selector NTT, [SCAN] scan start,
      //                 [UPPER] scan end, [FINAL] last multiply-accumulate end, [COUNT] end of run
      double acc[6] = {0, 0, 0, 0, 0, 0};
      for (int r = 0; r < c->prof_runs; ++r) {
        hipEvent_t* e = &c->ev[(size_t)r * (PH_COUNT + 1)];
        float t;
        HIP_TRY(hipEventElapsedTime(&t, e[PH_EXPAND], e[PH_SCAN]));
        acc[0] += t;
        HIP_TRY(hipEventElapsedTime(&t, e[PH_SCAN], e[PH_UPPER]));
        acc[2] += t;
        HIP_TRY(hipEventElapsedTime(&t, e[PH_UPPER], e[PH_FINAL]));
        acc[3] += t;
        HIP_TRY(hipEventElapsedTime(&t, e[PH_FINAL], e[PH_COUNT]));
        acc[4] += t;
        HIP_TRY(hipEventElapsedTime(&t, e[PH_EXPAND], e[PH_COUNT]));
        acc[5] += t;
      }
      for (int i = 0; i < 6; ++i) c->timings[i] = (float)(acc[i] / c->prof_runs);
      if (runs) *runs = (uint32_t)c->prof_runs;
      c->prof_runs = 0;
    } else if (runs) {
      *runs = 0;
    }
    memcpy(ms, c->timings, sizeof(c->timings));
    return PIRGPU_OK;
  });
}

int pirgpu_batch_scan_timings(pirgpu_ctx* c, float* mean_ms, float* min_ms, uint32_t* launches, uint32_t* workgroups,
                              uint32_t* queries) {
  return guarded(c, [&]() -> int {
    if (!mean_ms || !min_ms || !launches) return fail(c, PIRGPU_INVALID_ARGUMENT, "null buffer");
    sync_batch_streams(c);
    double sum = 0, mn = 1e30;
    for (uint32_t i = 0; i < c->bscan_n; ++i) {
      float t = 0;
      HIP_TRY(hipEventElapsedTime(&t, c->bscan_ev[2 * i], c->bscan_ev[2 * i + 1]));
      sum += t;
      mn = std::min<double>(mn, t);
    }
    *launches = c->bscan_n;
    *mean_ms = c->bscan_n ? (float)(sum / c->bscan_n) : 0.f;
    *min_ms = c->bscan_n ? (float)mn : 0.f;
    if (workgroups) *workgroups = c->bscan_wgs;
    if (queries) *queries = c->bscan_nq;
    c->bscan_n = 0;
    return PIRGPU_OK;
  });
}

uint32_t pirgpu_get_concurrency(pirgpu_ctx* c) { return c ? c->n_active : 0; }

// pirgpu_free: wire.cpp (response buffers are recycled)

}  // extern "C"
