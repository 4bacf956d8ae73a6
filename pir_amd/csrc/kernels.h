// kernels.h -- launch wrappers of the gfx950 kernels (kernels.hip, ntt_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_params.h"
#include "expansion_plan.h"

namespace pirgpu {

constexpr int kMaxScanChunks = 16;    // column chunks of one MFMA scan pass (wider matrices use the 64-bit kernels)
constexpr int kMaxMfmaQueries = 8;   // (query, comp) pairs fill the 16 columns of one MFMA tile
constexpr int kMaxScanGroups = 16;   // groups of <= 8 queries one scan launch can serve (slot-sharded multi-GPU step)
constexpr int kMaxSlices = 16;       // slot ranges (= ranks) a packed selector buffer / row-sum exchange can be cut into

// (kKsWideLevel and ks_digit_takes_c0, which the kernels share with the expansion's plan: expansion_plan.h)

struct MfmaPtrs {                    // one pointer per query of a group (by-value kernel argument)
  const void* p[kMaxMfmaQueries];
};

// Groups of one scan launch (by-value kernel argument): group g reads its packed selectors at sel[g] and writes query q
// to out[g] + q * out_qstride.
struct ScanGroups {
  uint32_t n;
  const uint8_t* sel[kMaxScanGroups];
  uint64_t* out[kMaxScanGroups];
  uint8_t nq[kMaxScanGroups];
};

// ... with a database per group (contexts with tables): group g scans the operand layout at db[g], every one a complete
// layout of the same geometry.
struct ScanGroupsDb : ScanGroups {
  const uint8_t* db[kMaxScanGroups];
};

// Slot ranges [cut[r], cut[r+1]) (multiples of 16, cut[0] = 0, cut[n] = k N) and, for sel_pack, the byte offset of each
// range's piece in the output buffer.
struct SliceMap {
  uint32_t n;
  uint32_t cut[kMaxSlices + 1];
  uint64_t off[kMaxSlices];
};

// Galois keys for ONE Galois element of the queries expanded together: tree ciphertext n (= node * B + query) is
// switched with p[n % B].  Keys are per request in the reference (PIRServer::ProcessRequest deserialises them into a
// local, server.cpp:46-48), so the queries of one group may come from different clients; B = 1: one key for all.
struct KeyPtrs {
  const uint64_t* p[kMaxMfmaQueries];
  uint32_t B;
};

// Kernels that contain an NTT, for one ring degree (ntt_kernels.hip is compiled once
// per degree; N = 32768 has its own translation unit, ntt_ring32k.hip, integer flavour only).  `mode` is an NttMode.
struct NttOps {
  hipError_t (*configure)(int mode);
  hipError_t (*ntt_batch)(hipStream_t st, int mode, const DevParams* P, uint64_t* data, uint64_t n_polys,
                          uint32_t mod_period, uint32_t mod_base, bool inverse);
  // src_is_tree: the source holds the expansion tree's element type (doubles in the fp64 flavours)
  hipError_t (*ct_ntt_fwd_oop)(hipStream_t st, int mode, const DevParams* P, uint32_t k, const uint64_t* src,
                               uint64_t* dst, uint64_t n_cts, bool src_is_tree);
  // same transform for B interleaved queries (source ciphertext i*B + q -> dst.p[q] + i): batched expansion
  hipError_t (*ct_ntt_fwd_split)(hipStream_t st, int mode, const DevParams* P, uint32_t k, const uint64_t* src,
                                 const MfmaPtrs& dst, uint32_t B, uint64_t n_cts_total);
  // planes > 1 (wide items, byte source only): source row pt is a whole item of bytes_per_pt bytes and plane j encodes
  // its bytes [j * plane_bytes, min((j + 1) * plane_bytes, bytes_per_pt)) into plaintext j * plane_stride + pt of db
  hipError_t (*db_encode)(hipStream_t st, int mode, const DevParams* P, uint32_t k, const uint64_t* coeffs,
                          const uint8_t* bytes, uint64_t bytes_per_pt, uint64_t total_bytes, uint32_t bits,
                          uint64_t n_pt, uint64_t* db, uint32_t planes, uint64_t plane_bytes, uint64_t plane_stride);
  // c0_out != nullptr (fp64 flavours, ks_digit_takes_c0(nodes)): the launch also writes NTT(c0) of every node into the
  // product buffer c0_out (NTT-domain last level), sparing ks_last_ntt its own launch for that (c0_done)
  // tree40: res_in holds the tree in the 5-byte form (wide levels of the fused expansion, ks_mac_combine's tout40)
  hipError_t (*ks_digit)(hipStream_t st, int mode, const DevParams* P, uint32_t k, const uint64_t* res_in,
                         uint32_t galois_elt, uint32_t nodes, uint64_t* dig, bool pack40, uint64_t* c0_out, bool tree40,
                         bool loop_targets);   // loop_targets (fp64 flavours, wide levels): one workgroup per source, k + 1 transforms each
  // key-level moduli I_base .. I_base + I_count - 1 (all: 0, k + 1; the special prime alone: k, 1)
  hipError_t (*ks_mac_intt)(hipStream_t st, int mode, const DevParams* P, uint32_t k, const uint64_t* dig,
                            const KeyPtrs& key, uint32_t nodes, uint64_t* prod, bool pack40, uint32_t I_base,
                            uint32_t I_count);
  // n_queries queries in one launch: query q reads src + q * src_qstride, selectors svq.p[q], writes part + q * part_qstride;
  // sel_f64 (fp64 flavours): the selectors are canonical residues stored as exact doubles (lane-internal form)
  hipError_t (*upper_fused)(hipStream_t st, int mode, const DevParams* P, uint32_t k, uint32_t enc_count,
                            const uint64_t* src, const MfmaPtrs& svq, uint64_t* part, uint32_t n_rows,
                            uint32_t n_dim, uint32_t n_children_total, uint32_t sv_first, uint32_t C,
                            uint32_t chunk_len, uint32_t n_chunks, uint32_t n_queries, uint64_t src_qstride,
                            uint64_t part_qstride, bool sel_f64);
  // last expansion level fused with the selectors' forward NTT (fp64 flavours): tree_cts tree ciphertexts
  // (index = slot * B + query) -> selectors slot and slot + shift_pow of query q at dst.p[q], if < n_items
  hipError_t (*ks_last_level)(hipStream_t st, int mode, const DevParams* P, uint32_t k, const uint64_t* tree,
                              const uint64_t* prod, uint32_t galois_elt, uint32_t shift_pow, uint32_t n_items,
                              uint32_t B, const MfmaPtrs& dst, uint32_t tree_cts, bool pack40);
  // split upper level, part 1 (fp64 flavours, large rings): re-encode + lift + forward NTT of the children
  // [b0, b0 + blk) of every row into scratch [query][row][cc][child in block][chunk][target modulus][N] doubles
  hipError_t (*upper_ntt)(hipStream_t st, int mode, const DevParams* P, uint32_t k, uint32_t enc_count,
                          const uint64_t* src, uint64_t* scratch, uint32_t n_rows, uint32_t n_dim,
                          uint32_t n_children_total, uint32_t C, uint32_t b0, uint32_t blk, uint32_t n_queries,
                          uint64_t src_qstride, bool loop_source);   // loop_source: one workgroup per (child, source polynomial)
  // data residues of one level below the last: MAC + inverse transform + combine with the special-prime product
  // (already in `prod`) + tree butterfly, tree_in -> tree_out (fp64 flavours); tin40 / tout40: that tree buffer holds
  // 5-byte polynomials (5 N bytes each, offset form) instead of doubles -- tout40 needs shift_pow < N / 16
  hipError_t (*ks_mac_combine)(hipStream_t st, int mode, const DevParams* P, uint32_t k, const uint64_t* dig,
                               const KeyPtrs& key, const uint64_t* prod, const uint64_t* tree_in, uint32_t galois_elt,
                               uint32_t nodes, uint32_t shift_pow, uint64_t* tree_out, bool pack40, bool tin40,
                               bool tout40, const uint64_t* xpow_c0ntt,    // xpow_c0ntt != null: the tree's c0 is in NTT form
                               const uint16_t* perm,    // ... and sigma_g's table for it (ctx.hip galois_perm_table)
                               bool c0_split);          // ... with component 0 as a launch of its own
  // last expansion level in the NTT domain (fp64 flavours): `prod` holds the special-prime products (ks_mac_intt with
  // I_base = k) and receives NTT(a_0); xpow = NTT_j(x^(-shift_pow)), [k][N] doubles; galois_inv = galois_elt^-1 mod 2N
  hipError_t (*ks_last_ntt)(hipStream_t st, int mode, const DevParams* P, uint32_t k, const uint64_t* tree,
                            const uint64_t* dig, const KeyPtrs& key, uint64_t* prod, const uint64_t* xpow,
                            uint32_t galois_elt, uint32_t galois_inv, uint32_t shift_pow, uint32_t n_items, uint32_t B,
                            const MfmaPtrs& dst, uint32_t nodes, bool pack40, bool out_f64, bool c0_done, int c0_tree,
                            const uint16_t* perm);   // [2][N]: sigma_g, sigma_(g^-1) on NTT positions as padded LDS indices
  // slot-sharded step: inverse NTT of the row sums of queries q0 .. q0 + nq - 1, gathered from the per-rank slot pieces
  // of the all-to-all receive buffer (nq_total queries per piece, RC = 2 rows polynomials per modulus and query) into
  // dst[(q - q0)][row, comp][k][N] -- launch_slots_assemble + ntt_batch(inverse) in one pass
  hipError_t (*ntt_inv_gather)(hipStream_t st, int mode, const DevParams* P, uint32_t k, const uint64_t* src,
                               uint64_t* dst, const SliceMap& map, uint32_t RC, uint32_t nq, uint32_t nq_total,
                               uint32_t q0);
  // c0 of `cts` tree ciphertexts (doubles) into NTT form, in place: the tree keeps c0 in NTT form from the first fused
  // level on (ks_combine_c0_ntt)
  hipError_t (*tree_c0_fwd)(hipStream_t st, int mode, const DevParams* P, uint32_t k, uint64_t* tree, uint32_t cts);
};

// pack_bytes: width of the packed key-switch intermediates the kernels are built for (5, 6 or 7; ntt_kernels.hip)
// (N = 32768: one table whatever the width -- its integer kernels never store packed intermediates)
const NttOps* ntt_ops_for(uint32_t N, int pack_bytes = 5);  // nullptr for unsupported degrees

hipError_t launch_ntt_reorder(hipStream_t st, uint32_t N, const uint64_t* in, uint64_t* out, uint64_t n_polys,
                              bool to_device, bool as_f64);
// rows of `words` words: dst[dst_idx ? dst_idx[i] : i] = src[src_idx ? src_idx[i] : i] for i < n (rows src_stride /
// dst_stride words apart) -- the staging copy's touched plaintexts in and out of an update's compact buffers
hipError_t launch_copy_rows(hipStream_t st, const uint64_t* src, uint64_t* dst, const uint64_t* src_idx,
                            const uint64_t* dst_idx, uint64_t n, uint64_t words, uint64_t src_stride, uint64_t dst_stride);
// coefficient-level splice of an item update: coef[n][N] holds residue 0 of the touched plaintexts in coefficient form;
// the plain lift is undone, the bits [8 o, 8 o + 8 item_bytes) of every updated item (upd[i][s] != 0: item slot s of
// plaintext i, new bytes at img[i][s * item_bytes ..]) are replaced in the MSB-first bits-wide coefficient stream, every
// other bit is kept.  coef receives the coefficients (< t), nonzero[i] whether plaintext i has a non-zero one.
hipError_t launch_db_splice(hipStream_t st, const DevParams* P, uint64_t* coef, uint32_t N, const uint8_t* img,
                            const uint8_t* upd, uint64_t n, uint64_t bytes_per_pt, uint32_t item_bytes, uint32_t bits,
                            uint32_t* nonzero);
// u64 residues < 2^40 <-> 5 bytes each (4 words <-> 5 dwords); words must be a multiple of 4
hipError_t launch_pack40x4(hipStream_t st, const uint64_t* in, uint32_t* out, uint64_t words);
hipError_t launch_unpack40x4(hipStream_t st, const uint32_t* in, uint64_t* out, uint64_t words);
hipError_t launch_ks_combine(hipStream_t st, const DevParams* P, int mode, uint32_t N, uint32_t k,
                             const uint64_t* res_in, const uint64_t* prod, uint32_t galois_inv, uint32_t nodes,
                             uint32_t shift_pow, bool expand_step, uint32_t hi_limit, bool pack40, uint64_t* res_out,
                             int pack_bytes = 5);
// to_tree with chunk_words != 0: the input consists of chunks of chunk_words words that lie in_stride words apart
hipError_t launch_tree_convert(hipStream_t st, const DevParams* P, int mode, const uint64_t* in, uint64_t* out,
                               uint64_t words, bool to_tree, uint64_t chunk_words = 0, uint64_t in_stride = 0);
hipError_t launch_monomial_shift(hipStream_t st, const DevParams* P, uint32_t N, uint32_t k, const uint64_t* in,
                                 uint32_t shift, uint64_t count, uint64_t* out);
hipError_t launch_scan(hipStream_t st, const DevParams* P, uint32_t N, uint32_t k, const uint64_t* db,
                       const uint64_t* sv, uint64_t* out, uint32_t rows, uint32_t cols, uint64_t num_pt,
                       uint32_t nsplit, uint32_t cols_per_split, uint32_t rows_per_thread, uint32_t block,
                       bool limb);
hipError_t launch_scan_mq(hipStream_t st, const DevParams* P, uint32_t N, uint32_t k, const uint64_t* db,
                          const uint64_t* const* sv, uint64_t* const* out, uint32_t nq, uint32_t rows,
                          uint32_t cols, uint32_t rows_per_wave, bool limb);
// n_queries > 1: query q folds part + q * part_qstride into out + q * out_qstride (one launch for a group)
hipError_t launch_reduce_splits(hipStream_t st, const DevParams* P, const uint64_t* part, uint32_t nsplit,
                                uint64_t words, uint64_t* out, uint32_t n_queries = 1, uint64_t part_qstride = 0,
                                uint64_t out_qstride = 0);
// Modulus switch of n_cts coefficient-form ciphertexts [2][k][N] per query from k to r primes (1 <= r < k), k - r drop
// steps, last prime first.  compact = false: residues 0..r-1 are written where they were read (stride k kept; in == out);
// compact = true: out is [n_cts][2][r][N].  Query q reads in + q * in_qstride and writes out + q * out_qstride.
hipError_t launch_mod_switch(hipStream_t st, const DevParams* P, const uint64_t* in, uint64_t* out, uint64_t n_cts,
                             uint32_t k, uint32_t r, uint32_t N, bool compact, uint32_t n_queries = 1,
                             uint64_t in_qstride = 0, uint64_t out_qstride = 0);

// Packed replies (reply_pack.hip): n_cts ciphertexts [2][in_r][N] of canonical residues per query,
// the first r residues of each component packed to w[j] bits a coefficient, into n_cts * ct_words words per query.
// Polynomial (c, j) of a ciphertext starts at word c * ct_words / 2 + off[j] of it.  Query q reads in + q * in_qstride and
// writes out + q * out_qstride.  reply_pack_args: the argument block for the moduli q[0 .. r), w[j] = bit length of q[j] - 1.
struct ReplyPackArgs {                 // by-value kernel argument
  uint32_t N, r, in_r, ct_words;
  uint32_t off[kMaxPrimes];
  uint8_t w[kMaxPrimes];
};
ReplyPackArgs reply_pack_args(uint32_t N, const uint64_t* q, uint32_t r, uint32_t in_r);
hipError_t launch_reply_pack(hipStream_t st, const ReplyPackArgs& args, const uint64_t* in, uint64_t* out, uint64_t n_cts,
                             uint32_t n_queries = 1, uint64_t in_qstride = 0, uint64_t out_qstride = 0);

// the same for the integer flavour at N = 32768 (ntt_ring32k.hip): scratch holds canonical u64 residues (upper_ntt of
// that degree), `acc` canonical partial sums
hipError_t launch_upper_mac_int(hipStream_t st, const DevParams* P, const uint64_t* scratch, const MfmaPtrs& svq,
                                uint64_t* acc, uint64_t* out, uint32_t n_queries, uint32_t n_rows, uint32_t C,
                                uint32_t enc_count, uint32_t k, uint32_t N, uint32_t sv_first, uint32_t b0, uint32_t blk,
                                uint32_t n_dim, bool first, bool last, uint64_t acc_qstride, uint64_t out_qstride);

// split upper level, part 2: acc[query][slot][comp][jt][i] (+)= sum over the block's children of
// scratch (.) selector, elementwise; `first` starts the sums, `last` writes canonical u64 residues to `out`
// (reduce_splits' output layout) instead of keeping signed doubles in `acc`
hipError_t launch_upper_mac(hipStream_t st, const DevParams* P, const uint64_t* scratch, const MfmaPtrs& svq,
                            uint64_t* acc, uint64_t* out, uint32_t n_queries, uint32_t n_rows, uint32_t C,
                            uint32_t enc_count, uint32_t k, uint32_t N, uint32_t sv_first, uint32_t b0, uint32_t blk,
                            uint32_t n_dim, bool first, bool last, uint64_t acc_qstride, uint64_t out_qstride);

// ---- digit-sliced int8-MFMA scan (scan_mfma.hip) ----
struct MfmaGeom {
  uint32_t L;        // balanced base-256 digits per residue (5, 6, 7); 0 = not applicable
  uint32_t RT;       // row tiles (16 rows)
  uint32_t KG;       // column groups (16 columns)
  uint32_t KS;       // k-steps (64 columns) per chunk, selectors of one chunk live in registers
  uint32_t GC;       // column groups per chunk = ceil(KG / nchunks) <= 4 KS
  uint32_t nchunks;  // column chunks (grid.y); > 1 leaves partial sums to reduce_splits_kernel
  uint32_t NW;       // waves (= slots) per workgroup: 8 (two waves per SIMD, KS <= 3) or 4 (one per SIMD, KS <= 7)
  uint32_t top4;     // 1: the top digit of both operands is stored as nibbles (residues < 2^(8 (L - 1) + 4))
  uint32_t tile_bytes;  // bytes of the L digit tiles of one (row tile, column group): L * 256, or (L - 1) * 256 + 128
  size_t db_bytes, sel_bytes;
};

// wide_override: -1 = choose by width, 0 / 1 = force the 8-wave / 4-wave kernel
MfmaGeom mfma_geometry(const DevParams& hp, uint32_t rows, uint32_t cols, int wide_override = -1, bool allow_top4 = true);
// slot0 / nslots: the slots of the ring the packed copy holds (nslots = 0: all from slot0 on), local index j - slot0
hipError_t launch_db_pack(hipStream_t st, const DevParams* P, const MfmaGeom& gm, const uint64_t* db, uint8_t* dbp,
                          uint32_t rows, uint32_t cols, uint32_t kN, uint32_t slot0 = 0, uint32_t nslots = 0);
// The same for a band of whole row tiles (streamed database loads): band = u64 [npts][kN], plaintexts in row-major order
// starting at matrix row 16 * rt0 and column 0, goes to the row tiles [rt0, rt0 + n_rt) of the packed copy; what the
// band does not hold of those tiles (npts < n_rt * 16 * cols) is stored as zero.  Full-tile stores, dbp is not read.
hipError_t launch_db_pack_band(hipStream_t st, const DevParams* P, const MfmaGeom& gm, const uint64_t* band, uint8_t* dbp,
                               uint32_t rt0, uint32_t n_rt, uint64_t npts, uint32_t cols, uint32_t kN, uint32_t slot0 = 0,
                               uint32_t nslots = 0);
hipError_t launch_db_unpack(hipStream_t st, const DevParams* P, const MfmaGeom& gm, const uint8_t* dbp, uint64_t* out,
                            uint32_t row, uint32_t col, uint32_t kN);
// In-place database updates (pirgpu_db_update_*).  One unit = one touched (row, column group) of the operand layout:
// `mask` holds its touched columns (bit c: column 16 kg + c); the touched plaintexts of a unit are numbered out0,
// out0 + 1, ... in column order (the plaintext rows of the update's compact buffers).
struct DbUnit {
  uint32_t r, kg, mask, out0;
};
// residue 0 (slots [0, N)) of every touched plaintext back from the operand layout: out[plaintext][N], in [0, q_0)
hipError_t launch_db_gather(hipStream_t st, const DevParams* P, const MfmaGeom& gm, const uint8_t* dbp,
                            const DbUnit* units, uint32_t n_units, uint64_t* out, uint32_t N);
// the partial twin of launch_db_pack: enc[plaintext][kN] (device order) into the touched columns of the operand layout,
// slots [slot0, slot0 + nslots) only; every other byte keeps its value
hipError_t launch_db_pack_update(hipStream_t st, const DevParams* P, const MfmaGeom& gm, const uint64_t* enc,
                                 const DbUnit* units, uint32_t n_units, uint8_t* dbp, uint32_t kN, uint32_t slot0,
                                 uint32_t nslots);
// map: the output cut into per-rank pieces by slot ranges (nullptr: one piece)
hipError_t launch_sel_pack(hipStream_t st, const DevParams* P, const MfmaGeom& gm, const MfmaPtrs& sv, uint32_t nq,
                           uint8_t* selp, uint32_t cols, uint32_t kN, bool sel_f64 = false, const SliceMap* map = nullptr);
// wgs: persistent workgroups of the launch (0 = one per CU; the batch pipeline asks for fewer, see scan_mfma.hip)
// f64_fold: fold the digit diagonals in exact fp64 arithmetic (every data modulus below 2^50)
// one group of nq <= 8 queries over the whole ring; query q writes [rows][2][kN] at out + q * out_qstride
hipError_t launch_scan_mfma(hipStream_t st, const DevParams* P, const MfmaGeom& gm, const uint8_t* dbp,
                            const uint8_t* selp, uint64_t* out, uint64_t out_qstride, uint32_t nq, uint32_t rows,
                            uint32_t kN, uint64_t chunk_stride, uint32_t wgs = 0, bool f64_fold = false);
// several groups over the slots [slot0, slot0 + nslots) in one launch (dbp / selectors / output indexed by local slot,
// an output row is out_rstride slots long)
hipError_t launch_scan_mfma_groups(hipStream_t st, const DevParams* P, const MfmaGeom& gm, const uint8_t* dbp,
                                   const ScanGroups& grp, uint32_t rows, uint64_t chunk_stride, uint32_t wgs, bool f64_fold,
                                   uint32_t slot0, uint32_t nslots, uint64_t out_qstride, uint32_t out_rstride,
                                   bool blk_major = false);   // blk_major: units ordered (slot block, group) instead of (group, slot block)
// TWO groups per database read (scan_mfma_pair.hip): grp holds exactly two groups, which share every tile a unit loads,
// the second one's selectors in LDS.  Same arguments; scan_mfma_pair_supported: the geometries it is built for (L = 5,
// 8 waves, one chunk) -- and only the whole ring, group-major (slot0 = 0, out_rstride = nslots, blk_major = false),
// grp.n = 2.  Anything else is hipErrorInvalidValue: the caller launches single passes.
bool scan_mfma_pair_supported(const MfmaGeom& gm);
hipError_t launch_scan_mfma_pair(hipStream_t st, const DevParams* P, const MfmaGeom& gm, const uint8_t* dbp,
                                 const ScanGroups& grp, uint32_t rows, uint64_t chunk_stride, uint32_t wgs, bool f64_fold,
                                 uint32_t slot0, uint32_t nslots, uint64_t out_qstride, uint32_t out_rstride,
                                 bool blk_major = false);
// several groups over the whole ring, each over ITS OWN database grp.db[g] (the runs of equal tables inside one batch
// group); scan_mfma_runs_supported: the geometries the launch is built for (the 8-wave kernels) -- others launch per run
bool scan_mfma_runs_supported(const MfmaGeom& gm);
hipError_t launch_scan_mfma_runs(hipStream_t st, const DevParams* P, const MfmaGeom& gm, const ScanGroupsDb& grp,
                                 uint32_t rows, uint32_t kN, uint64_t chunk_stride, uint32_t wgs, bool f64_fold,
                                 uint64_t out_qstride);
// row sums of queries q0 .. q0 + nq - 1 (of the nq_total the receive buffer holds per rank) back from the per-rank slot
// pieces of the all-to-all receive buffer to [query][row, comp][kN] at dst + (q - q0) * dst_qstride
hipError_t launch_slots_assemble(hipStream_t st, const uint64_t* src, uint64_t* dst, const SliceMap& map, uint32_t RC,
                                 uint32_t kN, uint32_t nq, uint64_t dst_qstride, uint32_t nq_total, uint32_t q0);

// Seed expansion (seed_expand.hip): object o of n_obj re-samples SEAL's sample_poly_uniform from
// seeds[o][64] over mod[0 .. n_mod) into out + o * obj_stride, [n_mod][N] canonical residues; one workgroup of
// kSeedThreads per object.  stats[0] += draws rejected, stats[1] = 1 if an object needed more than max_refills refills.
constexpr uint32_t kSeedThreads = 512;
struct SeedExpandArgs {                // by-value kernel argument
  ModConst mod[kMaxMod];
  uint64_t max_multiple[kMaxMod];      // (2^63 - 1) - ((2^63 - 1) mod q) - 1: candidates below it are accepted
  uint64_t max_refills;                // bound on the stream an object may consume (a workgroup never spins)
  uint32_t n_mod, N;
};
hipError_t launch_seed_expand(hipStream_t st, const SeedExpandArgs& args, const uint8_t* seeds, uint32_t n_obj, uint64_t* out,
                              uint64_t obj_stride, uint64_t* stats);

// Compact queries (query_expand.hip): n_cts compact ciphertexts per query, obj_words words each --
// polynomial j of c0 as N w[j] / 64 words at off[j] (w[j] = 64: plain words), then the 8 seed words -- at
// in[query][ct][obj_words].  Ciphertext ct of query q gets its c0 half, [k][N] canonical residues, at
// out + q * out_qstride + ct * ct_stride, and its seed at seeds[(q * n_cts + ct) * 8]; the c1 half is launch_seed_expand's.
// query_unpack_args: the argument block for the moduli q[0 .. k), packed ? w[j] = bit length of q[j] - 1 : 64.
struct QueryUnpackArgs {               // by-value kernel argument
  uint32_t N, k, obj_words;
  uint32_t off[kMaxPrimes];
  uint8_t w[kMaxPrimes];
};
QueryUnpackArgs query_unpack_args(uint32_t N, const uint64_t* q, uint32_t k, bool packed);
hipError_t launch_query_unpack(hipStream_t st, const QueryUnpackArgs& args, const uint64_t* in, uint64_t* out, uint64_t* seeds,
                               uint32_t n_cts, uint64_t ct_stride, uint32_t n_queries = 1, uint64_t out_qstride = 0);

}  // namespace pirgpu
