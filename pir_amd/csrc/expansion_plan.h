// expansion_plan.h -- what the oblivious expansion (ctx.hip, section [3]: expand_core) decides from numbers alone: which
// form every level of a group's tree runs in, how the tree is stored between two levels and where the walk may be cut
// between the head stream and a lane.  Host only: no HIP, no context, so that tests/cpp/expansion_plan_test.cpp can walk
// the whole domain without a GPU.  expand_core launches from these records and decides nothing itself.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "device_params.h"

namespace pirgpu {

constexpr uint32_t kKsWideLevel = 256;   // nodes per launch from which the key-switch kernels use the XCD-aware 1-D grid
inline bool ks_digit_takes_c0(uint32_t nodes) { return nodes >= kKsWideLevel && nodes % 8 == 0; }

// The resolved options of a context that shape the walk (ctx.hip, resolve_options).
struct ExpandOptions {
  int mode = kNttF64;               // arithmetic flavour (NttMode); the integer flavour has unfused levels only
  bool fuse_last_level = true;      // FUSE_LAST
  bool last_level_ntt = true;       // LAST_NTT
  bool fuse_mac_combine = true;     // FUSE_MAC_COMBINE
  uint32_t fuse_mac_nodes = 128;    // tree ciphertexts per level from which a single query's levels are fused
  bool tree40 = true;               // TREE40
  bool pack40 = true;               // PACK40
  bool c0_ntt = false;              // C0_NTT = 1 / 2
  bool c0_ntt_split = false;        // C0_NTT = 2
  bool loop_transforms = true;      // LOOP_TRANSFORMS (off in the integer flavour)
  uint32_t loop_min_sources = 1024;
};

// How a tree in the middle of its expansion is stored (the flags of ctx.hip's TreeState).
struct TreeFlags {
  bool cur40 = false;   // 5-byte polynomials instead of doubles
  bool c0ntt = false;   // c0 polynomials in NTT form
};

enum ExpandForm : uint32_t {
  kLevelUnfused = 0,     // ks_digit, ks_mac_intt over all moduli, ks_combine
  kLevelFused = 1,       // ks_digit, special-prime product, ks_mac_combine
  kLevelLastNtt = 2,     // last level in the NTT domain (ks_last_ntt)
  kLevelLastCoeff = 3,   // last level in coefficient form, fused with the selectors' forward transform (ks_last_level)
};
// Why a record cannot be launched: the three internal errors of expand_core.
enum ExpandInvalid : uint32_t {
  kLevelValid = 0,
  kTree40Unreadable = 1,   // "5-byte tree reached a level that cannot read it"
  kTree40Unfused = 2,      // "5-byte tree reached an unfused level"
  kC0NttUnfused = 3,       // "NTT-form c0 reached an unfused level"
};

struct ExpandLevel {
  uint32_t j = 0, nodes = 0;          // level and its tree ciphertexts (2^j * B)
  ExpandForm form = kLevelUnfused;
  ExpandInvalid invalid = kLevelValid;   // != 0: the walk ends with this record
  bool tin40 = false, tout40 = false;    // the tree is read / written as 5-byte polynomials
  bool c0_in_digit = false;              // ks_digit also transforms the nodes' c0 (NTT-domain last level)
  bool loop_targets = false;             // looped transforms in ks_digit
  bool c0ntt_in = false;                 // c0 of the incoming tree is in NTT form
  bool c0_before = false;                // ... it is converted in place before the level's launches
  bool c0_after = false;                 // the level's outputs get their c0 converted (the next level is a fused one)
  bool c0ntt_out = false;                // c0 of the tree this level leaves (c0_after included)
  uint32_t mac_base = 0, mac_count = 0;  // moduli of ks_mac_intt's inverse transforms
  uint32_t hi_limit = UINT32_MAX;        // ks_combine: outputs from here on are not written (n * B on the last level)
  bool c0ntt() const { return c0ntt_in || c0_before; }   // what the level's kernels read
};

constexpr uint32_t kMaxExpandLevels = 16;   // n <= N <= 32768: at most 15 levels
// (a fixed array: expand_core plans on every call, and the CPU test plans a hundred million walks)
struct ExpandLevels {
  ExpandLevel v[kMaxExpandLevels];
  uint32_t count = 0;
  void push_back(const ExpandLevel& L) { v[count++] = L; }
  const ExpandLevel* begin() const { return v; }
  const ExpandLevel* end() const { return v + count; }
  const ExpandLevel& operator[](uint32_t i) const { return v[i]; }
  const ExpandLevel& back() const { return v[count - 1]; }
  uint32_t size() const { return count; }
  bool empty() const { return count == 0; }
};
struct ExpandPlan {
  ExpandLevels levels;
  TreeFlags out;               // how the tree is stored after the last planned level
  bool leaves_owed = true;     // the caller still owes the forward transform of the leaves (no fused last level ran)
  bool valid() const { return levels.empty() || levels.back().invalid == kLevelValid; }
};

inline uint32_t expansion_depth(uint32_t n) {
  uint32_t l = 0;
  while (l < 32 && (1ull << l) < n) ++l;
  return l;
}

// Levels [j_begin, j_end) (j_end clamped to the depth) of a group of B queries expanding n slots each.  sel_dst: the
// selectors are produced by the last level (every caller but pirgpu_expand).  from: the tree was left by the earlier
// levels on another stream -- that buffer is read-only, so its c0 is never converted in place.
inline ExpandPlan plan_expansion(uint32_t N, uint32_t logN, uint32_t k, uint32_t B, uint32_t n, bool sel_dst,
                                 const ExpandOptions& o, uint32_t j_begin = 0, uint32_t j_end = UINT32_MAX,
                                 const TreeFlags* from = nullptr) {
  ExpandPlan p;
  const bool fp64 = o.mode != kNttInt;
  const uint32_t logm = expansion_depth(n);
  const bool fuse_last = sel_dst && fp64 && o.fuse_last_level;
  bool cur40 = from ? from->cur40 : false, c0ntt = from ? from->c0ntt : false;
  const uint32_t j_stop = std::min(std::min(j_end, logm), j_begin + kMaxExpandLevels);
  // c0 in NTT form through the fused levels: only for a tree whose leaves are consumed in NTT form by the last level
  const bool c0_path = o.c0_ntt && fuse_last && o.last_level_ntt && fp64 && o.fuse_mac_combine;
  // (a group of B queries reaches the width at which the fused form pays one level earlier than a single query:
  // measured +0.6 % batched with the threshold at 64 tree ciphertexts, while a single query loses latency below 128)
  const uint32_t fuse_from = B > 1 ? std::max<uint32_t>(o.fuse_mac_nodes / 2, 1) : o.fuse_mac_nodes;
  auto level_fused = [&](uint32_t j) {
    return fp64 && o.fuse_mac_combine && ((uint64_t)B << j) >= fuse_from && !(fuse_last && j + 1 == logm);
  };
  for (uint32_t j = j_begin; j < j_stop; ++j) {
    ExpandLevel L;
    L.j = j;
    L.nodes = B << j;
    const bool last = j + 1 == logm;
    const bool last_ntt = fuse_last && last && o.last_level_ntt;
    L.tin40 = cur40;
    L.c0ntt_in = c0ntt;
    L.c0_in_digit = last_ntt && !c0ntt && ks_digit_takes_c0(L.nodes);
    L.loop_targets = fp64 && o.loop_transforms && (uint64_t)L.nodes * k >= o.loop_min_sources;
    if (cur40 && last_ntt && !(c0ntt || L.c0_in_digit)) {
      L.form = kLevelLastNtt;
      L.invalid = kTree40Unreadable;
      p.levels.push_back(L);
      break;
    }
    // the root enters a fused level directly (a group wide enough at level 0): its c0 goes to NTT form in place
    if (c0_path && !c0ntt && level_fused(j) && !cur40 && !(from && j == j_begin)) {
      L.c0_before = true;
      c0ntt = true;
    }
    if (level_fused(j)) {
      // between two fused levels (and into the NTT-domain last level) the tree is written as 5-byte polynomials, as long
      // as one transform workgroup's threads cover a level's nodes
      const uint32_t next_nodes = L.nodes * 2;
      const bool next_last = j + 2 == logm;
      const bool next_reads40 = next_last ? (fuse_last && o.last_level_ntt && (c0ntt || ks_digit_takes_c0(next_nodes)))
                                          : (next_nodes >= fuse_from);
      L.form = kLevelFused;
      L.tout40 = o.tree40 && o.pack40 && j + 1 < logm && next_reads40 && (1u << j) < (N >> ntt_log_ept((int)logN));
      L.mac_base = k;
      L.mac_count = 1;
      L.c0ntt_out = c0ntt;
      p.levels.push_back(L);
      cur40 = L.tout40;
      continue;
    }
    if ((cur40 || c0ntt) && !last_ntt) {
      L.invalid = cur40 ? kTree40Unfused : kC0NttUnfused;
      p.levels.push_back(L);
      break;
    }
    if (last_ntt) {
      L.form = kLevelLastNtt;
      L.mac_base = k;
      L.mac_count = 1;
      L.c0ntt_out = c0ntt;
      p.levels.push_back(L);
      p.leaves_owed = false;
      break;
    }
    L.mac_base = 0;
    L.mac_count = k + 1;
    if (fuse_last && last) {
      L.form = kLevelLastCoeff;
      p.levels.push_back(L);
      p.leaves_owed = false;
      break;
    }
    // outputs n * B .. of the last level are never read (only the first n results per query are used)
    L.form = kLevelUnfused;
    L.hi_limit = last ? n * B : UINT32_MAX;
    // the next level is a fused one: this (narrow) level's outputs, in the stream's own buffer, get their c0 transformed
    if (c0_path && j + 1 < logm && level_fused(j + 1)) {
      L.c0_after = true;
      c0ntt = true;
    }
    L.c0ntt_out = c0ntt;
    p.levels.push_back(L);
  }
  p.out.cur40 = cur40;
  p.out.c0ntt = c0ntt;
  return p;
}

// Whether a group's first `head_levels` levels run on the head stream (expand_group_on_lane): one query ciphertext per
// query (query_cts = dim_sum / N + 1 == 1), a real group, and at least two levels left for the lane.  head_enabled: what
// HEAD_MODE and the way the batch was staged say (mode 2, or mode 1 and an asynchronously staged batch).
inline bool expansion_uses_head(uint32_t query_cts, uint32_t B, uint32_t head_levels, bool head_enabled, uint32_t depth) {
  return query_cts == 1 && B > 1 && head_levels > 0 && head_enabled && depth >= head_levels + 2;
}

// One level as pirgpu_expansion_forms reports it (the layout is documented in include/pirgpu.h).
inline uint32_t pack_expand_level(const ExpandLevel& L, bool on_head, bool sel_f64) {
  return (uint32_t)L.form | (L.tin40 ? 1u << 2 : 0) | (L.tout40 ? 1u << 3 : 0) | (L.c0_in_digit ? 1u << 4 : 0) |
         (L.loop_targets ? 1u << 5 : 0) | (L.c0ntt() ? 1u << 6 : 0) | (L.c0ntt_out ? 1u << 7 : 0) |
         (L.c0_before ? 1u << 8 : 0) | (L.c0_after ? 1u << 9 : 0) | (L.hi_limit != UINT32_MAX ? 1u << 10 : 0) |
         (L.mac_count == 1 ? 1u << 11 : 0) | (on_head ? 1u << 12 : 0) | ((uint32_t)L.invalid << 13) |
         (sel_f64 ? 1u << 15 : 0) | (L.j << 16);
}

}  // namespace pirgpu
