// batch_plan.h -- what the batch pipeline (ctx.hip, sections [8] and [9]) decides from numbers alone: how a call is cut
// into groups, pairs and lanes, the order a batch that names tables is served in, and how many leading replies of such a
// batch are complete.  Host only: no HIP, no context, so that tests/cpp/batch_plan_test.cpp can pin it without a GPU.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace pirgpu {

// Contexts with tables: the order a batch is served in.  The queries are sorted by table (stable: equal tables keep their
// submission order) so that equal tables meet in the same group of `group` queries; order[i] = the staged query served at
// position i.  A RUN is a maximal stretch of positions with one table inside one group: run r covers the positions
// [run_begin[r], run_begin[r + 1]) and is scanned against its table's operand layout.  Host only, no device state.
struct TablePlan {
  std::vector<uint32_t> order, run_begin;
  bool identity = true;   // order[i] == i: the batch is served exactly as a batch without tables
};
inline TablePlan plan_table_runs(const uint32_t* tables, uint32_t count, uint32_t group) {
  TablePlan tp;
  tp.order.resize(count);
  for (uint32_t i = 0; i < count; ++i) tp.order[i] = i;
  std::stable_sort(tp.order.begin(), tp.order.end(), [&](uint32_t a, uint32_t b) { return tables[a] < tables[b]; });
  group = std::max<uint32_t>(group, 1);
  for (uint32_t i = 0; i < count; ++i) {
    tp.identity = tp.identity && tp.order[i] == i;
    if (i == 0 || i % group == 0 || tables[tp.order[i]] != tables[tp.order[i - 1]]) tp.run_begin.push_back(i);
  }
  tp.run_begin.push_back(count);
  return tp;
}
// Workers a call may use: what pirgpu_set_concurrency asked for, of those that exist, at least one.
inline uint32_t active_workers(uint32_t n_active, uint32_t n_workers) { return std::max<uint32_t>(1, std::min(n_active, n_workers)); }
// Lanes that groups of G queries alternate between: a group's members are lane-bound (stream order on the lane covers
// the reuse of their buffers), so with fewer than 2 x G workers every group uses lane 0.
inline uint32_t lanes_in_use(uint32_t W, uint32_t G, uint32_t n_lanes) {
  return std::max<uint32_t>(1, std::min<uint32_t>(n_lanes, W / std::max<uint32_t>(G, 1)));
}
// One step of a call's walk: n[0] queries from first[0] on, or -- n[1] != 0 -- two groups that share one database pass.
struct GroupStep { uint32_t first[2], n[2]; };
struct GroupWalk {
  std::vector<GroupStep> steps;
  uint32_t n_groups = 0;   // groups the call queues, paired or not
};
// Groups of a call of `count` queries: runs of up to `step` consecutive queries that never cross a multiple of `span`
// (packed input: what one source rank sent; otherwise span = count).
inline uint32_t count_groups(uint32_t count, uint32_t span, uint32_t step) {
  uint32_t n = 0;
  for (uint32_t s0 = 0; span && step && s0 < count; s0 += span) n += (std::min<uint32_t>(span, count - s0) + step - 1) / step;
  return n;
}
// The walk, in the order the groups are queued.  With `pair` a full group and whatever follows it in the same span form
// one step; an odd last group of a span stays single.
inline GroupWalk plan_group_walk(uint32_t count, uint32_t span, uint32_t step, bool pair) {
  GroupWalk w;
  w.n_groups = count_groups(count, span, step);
  for (uint32_t s0 = 0; span && step && s0 < count; s0 += span) {
    const uint32_t in_span = std::min<uint32_t>(span, count - s0);
    for (uint32_t j0 = 0; j0 < in_span; j0 += step) {
      GroupStep g{{s0 + j0, 0}, {std::min<uint32_t>(step, in_span - j0), 0}};
      if (pair && j0 + step < in_span) {
        j0 += step;
        g.first[1] = s0 + j0;
        g.n[1] = std::min<uint32_t>(step, in_span - j0);
      }
      w.steps.push_back(g);
    }
  }
  return w;
}
// The part of the pairing rule (PIRGPU_SCAN_MFMA_PAIR = scan_pair) that depends on counts alone: 0 never, 2 wherever a
// call has two groups left, 1 only in calls of four groups or more on two lanes (a shorter call keeps the finer pipeline).
inline bool pair_by_count(uint32_t scan_pair, uint32_t n_groups, uint32_t lanes) {
  return scan_pair >= 2 || (scan_pair && n_groups >= 4 && lanes >= 2);
}

// A batch served in another order than it was submitted: mark() notes the submission indices whose replies a group has
// queued and returns how many LEADING queries of the batch are complete with them.
struct LeadingReplies {
  std::vector<uint8_t> queued;
  uint32_t lead = 0;
  explicit LeadingReplies(uint32_t count) : queued(count, 0) {}
  uint32_t mark(const uint32_t* idx, uint32_t n) {
    for (uint32_t q = 0; q < n; ++q) queued[idx[q]] = 1;
    while (lead < queued.size() && queued[lead]) ++lead;
    return lead;
  }
};

}  // namespace pirgpu
