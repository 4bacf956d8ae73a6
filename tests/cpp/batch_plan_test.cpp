// batch_plan_test.cpp -- the batch pipeline's planning logic (pir_amd/csrc/batch_plan.h) on the host: the group walk
// against a restatement of the nested loop it replaced, the pairing rule, the order of a batch that names tables and the
// leading-replies bookkeeping.  Stand-alone; built and run under AddressSanitizer + UBSan by tests/test_batch_plan.py.
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../pir_amd/csrc/batch_plan.h"

using namespace pirgpu;

static int g_failed = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                        \
    }                                                                    \
  } while (0)

// The loop batch_run_mfma walked before the plan existed, stated literally: the group count first, then the groups, with
// `run_pair(first_a, n_a, first_b, n_b)` and the single-group body recorded as steps.
static GroupWalk old_walk(uint32_t count, uint32_t span, uint32_t step, bool may_pair) {
  GroupWalk w;
  for (uint32_t rank0 = 0; rank0 < count; rank0 += span) {
    const uint32_t in_span = std::min<uint32_t>(span, count - rank0);
    w.n_groups += (in_span + step - 1) / step;
  }
  for (uint32_t rank0 = 0; rank0 < count; rank0 += span) {
    const uint32_t in_span = std::min<uint32_t>(span, count - rank0);
    for (uint32_t j0 = 0; j0 < in_span; j0 += step) {
      const uint32_t B = std::min<uint32_t>(step, in_span - j0);
      if (may_pair && j0 + step < in_span) {   // a full group and whatever follows it
        w.steps.push_back(GroupStep{{rank0 + j0, rank0 + j0 + step}, {B, std::min<uint32_t>(step, in_span - j0 - step)}});
        j0 += step;
        continue;
      }
      w.steps.push_back(GroupStep{{rank0 + j0, 0}, {B, 0}});
    }
  }
  return w;
}

static void test_walk() {
  unsigned cases = 0, pairs = 0;
  for (uint32_t count = 1; count <= 80; ++count)
    for (uint32_t span : {count, 1u, 3u, 8u, 9u, 16u, 24u})
      for (uint32_t step : {1u, 4u, 8u})
        for (int pair = 0; pair < 2; ++pair) {
          const GroupWalk want = old_walk(count, span, step, pair), got = plan_group_walk(count, span, step, pair);
          CHECK(got.n_groups == want.n_groups);
          CHECK(count_groups(count, span, step) == want.n_groups);
          CHECK(got.steps.size() == want.steps.size());
          uint32_t covered = 0, groups = 0;
          for (size_t i = 0; i < got.steps.size() && i < want.steps.size(); ++i) {
            const GroupStep &g = got.steps[i], &o = want.steps[i];
            CHECK(g.first[0] == o.first[0] && g.n[0] == o.n[0] && g.n[1] == o.n[1] && (!o.n[1] || g.first[1] == o.first[1]));
            // what the loop guaranteed: every query once and in order, full first halves, no step across a span boundary
            CHECK(g.first[0] == covered && g.n[0] >= 1 && g.n[0] <= step);
            if (g.n[1]) CHECK(pair && g.n[0] == step && g.first[1] == covered + step && g.n[1] <= step);
            CHECK(g.first[0] / span == (g.first[0] + g.n[0] + g.n[1] - 1) / span);
            covered += g.n[0] + g.n[1];
            groups += g.n[1] ? 2 : 1;
            pairs += g.n[1] != 0;
          }
          CHECK(covered == count && groups == got.n_groups);
          ++cases;
        }
  CHECK(cases == 80 * 7 * 3 * 2 && pairs > 0);
  // the shapes the headline and the packed exchange queue
  const GroupWalk h = plan_group_walk(64, 64, 8, true);
  CHECK(h.n_groups == 8 && h.steps.size() == 4 && h.steps[3].first[0] == 48 && h.steps[3].first[1] == 56);
  const GroupWalk odd = plan_group_walk(19, 19, 8, true);   // 8 + 8 paired, 3 alone
  CHECK(odd.n_groups == 3 && odd.steps.size() == 2 && odd.steps[0].n[1] == 8 && odd.steps[1].first[0] == 16 &&
        odd.steps[1].n[0] == 3 && odd.steps[1].n[1] == 0);
  const GroupWalk ranks = plan_group_walk(27, 9, 8, false);   // three source ranks of 9: 8 + 1 each
  CHECK(ranks.n_groups == 6 && ranks.steps[1].first[0] == 8 && ranks.steps[1].n[0] == 1 && ranks.steps[2].first[0] == 9);
  CHECK(plan_group_walk(0, 0, 8, true).steps.empty() && count_groups(5, 5, 0) == 0);
}

static void test_pairing_rule() {
  for (uint32_t groups : {3u, 4u})
    for (uint32_t lanes : {1u, 2u}) {
      CHECK(!pair_by_count(0, groups, lanes));                                  // off
      CHECK(pair_by_count(1, groups, lanes) == (groups == 4 && lanes == 2));    // long calls on two lanes only
      CHECK(pair_by_count(2, groups, lanes));                                   // wherever two groups are left
    }
  CHECK(pair_by_count(1, 8, 2) && !pair_by_count(1, 8, 1) && pair_by_count(3, 1, 1));
}

static void test_workers_and_lanes() {
  CHECK(active_workers(0, 0) == 1 && active_workers(16, 4) == 4 && active_workers(4, 16) == 4 && active_workers(0, 8) == 1);
  CHECK(lanes_in_use(16, 8, 2) == 2 && lanes_in_use(15, 8, 2) == 1 && lanes_in_use(1, 1, 2) == 1 && lanes_in_use(32, 8, 2) == 2);
  CHECK(lanes_in_use(4, 8, 2) == 1 && lanes_in_use(4, 0, 2) == 2 && lanes_in_use(16, 8, 0) == 1);
}

static void test_table_runs() {
  // sorted batch: the identity, runs cut at table changes and at every multiple of the group
  {
    const std::vector<uint32_t> t = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 2, 2, 2, 2, 2};
    const TablePlan tp = plan_table_runs(t.data(), (uint32_t)t.size(), 8);
    CHECK(tp.identity);
    for (uint32_t i = 0; i < t.size(); ++i) CHECK(tp.order[i] == i);
    CHECK((tp.run_begin == std::vector<uint32_t>{0, 8, 10, 12, 16, 19}));
  }
  // stable among equal tables, for every group size; every multiple of the group begins a run
  {
    const std::vector<uint32_t> t = {3, 1, 3, 0, 1, 3, 3, 0, 1, 1, 3, 3, 3, 3, 3, 3, 3};
    for (uint32_t group : {1u, 2u, 3u, 8u, 32u}) {
      const TablePlan tp = plan_table_runs(t.data(), (uint32_t)t.size(), group);
      CHECK(!tp.identity && tp.order.size() == t.size());
      for (uint32_t i = 1; i < t.size(); ++i) {
        CHECK(t[tp.order[i - 1]] <= t[tp.order[i]]);
        if (t[tp.order[i - 1]] == t[tp.order[i]]) CHECK(tp.order[i - 1] < tp.order[i]);
      }
      CHECK(tp.run_begin.front() == 0 && tp.run_begin.back() == t.size());
      for (uint32_t i = 1; i < t.size(); ++i) {
        const bool cut = std::binary_search(tp.run_begin.begin(), tp.run_begin.end(), i);
        CHECK(cut == (i % group == 0 || t[tp.order[i]] != t[tp.order[i - 1]]));
      }
    }
    CHECK(plan_table_runs(t.data(), 0, 8).run_begin == std::vector<uint32_t>{0});
    CHECK(plan_table_runs(t.data(), 3, 0).run_begin.size() == 4);   // group 0 counts as 1
  }
  // the batch of tests/test_gpu_tables.py (ISSUE_BATCH), worked out by hand: its served order, its runs, and what its
  // three groups of 8 report as complete
  {
    const std::vector<uint32_t> t = {2, 0, 1, 1, 0, 2, 2, 2, 2, 2, 2, 2, 2, 2, 0, 1, 2, 0, 1};
    const TablePlan tp = plan_table_runs(t.data(), (uint32_t)t.size(), 8);
    CHECK(!tp.identity);
    CHECK((tp.order == std::vector<uint32_t>{1, 4, 14, 17, 2, 3, 15, 18, 0, 5, 6, 7, 8, 9, 10, 11, 12, 13, 16}));
    CHECK((tp.run_begin == std::vector<uint32_t>{0, 4, 8, 16, 19}));
    const GroupWalk w = plan_group_walk(19, 19, 8, false);
    CHECK(w.steps.size() == 3);
    LeadingReplies lead(19);
    std::vector<uint32_t> reported;
    for (const GroupStep& g : w.steps) reported.push_back(lead.mark(tp.order.data() + g.first[0], g.n[0]));
    CHECK((reported == std::vector<uint32_t>{0, 12, 19}));
  }
  // an unpermuted batch reports the ends of its groups
  {
    LeadingReplies lead(19);
    const uint32_t ids[19] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18};
    CHECK(lead.mark(ids, 8) == 8 && lead.mark(ids + 8, 8) == 16 && lead.mark(ids + 16, 3) == 19 && lead.mark(ids, 0) == 19);
  }
}

int main() {
  test_walk();
  test_pairing_rule();
  test_workers_and_lanes();
  test_table_runs();
  if (g_failed) {
    fprintf(stderr, "%d checks failed\n", g_failed);
    return 1;
  }
  printf("batch_plan_test OK\n");
  return 0;
}
