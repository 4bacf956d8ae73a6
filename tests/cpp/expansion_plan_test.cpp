// expansion_plan_test.cpp -- the oblivious expansion's per-level plan (pir_amd/csrc/expansion_plan.h) on the host: the
// invariants that make expand_core's three internal errors unreachable, over the whole domain of rings, group sizes, slot
// counts, option switches and head splits; the forms restated from the rule table; and a table of walks pinned by hand.
// Stand-alone; built and run under AddressSanitizer + UBSan by tests/test_expansion_plan.py.
//
//   expansion_plan_test                       the checks (exit code 0 and "expansion_plan_test OK")
//   expansion_plan_test --reachable N k n...  no checks: the (form, tin40, tout40, c0_in_digit, loop_targets, c0ntt)
//                                             combinations reachable at ring (N, k) for B = 1 .. 8 and the listed n, per
//                                             option setting of tests/test_gpu_expansion_forms.py, unsplit and split at
//                                             1 .. 8 -- what that file's coverage condition is measured against
//
// The domain.  N in {2048, 4096, 8192, 16384} in the fp64 flavours plus the integer flavour at 4096 and 32768; k = 1 .. 4;
// B = 1 .. 8; selectors produced, or not for B = 1 (only pirgpu_expand, a single-query call, expands without them); every
// split point 0 .. 8 wherever the head rule allows it.  The full product with every n and every combination of switches
// is about 10^9 walks -- the first version of this program ran 1.4 * 10^8 of them in seven and a half minutes under the
// sanitizers -- so it is cut in two tiers:
//   tier 1  every n = 1 .. N for N <= 4096 (fp64 2048 and 4096, integer 4096): every k with the defaults; k = 2 with every
//           switch flipped alone, all of them flipped, and C0_NTT = 1 / 2 (k moves the loop threshold and nothing else);
//   tier 2  every ring and every k, with EVERY combination of the six boolean switches x C0_NTT in {0, 1, 2} at every n
//           within 2 of a power of two, and the settings of tier 1 at 64 random n; fuse_mac_nodes in {16, 2} and
//           loop_min_sources = 64 (the library keeps them at 128 and 1024; the small ones make the root enter a fused
//           level) with the defaults and with FUSE_LAST, LAST_NTT or TREE40 off, each x C0_NTT in {0, 1, 2}.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "../../pir_amd/csrc/expansion_plan.h"

using namespace pirgpu;

static int g_failed = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      if (g_failed < 40) fprintf(stderr, "%s:%d: CHECK failed: %s  [%s]\n", __FILE__, __LINE__, #cond, where()); \
      ++g_failed;                                                        \
    }                                                                    \
  } while (0)
// where a failing check was: a pinned row's name, or the point of the domain (formatted only when a check fails)
static struct { const char* row; uint32_t N, k, B, n, split; int mode, sel; const char* opt; } g_at = {nullptr, 0, 0, 0, 0, 0, 0, 0, ""};
static const char* where() {
  static char buf[256];
  if (g_at.row) snprintf(buf, sizeof buf, "pinned row '%s'", g_at.row);
  else snprintf(buf, sizeof buf, "N=%u mode=%d k=%u B=%u n=%u selectors=%d options=%s split=%u", g_at.N, g_at.mode, g_at.k, g_at.B, g_at.n, g_at.sel, g_at.opt, g_at.split);
  return buf;
}

struct Ring { uint32_t N, logN; int mode; };
static const Ring kRings[] = {{2048, 11, kNttF64}, {4096, 12, kNttF64}, {8192, 13, kNttF64Wide}, {16384, 14, kNttF64},
                              {4096, 12, kNttInt}, {32768, 15, kNttInt}};

// residues a transform thread holds, restated (device_params.h: 16 below N = 32768, 1 there)
static uint32_t log_ept(uint32_t logN) { return logN >= 15 ? 0 : 4; }
static uint32_t depth_of(uint32_t n) {
  uint32_t l = 0;
  while ((1ull << l) < n) ++l;
  return l;
}

struct Walk {
  ExpandLevels rec;
  uint32_t split = 0;        // index of the lane's first record (0: unsplit)
  TreeFlags handed;          // what the head handed over
  bool leaves_owed = true;
};

static Walk walk(const Ring& r, uint32_t k, uint32_t B, uint32_t n, bool sel, const ExpandOptions& o, uint32_t h) {
  Walk w;
  if (h == 0) {
    const ExpandPlan p = plan_expansion(r.N, r.logN, k, B, n, sel, o);
    w.rec = p.levels;
    w.leaves_owed = p.leaves_owed;
    return w;
  }
  const ExpandPlan head = plan_expansion(r.N, r.logN, k, B, n, sel, o, 0, h);
  w.rec = head.levels;
  w.split = w.rec.size();
  w.handed = head.out;
  CHECK(head.leaves_owed && head.levels.size() == h);
  const ExpandPlan lane = plan_expansion(r.N, r.logN, k, B, n, sel, o, h, UINT32_MAX, &head.out);
  for (const ExpandLevel& L : lane.levels)
    if (w.rec.size() < kMaxExpandLevels) w.rec.push_back(L);
  w.leaves_owed = lane.leaves_owed;
  return w;
}

// The rule table of the expansion, restated: which form level j takes.
static ExpandForm form_by_rule(const Ring& r, uint32_t B, uint32_t n, bool sel, const ExpandOptions& o, uint32_t j) {
  const bool fp64 = r.mode != kNttInt, last = j + 1 == depth_of(n);
  const bool fused_last = sel && fp64 && o.fuse_last_level;
  if (last && fused_last) return o.last_level_ntt ? kLevelLastNtt : kLevelLastCoeff;
  const uint32_t from = B > 1 ? (o.fuse_mac_nodes / 2 ? o.fuse_mac_nodes / 2 : 1) : o.fuse_mac_nodes;
  return fp64 && o.fuse_mac_combine && (B << j) >= from ? kLevelFused : kLevelUnfused;
}

static void check_walk(const Ring& r, uint32_t k, uint32_t B, uint32_t n, bool sel, const ExpandOptions& o, const Walk& w) {
  const uint32_t logm = depth_of(n);
  CHECK(w.rec.size() == logm);
  bool prev40 = false, prevc0 = false;
  for (uint32_t i = 0; i < w.rec.size(); ++i) {
    const ExpandLevel& L = w.rec[i];
    const bool last = i + 1 == logm;
    CHECK(L.invalid == kLevelValid);   // the three internal errors of expand_core are unreachable
    CHECK(L.j == i && L.nodes == (B << i));
    CHECK(L.form == form_by_rule(r, B, n, sel, o, i));
    CHECK((L.form == kLevelLastNtt || L.form == kLevelLastCoeff) ? last : true);
    // the 5-byte tree: written only below the transform workgroup's width, only with both switches, only for a reader
    if (L.tout40) {
      CHECK((1u << i) < (r.N >> log_ept(r.logN)));
      CHECK(o.tree40 && o.pack40);
      CHECK(L.form == kLevelFused);
      CHECK(i + 1 < w.rec.size() && w.rec[i + 1].tin40);
    }
    if (w.split && i == w.split) {
      CHECK(L.tin40 == w.handed.cur40 && w.handed.cur40 == prev40);   // across the split: what the TreeState says
      CHECK(L.c0ntt_in == w.handed.c0ntt && w.handed.c0ntt == prevc0);
      CHECK(!L.c0_before);   // never converted in a buffer another stream handed over
    }
    CHECK(L.tin40 == prev40);
    CHECK(L.c0ntt_in == prevc0);
    CHECK(L.tin40 ? (L.form == kLevelFused || L.form == kLevelLastNtt) : true);
    if (r.mode == kNttInt)
      CHECK(L.form == kLevelUnfused && !L.tin40 && !L.tout40 && !L.c0ntt() && !L.c0ntt_out && !L.loop_targets && !L.c0_in_digit &&
            !L.c0_before && !L.c0_after);
    // c0 in NTT form never reaches an unfused (or coefficient-form last) level, and is only produced for a fused one
    CHECK(L.c0ntt() ? (L.form == kLevelFused || L.form == kLevelLastNtt) : true);
    CHECK(L.c0_before ? L.form == kLevelFused : true);
    CHECK(L.c0_after ? (L.form == kLevelUnfused && i + 1 < w.rec.size() && w.rec[i + 1].form == kLevelFused) : true);
    CHECK(L.c0ntt_out == (L.c0ntt() || L.c0_after));
    CHECK((L.c0ntt() || L.c0ntt_out) ? (o.c0_ntt && o.fuse_mac_combine && sel) : true);
    // a 5-byte tree carries no c0 in doubles: the NTT-domain last level needs it from the tree or from the digit kernel
    CHECK((L.form == kLevelLastNtt && L.tin40) ? (L.c0ntt() || L.c0_in_digit) : true);
    CHECK(L.c0_in_digit == (L.form == kLevelLastNtt && !L.c0ntt() && L.nodes >= 256 && L.nodes % 8 == 0));
    CHECK(L.loop_targets == (r.mode != kNttInt && o.loop_transforms && (uint64_t)L.nodes * k >= o.loop_min_sources));
    CHECK(L.hi_limit == ((L.form == kLevelUnfused && last) ? n * B : UINT32_MAX));
    const bool special_only = L.form == kLevelFused || L.form == kLevelLastNtt;
    CHECK(L.mac_base == (special_only ? k : 0) && L.mac_count == (special_only ? 1 : k + 1));
    prev40 = L.tout40;
    prevc0 = L.c0ntt_out;
  }
  const bool fused_last = !w.rec.empty() && (w.rec.back().form == kLevelLastNtt || w.rec.back().form == kLevelLastCoeff);
  CHECK(w.leaves_owed == !fused_last);
}

static bool same_record(const ExpandLevel& a, const ExpandLevel& b) {
  return a.j == b.j && a.nodes == b.nodes && a.form == b.form && a.invalid == b.invalid && a.tin40 == b.tin40 &&
         a.tout40 == b.tout40 && a.c0_in_digit == b.c0_in_digit && a.loop_targets == b.loop_targets &&
         a.c0ntt_in == b.c0ntt_in && a.c0_before == b.c0_before && a.c0_after == b.c0_after && a.c0ntt_out == b.c0ntt_out &&
         a.mac_base == b.mac_base && a.mac_count == b.mac_count && a.hi_limit == b.hi_limit;
}
// ... but for where (and so whether a level reads) c0 in NTT form
static bool same_but_c0(const ExpandLevel& a, const ExpandLevel& b) {
  return a.j == b.j && a.nodes == b.nodes && a.form == b.form && a.invalid == b.invalid && a.loop_targets == b.loop_targets &&
         a.mac_base == b.mac_base && a.mac_count == b.mac_count && a.hi_limit == b.hi_limit;
}

static unsigned long long g_walks = 0;
// one (ring, k, B, n, sel, options) point: the unsplit walk and every split the head rule allows
static void check_point(const Ring& r, uint32_t k, uint32_t B, uint32_t n, bool sel, const ExpandOptions& o, const char* oname) {
  g_at = {nullptr, r.N, k, B, n, 0, r.mode, (int)sel, oname};
  const Walk u = walk(r, k, B, n, sel, o, 0);
  check_walk(r, k, B, n, sel, o, u);
  ++g_walks;
  for (uint32_t h = 1; h <= 8; ++h) {
    const bool allowed = B > 1 && depth_of(n) >= h + 2;   // the head rule, restated (one query ciphertext, head enabled)
    CHECK(expansion_uses_head(1, B, h, true, expansion_depth(n)) == allowed);
    CHECK(!expansion_uses_head(2, B, h, true, expansion_depth(n)) && !expansion_uses_head(1, B, h, false, expansion_depth(n)));
    if (!allowed) continue;
    g_at.split = h;
    const Walk s = walk(r, k, B, n, sel, o, h);
    check_walk(r, k, B, n, sel, o, s);
    ++g_walks;
    CHECK(s.rec.size() == u.rec.size());
    for (uint32_t i = 0; i < s.rec.size() && i < u.rec.size(); ++i)
      CHECK(o.c0_ntt ? same_but_c0(s.rec[i], u.rec[i]) : same_record(s.rec[i], u.rec[i]));
  }
  CHECK(!expansion_uses_head(1, B, 0, true, expansion_depth(n)));
}

static ExpandOptions options(const Ring& r, unsigned bits, unsigned c0, uint32_t fuse_nodes = 128, uint32_t loop_min = 1024) {
  ExpandOptions o;
  o.mode = r.mode;
  o.fuse_last_level = bits & 1;
  o.last_level_ntt = bits & 2;
  o.fuse_mac_combine = bits & 4;
  o.tree40 = bits & 8;
  o.pack40 = bits & 16;
  o.loop_transforms = bits & 32;
  o.c0_ntt = c0 != 0;
  o.c0_ntt_split = c0 >= 2;
  o.fuse_mac_nodes = fuse_nodes;
  o.loop_min_sources = loop_min;
  return o;
}

static void check_groups(const Ring& r, uint32_t n, unsigned bits, unsigned c0, uint32_t fuse_nodes = 128, uint32_t loop_min = 1024,
                         uint32_t only_k = 0) {
  char name[64];
  snprintf(name, sizeof name, "bits%u/c0=%u/fuse%u/loop%u", bits, c0, fuse_nodes, loop_min);
  const ExpandOptions o = options(r, bits, c0, fuse_nodes, loop_min);
  for (uint32_t k = 1; k <= 4; ++k) {
    if (only_k && k != only_k) continue;
    check_point(r, k, 1, n, false, o, name);
    for (uint32_t B = 1; B <= 8; ++B) check_point(r, k, B, n, true, o, name);
  }
}

static void test_domain() {
  struct Star { unsigned bits, c0; };
  std::vector<Star> star = {{63, 0}, {0, 0}, {63, 1}, {63, 2}};
  for (unsigned b = 1; b < 64; b <<= 1) star.push_back({63 & ~b, 0});
  // tier 1: every n, a star of option settings around the defaults
  for (const Ring& r : kRings)
    for (uint32_t n = 1; n <= r.N && r.N <= 4096; ++n)
      for (const Star& s : star) check_groups(r, n, s.bits, s.c0, 128, 1024, s.bits == 63 && s.c0 == 0 ? 0 : 2);
  // tier 2: every combination of the switches at the powers of two; the star at 64 random n
  uint64_t rng = 0x9e3779b97f4a7c15ull;
  for (const Ring& r : kRings) {
    for (uint32_t p = 1; p <= r.N; p <<= 1)
      for (int d = -2; d <= 2; ++d) {
        const int64_t n = (int64_t)p + d;
        if (n < 1 || n > (int64_t)r.N) continue;
        for (unsigned bits = 0; bits < 64; ++bits)
          for (unsigned c0 = 0; c0 < 3; ++c0) check_groups(r, (uint32_t)n, bits, c0);
        for (unsigned bits : {63u, 62u, 61u, 55u})
          for (unsigned c0 = 0; c0 < 3; ++c0) {
            check_groups(r, (uint32_t)n, bits, c0, 16, 1024);
            check_groups(r, (uint32_t)n, bits, c0, 2, 64);
          }
      }
    for (int i = 0; i < 64; ++i) {
      rng = rng * 6364136223846793005ull + 1442695040888963407ull;
      for (const Star& s : star) check_groups(r, 1 + (uint32_t)((rng >> 33) % r.N), s.bits, s.c0);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Walks pinned by hand.  Every row was derived on paper from expand_core as it stood BEFORE the plan existed (the loop
// with its level_fused lambda, out40 expression and loop threshold), never by running plan_expansion: a threshold that
// moves silently fails here by the row's name.  One letter per level: u unfused, F fused, N NTT-domain last level,
// C coefficient-form last level; the flag strings have one character per level, '1' = set.
struct Pinned {
  const char* name;
  Ring r;
  uint32_t k, B, n, split;
  unsigned c0;
  const char *form, *tin40, *tout40, *loop, *c0dig, *c0ntt, *c0after;
};
static const Pinned kPinned[] = {
    // nodes 8 .. 1024; fused from 64 nodes (j = 3); looped from 512 nodes (k = 2); last level 1024 nodes takes c0 in the digit kernel
    {"N4096 k2 B8 n213 defaults", {4096, 12, kNttF64}, 2, 8, 213, 0, 0,
     "uuuFFFFN", "00001111", "00011110", "00000011", "00000001", "00000000", "00000000"},
    // a single query fuses from 128 nodes, but its 128-node level is the last one: no fused level, no 5-byte tree, and
    // 128 nodes are too few for c0 in the digit kernel or (x 2 = 256 sources) the looped transforms
    {"N4096 k2 B1 n200 defaults", {4096, 12, kNttF64}, 2, 1, 200, 0, 0,
     "uuuuuuuN", "00000000", "00000000", "00000000", "00000000", "00000000", "00000000"},
    // nodes 3 * 2^j: fused from j = 5 (96); 5-byte outputs while 2^j < 4096 / 16 = 256, i.e. up to j = 7; looped from 768 (j = 8)
    {"N4096 k2 B3 n1500 defaults (crosses 2^j = N / 16)", {4096, 12, kNttF64}, 2, 3, 1500, 0, 0,
     "uuuuuFFFFFN", "00000011100", "00000111000", "00000000111", "00000000001", "00000000000", "00000000000"},
    // nodes 5 * 2^j: fused from j = 4 (80); head = levels 0 .. 4, hands a 5-byte tree over; last level 640 nodes
    {"N4096 k2 B5 n213 split at 5", {4096, 12, kNttF64}, 2, 5, 213, 5, 0,
     "uuuuFFFN", "00000111", "00001110", "00000001", "00000001", "00000000", "00000000"},
    // C0_NTT = 1: level 2 (the last unfused one) converts its outputs' c0; the last level reads it from the tree
    {"N4096 k2 B8 n213 C0_NTT=1", {4096, 12, kNttF64}, 2, 8, 213, 0, 1,
     "uuuFFFFN", "00001111", "00011110", "00000011", "00000000", "00011111", "00100000"},
    // N = 2048, k = 1: looped from 1024 nodes; 5-byte outputs while 2^j < 128, so level 7 (1024 nodes) writes doubles
    {"N2048 k1 B8 n257 defaults", {2048, 11, kNttF64}, 1, 8, 257, 0, 0,
     "uuuFFFFFN", "000011110", "000111100", "000000011", "000000001", "000000000", "000000000"},
};

static void test_pinned() {
  for (const Pinned& p : kPinned) {
    g_at.row = p.name;
    ExpandOptions o = options(p.r, 63, p.c0);
    const Walk w = walk(p.r, p.k, p.B, p.n, true, o, p.split);
    const size_t len = strlen(p.form);
    CHECK(w.rec.size() == len);
    if (w.rec.size() != len) continue;
    CHECK(p.split ? w.split == p.split : w.split == 0);
    for (size_t i = 0; i < len; ++i) {
      const ExpandLevel& L = w.rec[i];
      CHECK("uFNC"[L.form] == p.form[i]);
      CHECK(L.tin40 == (p.tin40[i] == '1'));
      CHECK(L.tout40 == (p.tout40[i] == '1'));
      CHECK(L.loop_targets == (p.loop[i] == '1'));
      CHECK(L.c0_in_digit == (p.c0dig[i] == '1'));
      CHECK(L.c0ntt() == (p.c0ntt[i] == '1'));
      CHECK(L.c0_after == (p.c0after[i] == '1'));
      CHECK(!L.c0_before && L.invalid == kLevelValid && L.hi_limit == UINT32_MAX);
    }
    CHECK(!w.leaves_owed);
  }
  // pirgpu_expand's walk (no selectors): the last level is an ordinary one, cut at n * B outputs
  g_at.row = "N4096 k2 B1 n300 without selectors";
  const Ring r{4096, 12, kNttF64};
  const Walk w = walk(r, 2, 1, 300, false, options(r, 63, 0), 0);
  CHECK(w.rec.size() == 9 && w.leaves_owed);
  for (size_t i = 0; i < w.rec.size(); ++i) {
    CHECK(w.rec[i].form == (i >= 7 ? kLevelFused : kLevelUnfused));   // 128 and 256 nodes
    CHECK(!w.rec[i].tout40);                                           // (only into a last level that is the NTT-domain one)
    CHECK(w.rec[i].hi_limit == UINT32_MAX);                            // (the fused kernel writes every output)
  }
  // the packed word of pirgpu_expansion_forms (include/pirgpu.h)
  ExpandLevel L;
  L.j = 7;
  L.form = kLevelLastNtt;
  L.tin40 = L.c0_in_digit = L.loop_targets = true;
  L.mac_base = 2;
  L.mac_count = 1;
  CHECK(pack_expand_level(L, false, true) == (2u | 1u << 2 | 1u << 4 | 1u << 5 | 1u << 11 | 1u << 15 | 7u << 16));
  L = ExpandLevel();
  L.j = 2;
  L.c0_after = L.c0ntt_out = true;
  L.mac_count = 3;
  CHECK(pack_expand_level(L, true, false) == (1u << 7 | 1u << 9 | 1u << 12 | 2u << 16));
}

// --reachable N k n...: see the head of the file
static int reachable(int argc, char** argv) {
  if (argc < 5) return 2;
  const uint32_t N = (uint32_t)atoi(argv[2]), k = (uint32_t)atoi(argv[3]);
  uint32_t logN = 0;
  while ((1u << logN) < N) ++logN;
  struct Setting { const char* name; unsigned bits, c0; int mode; };
  const Setting settings[] = {{"default", 63, 0, kNttF64},       {"TREE40=0", 63 & ~8u, 0, kNttF64},
                              {"PACK40=0", 63 & ~16u, 0, kNttF64}, {"FUSE_MAC_COMBINE=0", 63 & ~4u, 0, kNttF64},
                              {"LAST_NTT=0", 63 & ~2u, 0, kNttF64}, {"FUSE_LAST=0", 63 & ~1u, 0, kNttF64},
                              {"LOOP_TRANSFORMS=0", 63 & ~32u, 0, kNttF64}, {"C0_NTT=1", 63, 1, kNttF64},
                              {"C0_NTT=2", 63, 2, kNttF64},       {"PIRGPU_NTT_MODE=0", 63, 0, kNttInt}};
  for (const Setting& s : settings) {
    const Ring r{N, logN, s.mode};
    const ExpandOptions o = options(r, s.bits, s.c0);
    for (uint32_t h = 0; h <= 8; ++h) {
      if (h && strcmp(s.name, "default") != 0) continue;   // the head split is run with the defaults only
      std::set<std::string> seen;
      for (int a = 4; a < argc; ++a) {
        const uint32_t n = (uint32_t)atoi(argv[a]);
        if (n < 1 || n > N) continue;
        for (uint32_t B = 1; B <= 8; ++B) {
          if (h && !expansion_uses_head(1, B, h, true, expansion_depth(n))) continue;
          for (const ExpandLevel& L : walk(r, k, B, n, true, o, h).rec) {
            char t[64];
            snprintf(t, sizeof t, "%c %d %d %d %d %d", "uFNC"[L.form], (int)L.tin40, (int)L.tout40, (int)L.c0_in_digit,
                     (int)L.loop_targets, (int)L.c0ntt());
            seen.insert(t);
          }
        }
      }
      for (const std::string& t : seen) printf("%s split=%u : %s\n", s.name, h, t.c_str());
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "--reachable") == 0) return reachable(argc, argv);
  test_pinned();
  test_domain();
  if (g_failed) {
    fprintf(stderr, "expansion_plan_test: %d checks FAILED\n", g_failed);
    return 1;
  }
  printf("expansion_plan_test OK (%llu walks)\n", g_walks);
  return 0;
}
