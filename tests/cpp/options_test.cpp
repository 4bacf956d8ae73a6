// options_test.cpp -- the option registry (pir_amd/csrc/options.h) on the host: the list, name lookup, the environment
// gate, precedence, raw values, kinds and counters.  Stand-alone, single-threaded; sets and unsets environment
// variables itself.  Built and run under AddressSanitizer + UBSan by tests/test_options_registry.py.
#include <ctype.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>

#include "../../pir_amd/csrc/options.h"

using namespace pirgpu;

static int g_failed = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                                        \
    }                                                                    \
  } while (0)

// The ABI surface, stated a second time: a row cannot vanish from options.h, or change its kind, unnoticed.
static const char* const kEarly[] = {
    "UPPER_BLOCKS", "UPPER_BLOCKS_BATCH", "SCAN_LIMB", "SCAN_MQ_SINGLE", "SCAN_ROWS", "SCAN_BLOCK", "SCAN_NSPLIT",
    "FUSE_LAST", "FUSE_MAC_COMBINE", "LAST_NTT", "C0_NTT", "SEL_F64", "TREE40", "SPLIT_UPPER", "SPLIT_UPPER_MB", "PACK40",
    "PACK_BYTES", "TREE40_WIDE", "SCAN_MFMA", "SCAN_MFMA_WIDE", "SCAN_MFMA_TOP4", "SCAN_MFMA_NQ", "SCAN_MFMA_SINGLE",
    "HEAD_LEVELS", "HEAD_MODE", "SCAN_F64_FOLD", "SCAN_F64_FOLD_BATCH", "LOOP_TRANSFORMS", "DB_STREAM_MB", "CT_SCRATCH_MB",
    "CT_SHARED_SEL"};
static const char* const kLive[] = {"SCAN_MFMA_WGS_BATCH", "SLOTS_SCAN_WGS", "SLOTS_GATHER_NTT", "SLOTS_SCAN_BLK_MAJOR",
                                    "TABLES_ONE_LAUNCH", "CT_ROWSUM_SPLITS"};
static const char* const kCounter[] = {"SCAN_LAUNCHES", "CT_BLOCKS", "UPPER_PARTS", "CT_RELINS", "CT_LIFTS"};

template <size_t n>
static void check_kind(const char* const (&names)[n], OptKind kind, size_t expect) {
  CHECK(n == expect);
  for (const char* name : names) {
    const OptId id = find_option(name);
    CHECK(id != OPT_COUNT);
    if (id != OPT_COUNT) {
      CHECK(kOptRows[id].kind == kind);
      CHECK(strcmp(kOptRows[id].name, name) == 0);
    }
  }
}

static void test_list() {
  CHECK(OPT_COUNT == 42);
  std::set<std::string> seen;
  for (int id = 0; id < OPT_COUNT; ++id) {
    const OptRow& row = kOptRows[id];
    CHECK(row.name && row.name[0]);
    CHECK(seen.insert(row.name).second);   // distinct
    for (const char* p = row.name; *p; ++p) CHECK(isupper((unsigned char)*p) || isdigit((unsigned char)*p) || *p == '_');
    CHECK(std::string(row.env) == std::string("PIRGPU_") + row.name);
    CHECK(row.doc && row.doc[0]);
    CHECK(find_option(row.name) == id);
  }
  CHECK(seen.size() == 42);
  check_kind(kEarly, OptKind::Early, 31);
  check_kind(kLive, OptKind::Live, 6);
  check_kind(kCounter, OptKind::Counter, 5);
}

static void test_lookup() {
  CHECK(find_option("Head_Levels") == OPT_HEAD_LEVELS);
  CHECK(find_option("head_levels") == OPT_HEAD_LEVELS);
  CHECK(find_option("HEAD_LEVELS") == OPT_HEAD_LEVELS);
  CHECK(find_option("LANES") == OPT_COUNT);              // settled sweeps that used to be options
  CHECK(find_option("LOOP_MIN_SOURCES") == OPT_COUNT);
  CHECK(find_option("") == OPT_COUNT);
  CHECK(find_option("HEAD_LEVEL") == OPT_COUNT);         // a prefix of a name ...
  CHECK(find_option("HEAD_LEVELS_") == OPT_COUNT);       // ... and a name with a tail
  CHECK(find_option("PIRGPU_HEAD_LEVELS") == OPT_COUNT);
}

static void test_environment_gate() {
  OptionStore st;
  bool present = true;
  setenv("PIRGPU_SCAN_MFMA", "0", 1);
  unsetenv("PIRGPU_ALLOW_ENV");
  CHECK(st.value(OPT_SCAN_MFMA, 1, &present) == 1 && !present);
  CHECK(st.get(OPT_SCAN_MFMA) == -1);
  setenv("PIRGPU_ALLOW_ENV", "0", 1);
  CHECK(st.value(OPT_SCAN_MFMA, 1, &present) == 1 && !present);
  setenv("PIRGPU_ALLOW_ENV", "1", 1);
  CHECK(st.value(OPT_SCAN_MFMA, 1, &present) == 0 && present);
  CHECK(st.get(OPT_SCAN_MFMA) == 0);
  setenv("PIRGPU_SCAN_MFMA", "", 1);                     // empty: unset
  CHECK(st.value(OPT_SCAN_MFMA, 1, &present) == 1 && !present);
  CHECK(st.get(OPT_SCAN_MFMA) == -1);
  unsetenv("PIRGPU_SCAN_MFMA");
  CHECK(st.value(OPT_SCAN_MFMA, 7, &present) == 7 && !present);
  CHECK(st.value(OPT_SCAN_MFMA, 7) == 7);                // `present` is optional
}

static void test_precedence_and_raw_values() {
  OptionStore st;
  bool present = false;
  setenv("PIRGPU_ALLOW_ENV", "1", 1);
  setenv("PIRGPU_HEAD_LEVELS", "3", 1);
  CHECK(st.value(OPT_HEAD_LEVELS, 5, &present) == 3 && present);       // environment over default
  st.set(OPT_HEAD_LEVELS, 2);
  CHECK(st.value(OPT_HEAD_LEVELS, 5, &present) == 2 && present);       // by name over environment
  CHECK(st.get(OPT_HEAD_LEVELS) == 2);
  unsetenv("PIRGPU_HEAD_LEVELS");
  CHECK(st.value(OPT_HEAD_LEVELS, 5, &present) == 2 && present);
  CHECK(st.value(OPT_HEAD_MODE, 1, &present) == 1 && !present);        // the default, and only for the option set
  st.set(OPT_HEAD_LEVELS, -5);                                          // raw: clamping is the reader's business
  CHECK(st.value(OPT_HEAD_LEVELS, 5, &present) == -5 && present);
  CHECK(st.get(OPT_HEAD_LEVELS) == -5);
  st.set(OPT_SLOTS_SCAN_WGS, 0);                                        // 0 is a value, not "unset"
  CHECK(st.value(OPT_SLOTS_SCAN_WGS, 128, &present) == 0 && present);
  CHECK(st.get(OPT_CT_SHARED_SEL, 1) == 1 && st.get(OPT_CT_SHARED_SEL, 0) == 0);   // the caller's report for "unset"
  OptionStore other;                                                    // stores are independent
  CHECK(other.get(OPT_HEAD_LEVELS) == -1);
}

static void test_counters() {
  OptionStore st;
  setenv("PIRGPU_ALLOW_ENV", "1", 1);
  setenv("PIRGPU_CT_BLOCKS", "99", 1);                   // a counter ignores the environment
  CHECK(st.get(OPT_CT_BLOCKS) == 0);
  st.counter(OPT_CT_BLOCKS) += 4;
  ++st.counter(OPT_CT_BLOCKS);
  CHECK(st.get(OPT_CT_BLOCKS) == 5);
  st.set(OPT_CT_BLOCKS, 7);
  CHECK(st.get(OPT_CT_BLOCKS) == 7 && st.counter(OPT_CT_BLOCKS) == 7);
  st.set(OPT_CT_BLOCKS, -3);
  CHECK(st.get(OPT_CT_BLOCKS) == 0);
  CHECK(st.get(OPT_CT_LIFTS) == 0 && st.get(OPT_SCAN_LAUNCHES, 5) == 0);   // never "unset"
  unsetenv("PIRGPU_CT_BLOCKS");
}

int main() {
  test_list();
  test_lookup();
  test_environment_gate();
  test_precedence_and_raw_values();
  test_counters();
  unsetenv("PIRGPU_ALLOW_ENV");
  if (g_failed) {
    fprintf(stderr, "options_test: %d checks failed\n", g_failed);
    return 1;
  }
  printf("options_test OK\n");
  return 0;
}
