// The host side of compact queries without a GPU: rpk::check_poly (pir_amd/csrc/reply_pack.h) and
// the query codec -- query_compact_form, the splitting loader load_query_compact_into, the host expansion of the packed
// form in load_query_into -- of pir_amd/csrc/wire_codec.cpp.  Stand-alone:
//   g++ -std=c++17 -fsanitize=address,undefined tests/cpp/query_compact_test.cpp pir_amd/csrc/wire_codec.cpp -o t && ./t
// Every input lives in an exactly-sized heap block: a read past its end is an AddressSanitizer report.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "../../pir_amd/csrc/reply_pack.h"
#include "../../pir_amd/csrc/wire_codec.h"

using namespace pirgpu;

static int g_failed = 0;
#define CHECK(cond)                                             \
  do {                                                          \
    if (!(cond)) {                                              \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      ++g_failed;                                               \
    }                                                           \
  } while (0)

static wire::Shape small_shape() {
  pirgpu_params prm{};
  prm.poly_modulus_degree = 64;
  prm.num_data_primes = 2;
  prm.coeff_modulus[0] = 1153;            // 11 bits (the codec checks ranges only, not primality)
  prm.coeff_modulus[1] = 68719403009ull;  // 36 bits
  prm.special_prime = 68719230977ull;
  prm.plain_modulus = 257;
  return wire::make_shape(prm);
}

// `bytes` at offset `odd` of an exactly-sized block
struct Block {
  std::unique_ptr<uint8_t[]> mem;
  const uint8_t* p;
  size_t n;
  Block(const std::string& bytes, size_t odd) : mem(new uint8_t[bytes.size() + odd]), p(mem.get() + odd), n(bytes.size()) {
    memcpy(mem.get() + odd, bytes.data(), bytes.size());
  }
};

static std::string message(const std::vector<std::string>& objects) {
  std::string msg;
  for (const std::string& o : objects) wire::put_bytes_field(msg, 1, o);
  return msg;
}

// status of the splitting loader on a message (0 = loaded), the count through *n
static int split_status(const wire::Shape& sh, const std::string& msg, bool packed, size_t odd, std::vector<uint64_t>* out,
                        uint32_t* n, std::string* why = nullptr) {
  Block b(msg, odd);
  std::unique_ptr<uint64_t[]> dst(new uint64_t[4 * wire::query_compact_words(sh, packed)]);
  try {
    *n = wire::load_query_compact_into(sh, b.p, b.n, packed, dst.get(), 4);
    if (out) out->assign(dst.get(), dst.get() + (size_t)(*n < 4 ? *n : 4) * wire::query_compact_words(sh, packed));
    return 0;
  } catch (const wire::Err& e) {
    if (why) *why = e.msg;
    return e.code;
  }
}

static int host_status(const wire::Shape& sh, const std::string& msg, size_t odd, std::vector<uint64_t>* out, uint32_t* n) {
  Block b(msg, odd);
  std::unique_ptr<uint64_t[]> dst(new uint64_t[4 * 2 * (size_t)sh.k * sh.N]);
  try {
    *n = wire::load_query_into(sh, b.p, b.n, dst.get(), 4);
    if (out) out->assign(dst.get(), dst.get() + (size_t)(*n < 4 ? *n : 4) * 2 * sh.k * sh.N);
    return 0;
  } catch (const wire::Err& e) {
    return e.code;
  }
}

static void test_check_poly() {
  // widths 11, 36, 37, 49, 60 and 64 (the plain form); q - 1 passes, q and 2^w - 1 fail, at the first, the last and a
  // word-straddling coefficient; at an even and at an odd address
  const uint32_t N = 128;
  for (uint64_t q : {1153ull, 68719403009ull, 137438822401ull, 562949953216513ull, 1152921504606830593ull, ~0ull}) {
    const uint32_t w = rpk::width(q);
    uint32_t straddle = 1;
    while ((straddle * w) % 64 + w <= 64 && straddle < N - 1) ++straddle;
    std::vector<uint64_t> x(N);
    for (uint32_t i = 0; i < N; ++i) x[i] = (0x9E3779B97F4A7C15ull * (i + 1)) % q;
    const size_t pw = rpk::poly_words(N, w);
    for (uint32_t at : {0u, N - 1, straddle})
      for (int kind = 0; kind < 3; ++kind) {
        std::vector<uint64_t> y = x;
        const uint64_t top = w >= 64 ? ~0ull : (1ull << w) - 1;
        y[at] = kind == 0 ? q - 1 : kind == 1 ? q : top;
        const bool want = y[at] < q;
        for (size_t odd : {0u, 1u, 3u}) {
          std::unique_ptr<uint8_t[]> mem(new uint8_t[pw * 8 + odd]);
          rpk::pack_poly(y.data(), N, w, mem.get() + odd);
          CHECK(rpk::check_poly(mem.get() + odd, N, w, q) == want);
          std::vector<uint64_t> back(N);
          CHECK(rpk::unpack_poly(mem.get() + odd, N, w, q, back.data()) == want && back == y);
        }
      }
  }
}

static void test_loader() {
  const wire::Shape sh = small_shape();
  const uint32_t N = sh.N, k = sh.k;
  uint8_t seed[wire::kSeedBytes];
  for (size_t i = 0; i < sizeof(seed); ++i) seed[i] = (uint8_t)(7 * i + 1);
  std::vector<uint64_t> c0((size_t)k * N);
  for (size_t i = 0; i < c0.size(); ++i) {
    const uint64_t q = sh.q[i / N];
    c0[i] = i % 5 == 0 ? q - 1 : (0x9E3779B97F4A7C15ull * (i + 1)) % q;
  }
  // what the host expansion must give: c0, then sample_poly_uniform over the data moduli
  std::vector<uint64_t> full((size_t)2 * k * N);
  memcpy(full.data(), c0.data(), c0.size() * 8);
  {
    wire::SealPrng rng(seed);
    wire::sample_poly_uniform(rng, sh.q, k, N, full.data() + c0.size());
  }
  for (int packed = 0; packed < 2; ++packed) {
    const size_t cw = wire::query_compact_words(sh, packed != 0);
    CHECK(cw == (packed ? (size_t)(11 + 36) : (size_t)k * N) + 8);
    auto compact_of = [&](const std::vector<uint64_t>& c) {
      std::vector<uint64_t> obj(cw);
      uint8_t* o = reinterpret_cast<uint8_t*>(obj.data());
      for (uint32_t j = 0; j < k; ++j) {
        const uint32_t w = packed ? rpk::width(sh.q[j]) : 64;
        rpk::pack_poly(c.data() + (size_t)j * N, N, w, o);
        o += rpk::poly_words(N, w) * 8;
      }
      memcpy(o, seed, sizeof(seed));
      return obj;
    };
    const std::vector<uint64_t> obj = compact_of(c0);
    const std::string ct = wire::save_query_compact(sh, obj.data(), packed != 0);
    const std::string msg = message({ct, ct});
    // compact objects at odd alignments: the form, the split (bytes as they lie) and the host expansion
    for (size_t odd : {0u, 1u, 3u, 5u}) {
      Block b(msg, odd);
      uint32_t n = 0;
      CHECK(wire::query_compact_form(sh, b.p, b.n, &n) == (packed ? 2 : 1) && n == 2);
      std::vector<uint64_t> got;
      CHECK(split_status(sh, msg, packed != 0, odd, &got, &n) == 0 && n == 2);
      CHECK(got.size() == 2 * cw && memcmp(got.data(), obj.data(), cw * 8) == 0 &&
            memcmp(got.data() + cw, obj.data(), cw * 8) == 0);
      CHECK(host_status(sh, msg, odd, &got, &n) == 0 && n == 2);
      CHECK(got.size() == 2 * full.size() && memcmp(got.data(), full.data(), full.size() * 8) == 0 &&
            memcmp(got.data() + full.size(), full.data(), full.size() * 8) == 0);
    }
    // the other form's loader refuses it
    uint32_t n = 0;
    CHECK(split_status(sh, msg, packed == 0, 1, nullptr, &n) == PIRGPU_INVALID_ARGUMENT);
    // truncated inside the seed, inside the array and inside the header: InvalidArgument, form 0
    const size_t prefix = 16 + 32 + 33;
    for (size_t keep : {ct.size() - 1, ct.size() - 33, ct.size() - 64 - 9, prefix + 16 + 8 + 3, prefix + 7, (size_t)20, (size_t)9}) {
      std::string cut = ct.substr(0, keep);
      const std::string m = message({cut});
      for (size_t odd : {0u, 1u}) {
        Block b(m, odd);
        CHECK(wire::query_compact_form(sh, b.p, b.n, &n) == 0);
        CHECK(split_status(sh, m, packed != 0, odd, nullptr, &n) == PIRGPU_INVALID_ARGUMENT);
        CHECK(host_status(sh, m, odd, nullptr, &n) == PIRGPU_INVALID_ARGUMENT);
      }
      // ... and with the outer size field adjusted to the shorter object
      const uint64_t total = keep;
      if (keep >= 16) {
        memcpy(&cut[8], &total, 8);
        const std::string m2 = message({cut});
        CHECK(split_status(sh, m2, packed != 0, 1, nullptr, &n) == PIRGPU_INVALID_ARGUMENT);
        CHECK(host_status(sh, m2, 1, nullptr, &n) == PIRGPU_INVALID_ARGUMENT);
      }
    }
    // the packed array is exact: 8 bytes of padding between the stream and the seed (both size fields adjusted) are refused
    if (packed) {
      std::string pad = ct;
      pad.insert(pad.size() - wire::kSeedBytes, 8, '\0');
      uint64_t inner, outer = pad.size();
      memcpy(&inner, &pad[prefix + 8], 8);
      inner += 8;
      memcpy(&pad[prefix + 8], &inner, 8);
      memcpy(&pad[8], &outer, 8);
      const std::string m = message({pad});
      Block b(m, 1);
      CHECK(wire::query_compact_form(sh, b.p, b.n, &n) == 0);
      CHECK(split_status(sh, m, true, 1, nullptr, &n) == PIRGPU_INVALID_ARGUMENT);
      CHECK(host_status(sh, m, 1, nullptr, &n) == PIRGPU_INVALID_ARGUMENT);
    }
    // a c0 coefficient equal to q in the first and in the last position
    for (size_t at : {(size_t)0, c0.size() - 1}) {
      std::vector<uint64_t> bad = c0;
      bad[at] = sh.q[at / N];
      const std::vector<uint64_t> bobj = compact_of(bad);
      const std::string m = message({ct, wire::save_query_compact(sh, bobj.data(), packed != 0)});
      std::string why;
      CHECK(split_status(sh, m, packed != 0, 3, nullptr, &n, &why) == PIRGPU_INVALID_ARGUMENT);
      CHECK(why == "ciphertext data is invalid (coefficient out of range)");
      CHECK(host_status(sh, m, 3, nullptr, &n) == PIRGPU_INVALID_ARGUMENT);
      Block b(m, 0);
      CHECK(wire::query_compact_form(sh, b.p, b.n, &n) == (packed ? 2 : 1));   // the headers alone are sound
    }
  }
  // the packed byte on a full-size array stays what it was for a request (Unimplemented, like any compression byte:
  // tests/cpp/reply_pack_test.cpp pins it); form 0
  {
    std::string ct = wire::save_ciphertext(sh, full.data());
    CHECK((uint8_t)ct[16 + 32 + 33 + 5] == 0);
    uint32_t n = 0;
    CHECK(host_status(sh, message({ct}), 1, nullptr, &n) == 0 && n == 1);
    Block plain(message({ct}), 1);
    CHECK(wire::query_compact_form(sh, plain.p, plain.n, &n) == 0 && n == 1);   // fully expanded: the host's
    ct[16 + 32 + 33 + 5] = (char)rpk::kPackedComprByte;
    const std::string m = message({ct});
    Block b(m, 1);
    CHECK(wire::query_compact_form(sh, b.p, b.n, &n) == 0);
    CHECK(host_status(sh, m, 1, nullptr, &n) == PIRGPU_UNIMPLEMENTED);
    CHECK(split_status(sh, m, true, 1, nullptr, &n) == PIRGPU_UNIMPLEMENTED);
  }
  // a mixed message (one compact, one expanded) has no form; the host loads it
  {
    std::vector<uint64_t> obj((size_t)k * N + 8);
    memcpy(obj.data(), c0.data(), c0.size() * 8);
    memcpy(obj.data() + c0.size(), seed, sizeof(seed));
    const std::string m = message({wire::save_query_compact(sh, obj.data(), false), wire::save_ciphertext(sh, full.data())});
    Block b(m, 1);
    uint32_t n = 0;
    CHECK(wire::query_compact_form(sh, b.p, b.n, &n) == 0 && n == 2);
    std::vector<uint64_t> got;
    CHECK(host_status(sh, m, 1, &got, &n) == 0 && n == 2);
    CHECK(memcmp(got.data(), full.data(), full.size() * 8) == 0 && memcmp(got.data() + full.size(), full.data(), full.size() * 8) == 0);
  }
}

int main() {
  test_check_poly();
  test_loader();
  if (g_failed) {
    printf("%d checks failed\n", g_failed);
    return 1;
  }
  printf("query_compact_test OK\n");
  return 0;
}
