// Host pack / unpack of packed replies (pir_amd/csrc/reply_pack.h) and their wire form (wire_codec.cpp) without a GPU,
// against vectors the Python model wrote (tests/reply_pack_model.py via tests/test_reply_pack_host.py).  Stand-alone:
//   g++ -std=c++17 -fsanitize=address,undefined tests/cpp/reply_pack_test.cpp pir_amd/csrc/wire_codec.cpp -o t && ./t vectors.bin
// Vector file, little-endian: u64 n_cases, then per case u64 w, N, q, n_words, x[N], packed[n_words].
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

static std::vector<uint64_t> read_words(FILE* f, size_t n) {
  std::vector<uint64_t> v(n);
  if (n && fread(v.data(), 8, n, f) != n) {
    printf("vector file truncated\n");
    exit(2);
  }
  return v;
}

// Exactly-sized heap copies: a read or write one word past the end is an AddressSanitizer report.
static std::unique_ptr<uint64_t[]> exact(const std::vector<uint64_t>& v) {
  std::unique_ptr<uint64_t[]> p(new uint64_t[v.size() ? v.size() : 1]);
  if (!v.empty()) memcpy(p.get(), v.data(), v.size() * 8);
  return p;
}

static void test_vectors(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    printf("cannot open %s\n", path);
    exit(2);
  }
  const uint64_t n_cases = read_words(f, 1)[0];
  bool seen[65] = {};
  for (uint64_t c = 0; c < n_cases; ++c) {
    const std::vector<uint64_t> head = read_words(f, 4);
    const uint32_t w = (uint32_t)head[0], N = (uint32_t)head[1];
    const uint64_t q = head[2], n_words = head[3];
    const std::vector<uint64_t> x = read_words(f, N), want = read_words(f, n_words);
    seen[w] = true;
    CHECK(rpk::width(q) == w);
    CHECK(rpk::poly_words(N, w) == n_words);
    auto xin = exact(x);
    std::unique_ptr<uint64_t[]> got(new uint64_t[n_words]);
    rpk::pack_poly(xin.get(), N, w, got.get());
    CHECK(memcmp(got.get(), want.data(), n_words * 8) == 0);
    std::unique_ptr<uint64_t[]> back(new uint64_t[N]);
    auto pin = exact(want);
    CHECK(rpk::unpack_poly(pin.get(), N, w, q, back.get()));
    CHECK(memcmp(back.get(), x.data(), (size_t)N * 8) == 0);
    // the same through bytes at an odd address (the wire hands the words over unaligned)
    std::unique_ptr<uint8_t[]> odd(new uint8_t[n_words * 8 + 1]);
    memcpy(odd.get() + 1, want.data(), n_words * 8);
    CHECK(rpk::unpack_poly(odd.get() + 1, N, w, q, back.get()));
    CHECK(memcmp(back.get(), x.data(), (size_t)N * 8) == 0);
    rpk::pack_poly(xin.get(), N, w, odd.get() + 1);
    CHECK(memcmp(odd.get() + 1, want.data(), n_words * 8) == 0);
  }
  fclose(f);
  for (uint32_t w : {2u, 30u, 36u, 37u, 43u, 49u, 60u, 61u}) CHECK(seen[w]);
}

static void test_out_of_range_coefficient() {
  // q = 5 (width 3): the values 5, 6, 7 fit the width and are not residues
  const uint32_t N = 64, w = 3;
  std::vector<uint64_t> x(N, 4), p(rpk::poly_words(N, w)), back(N);
  rpk::pack_poly(x.data(), N, w, p.data());
  CHECK(rpk::unpack_poly(p.data(), N, w, 5, back.data()));
  for (uint64_t bad : {5ull, 6ull, 7ull})
    for (uint32_t at : {0u, 21u, 63u}) {   // coefficient 21 straddles the first word boundary
      std::vector<uint64_t> y = x;
      y[at] = bad;
      rpk::pack_poly(y.data(), N, w, p.data());
      CHECK(!rpk::unpack_poly(p.data(), N, w, 5, back.data()));
      CHECK(back == y);   // every coefficient is still decoded
    }
}

static wire::Shape small_shape() {
  pirgpu_params prm{};
  prm.poly_modulus_degree = 64;
  prm.num_data_primes = 2;
  prm.coeff_modulus[0] = 1153;            // 11 bits, == 1 mod 128 (the codec checks ranges only, not primality)
  prm.coeff_modulus[1] = 68719403009ull;  // 36 bits
  prm.special_prime = 68719230977ull;
  prm.plain_modulus = 257;
  return wire::make_shape(prm);
}

static std::string ciphertexts_message(const std::string& object) {
  std::string msg;
  wire::put_bytes_field(msg, 1, object);
  return msg;
}

static void test_wire_form() {
  const wire::Shape sh = small_shape();
  const uint32_t N = sh.N, k = sh.k;
  std::vector<uint64_t> ct((size_t)2 * k * N);
  for (size_t i = 0; i < ct.size(); ++i) {
    const uint64_t q = sh.q[(i / N) % k];
    ct[i] = (i % 3 == 0) ? q - 1 : (0x9E3779B97F4A7C15ull * (i + 1)) % q;
  }
  const size_t pw = rpk::ct_words(N, sh.q, k);
  CHECK(pw == 2 * (size_t)(11 + 36));
  std::vector<uint64_t> packed(pw);
  rpk::pack_ct(ct.data(), N, sh.q, k, k, packed.data());
  std::vector<uint64_t> back(ct.size());
  CHECK(rpk::unpack_ct(packed.data(), N, sh.q, k, back.data()) && back == ct);

  std::string obj;
  wire::append_ciphertext_prefix_packed(obj, sh);
  const size_t prefix = obj.size();
  obj.append(reinterpret_cast<const char*>(packed.data()), pw * 8);
  CHECK(obj.size() == wire::saved_ciphertext_size_packed(sh));
  CHECK(wire::saved_ciphertext_size(sh) - obj.size() == ((size_t)2 * k * N - pw) * 8);
  // outer header as SEAL writes it, inner header with compression byte 0x80 and the count still 2 k N
  std::string plain;
  wire::append_ciphertext_prefix(plain, sh);
  CHECK(plain.size() == prefix);
  const size_t inner = prefix - 8 - wire::kHeader;
  CHECK((uint8_t)obj[5] == 0 && (uint8_t)obj[inner + 5] == 0x80 && (uint8_t)plain[inner + 5] == 0);
  CHECK(memcmp(obj.data() + wire::kHeader, plain.data() + wire::kHeader, inner - wire::kHeader) == 0);   // parms_id, shape
  uint64_t count;
  memcpy(&count, obj.data() + prefix - 8, 8);
  CHECK(count == (uint64_t)2 * k * N);

  // the reply loader takes either form; the request loader refuses the packed one
  std::vector<uint64_t> out;
  {
    const std::string msg = ciphertexts_message(obj);
    std::unique_ptr<uint8_t[]> heap(new uint8_t[msg.size()]);
    memcpy(heap.get(), msg.data(), msg.size());
    CHECK(wire::load_reply(sh, heap.get(), msg.size(), out) == 1 && out == ct);
    bool refused = false;
    try {
      wire::load_query(sh, heap.get(), msg.size(), out);
    } catch (const wire::Err& e) {
      refused = e.code == PIRGPU_UNIMPLEMENTED;
    }
    CHECK(refused);
  }
  {
    const std::string msg = ciphertexts_message(wire::save_ciphertext(sh, ct.data()));
    CHECK(wire::load_reply(sh, reinterpret_cast<const uint8_t*>(msg.data()), msg.size(), out) == 1 && out == ct);
  }
  // truncated: every cut of the object, each in an exactly-sized heap buffer
  for (size_t cut : {(size_t)0, (size_t)8, wire::kHeader, prefix - 8, prefix, prefix + 8, obj.size() - 8, obj.size() - 1}) {
    const std::string msg = ciphertexts_message(obj.substr(0, cut));
    std::unique_ptr<uint8_t[]> heap(new uint8_t[msg.size()]);
    memcpy(heap.get(), msg.data(), msg.size());
    bool threw = false;
    try {
      wire::load_reply(sh, heap.get(), msg.size(), out);
    } catch (const wire::Err& e) {
      threw = e.code == PIRGPU_INVALID_ARGUMENT;
    }
    CHECK(threw);
  }
  // an object whose headers promise the full size over too few words
  {
    std::string lying = obj.substr(0, obj.size() - 8);
    const std::string msg = ciphertexts_message(lying);
    bool threw = false;
    try {
      wire::load_reply(sh, reinterpret_cast<const uint8_t*>(msg.data()), msg.size(), out);
    } catch (const wire::Err&) {
      threw = true;
    }
    CHECK(threw);
  }
  // a coefficient at its modulus: q_0 = 1153 fits 11 bits
  {
    std::vector<uint64_t> bad_ct = ct;
    bad_ct[5] = sh.q[0];
    std::vector<uint64_t> bad(pw);
    rpk::pack_ct(bad_ct.data(), N, sh.q, k, k, bad.data());
    std::string o2 = obj.substr(0, prefix);
    o2.append(reinterpret_cast<const char*>(bad.data()), pw * 8);
    const std::string msg = ciphertexts_message(o2);
    bool threw = false;
    try {
      wire::load_reply(sh, reinterpret_cast<const uint8_t*>(msg.data()), msg.size(), out);
    } catch (const wire::Err& e) {
      threw = e.code == PIRGPU_INVALID_ARGUMENT && e.msg.find("out of range") != std::string::npos;
    }
    CHECK(threw);
  }
  // pack_ct reads the first r residues of ciphertexts that keep k (the switched-in-place level 0 of a packed context)
  {
    std::vector<uint64_t> one(rpk::ct_words(N, sh.q, 1)), first((size_t)2 * N), b1((size_t)2 * N);
    rpk::pack_ct(ct.data(), N, sh.q, 1, k, one.data());
    for (uint32_t c = 0; c < 2; ++c) memcpy(first.data() + (size_t)c * N, ct.data() + (size_t)c * k * N, (size_t)N * 8);
    CHECK(rpk::unpack_ct(one.data(), N, sh.q, 1, b1.data()) && b1 == first);
  }
}

int main(int argc, char** argv) {
  if (argc != 2) {
    printf("usage: %s vectors.bin\n", argv[0]);
    return 2;
  }
  test_vectors(argv[1]);
  test_out_of_range_coefficient();
  test_wire_form();
  if (g_failed) {
    printf("%d checks failed\n", g_failed);
    return 1;
  }
  printf("reply_pack_test OK\n");
  return 0;
}
