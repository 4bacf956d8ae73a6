// reply_pack.h -- packed replies on the host: host-only, shared by the wire codec, the client and
// the context's test hooks.  The device twin is reply_pack.hip.
//
// A reply ciphertext is [2][r][N] canonical residues.  For modulus q_j the width is w_j = bit length of q_j - 1.
// Polynomial (c, j) becomes a little-endian bit stream of N w_j bits -- bit b of coefficient i is stream bit i w_j + b --
// stored as N w_j / 64 little-endian u64 words (whole words: N is a multiple of 64).  A packed ciphertext is its 2 r
// polynomials in the order (c, j).  Words are read and written through memcpy: the wire hands them over at any alignment.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace pirgpu {
namespace rpk {

constexpr uint8_t kPackedComprByte = 0x80;   // inner IntArray header byte 5 of a packed reply ciphertext (SEAL: 0, 1)

inline uint32_t width(uint64_t q) {          // bit length of q - 1 (q >= 2)
  uint32_t w = 0;
  for (uint64_t v = q - 1; v; v >>= 1) ++w;
  return w;
}
inline size_t poly_words(uint32_t N, uint32_t w) { return (size_t)N * w / 64; }
inline size_t ct_words(uint32_t N, const uint64_t* q, uint32_t r) {
  size_t s = 0;
  for (uint32_t j = 0; j < r; ++j) s += poly_words(N, width(q[j]));
  return 2 * s;
}

// x[N] (values < 2^w, 1 <= w <= 64) -> out[N w / 64], `out` at any alignment
inline void pack_poly(const uint64_t* x, uint32_t N, uint32_t w, void* out) {
  uint8_t* o = static_cast<uint8_t*>(out);
  uint64_t acc = 0;       // the bits of the word being filled
  uint32_t have = 0;      // how many of them are set
  for (uint32_t i = 0; i < N; ++i) {
    const uint64_t v = x[i];
    acc |= v << have;     // have < 64
    if (have + w >= 64) {
      memcpy(o, &acc, 8);
      o += 8;
      const uint32_t used = 64 - have;           // bits of v that went into the stored word, 1 .. 64
      acc = used < 64 ? v >> used : 0;
      have = w - used;
    } else {
      have += w;
    }
  }
}

// in[N w / 64] at any alignment -> out[N]; returns false if a coefficient is >= q (every coefficient is still written)
inline bool unpack_poly(const void* in, uint32_t N, uint32_t w, uint64_t q, uint64_t* out) {
  const uint8_t* p = static_cast<const uint8_t*>(in);
  const uint64_t mask = w >= 64 ? ~0ull : (1ull << w) - 1;
  uint64_t acc = 0;       // unread bits of the current word, at the bottom
  uint32_t have = 0;
  uint64_t bad = 0;
  for (uint32_t i = 0; i < N; ++i) {
    uint64_t v;
    if (have >= w) {
      v = acc & mask;
      acc = w < 64 ? acc >> w : 0;
      have -= w;
    } else {
      uint64_t next;
      memcpy(&next, p, 8);
      p += 8;
      v = have ? (acc | next << have) & mask : next & mask;
      const uint32_t took = w - have;            // bits taken from `next`, 1 .. 64
      acc = took < 64 ? next >> took : 0;
      have = 64 - took;
    }
    out[i] = v;
    bad |= (uint64_t)(v >= q);
  }
  return !bad;
}

// unpack_poly for its verdict alone: in[N w / 64] at any alignment, nothing stored; false if a coefficient is >= q
// (compact queries, DESIGN.md section 6.9: the host checks what the device unpacks)
inline bool check_poly(const void* in, uint32_t N, uint32_t w, uint64_t q) {
  const uint8_t* p = static_cast<const uint8_t*>(in);
  const uint64_t mask = w >= 64 ? ~0ull : (1ull << w) - 1;
  uint64_t acc = 0;       // unread bits of the current word, at the bottom
  uint32_t have = 0;
  uint64_t bad = 0;
  for (uint32_t i = 0; i < N; ++i) {
    uint64_t v;
    if (have >= w) {
      v = acc & mask;
      acc = w < 64 ? acc >> w : 0;
      have -= w;
    } else {
      uint64_t next;
      memcpy(&next, p, 8);
      p += 8;
      v = have ? (acc | next << have) & mask : next & mask;
      const uint32_t took = w - have;            // bits taken from `next`, 1 .. 64
      acc = took < 64 ? next >> took : 0;
      have = 64 - took;
    }
    bad |= (uint64_t)(v >= q);
  }
  return !bad;
}

// ct [2][in_r][N], the first r residues of each component -> out[ct_words(N, q, r)]
inline void pack_ct(const uint64_t* ct, uint32_t N, const uint64_t* q, uint32_t r, uint32_t in_r, void* out) {
  uint8_t* o = static_cast<uint8_t*>(out);
  for (uint32_t c = 0; c < 2; ++c)
    for (uint32_t j = 0; j < r; ++j) {
      const uint32_t w = width(q[j]);
      pack_poly(ct + ((size_t)c * in_r + j) * N, N, w, o);
      o += poly_words(N, w) * 8;
    }
}

// packed[ct_words(N, q, r)] -> out [2][r][N]; false if any coefficient is >= its modulus
inline bool unpack_ct(const void* packed, uint32_t N, const uint64_t* q, uint32_t r, uint64_t* out) {
  const uint8_t* p = static_cast<const uint8_t*>(packed);
  bool ok = true;
  for (uint32_t c = 0; c < 2; ++c)
    for (uint32_t j = 0; j < r; ++j) {
      const uint32_t w = width(q[j]);
      ok &= unpack_poly(p, N, w, q[j], out + ((size_t)c * r + j) * N);
      p += poly_words(N, w) * 8;
    }
  return ok;
}

}  // namespace rpk
}  // namespace pirgpu
