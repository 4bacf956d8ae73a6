// ctmult.h -- ciphertext-multiplication mode: the auxiliary base, the constants of the exact base
// conversions and the launch wrappers of ctmult.hip, ctmult_rowsum.hip (deferred rounding) and ctmult_shared.hip (shared selectors).
//
// The product of two ciphertexts is the EXACT BFV product: x0 = a0 b0, x1 = a0 b1 + a1 b0, x2 = a1 b1 over Z[x]/(x^N + 1)
// on the centred lifts, d_i = floor((t x_i + h) / Q), h = (Q - 1) / 2.  The ring products run as dyadic products at the
// 2k + 2 moduli of Q and of an auxiliary base B (k + 2 primes), wide enough to hold t x + h without wrap-around; the one
// primitive beside the transforms is the exact base conversion (Garner digits, centring by digit comparison, Horner).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "device_params.h"
#include "host_math.h"

namespace pirgpu {

constexpr int kCtmMaxQ = 6;              // data primes a ciphertext-multiplication context may have ...
constexpr int kCtmMaxB = kCtmMaxQ + 2;   // ... so that the auxiliary base fits a DevParams (kMaxPrimes)
static_assert(kCtmMaxB <= kMaxPrimes, "the auxiliary base is transformed through a DevParams of its own");

// Exact conversion of a value given by its residues at the source moduli s_0 .. s_{n-1} (product P) to the target
// moduli: mixed-radix digits v (x = v_0 + v_1 s_0 + v_2 s_0 s_1 + ...), the digits of (P - 1) / 2 for the centring
// decision, Horner into every target.
struct CtmConv {
  ModConst s[kCtmMaxB];
  Twiddle inv[kCtmMaxB][kCtmMaxB];       // [i][j], i < j: s_i^-1 mod s_j
  uint64_t half[kCtmMaxB];               // mixed-radix digits of (P - 1) / 2
  ModConst t[kCtmMaxB];
  Twiddle s_mod_t[kCtmMaxB][kCtmMaxB];   // [j][i]: s_j mod t_i
  uint64_t P_mod_t[kCtmMaxB];
};

struct CtmParams {
  uint32_t N, k, kb, pad0;
  CtmConv q2b, b2q;
  uint64_t t_q[kCtmMaxQ], h_q[kCtmMaxQ];   // t and h = (Q - 1) / 2 mod q_j
  uint64_t t_b[kCtmMaxB], h_b[kCtmMaxB];   // ... mod b_i
  Twiddle qinv_b[kCtmMaxB];                // Q^-1 mod b_i
};

// ---- host: little-endian multi-word naturals, just enough for the bound check and the table constants ----
namespace ctm {

typedef std::vector<uint64_t> Nat;

inline void trim(Nat& a) {
  while (!a.empty() && a.back() == 0) a.pop_back();
}
inline Nat nat(uint64_t v) {
  Nat a{v};
  trim(a);
  return a;
}
inline Nat mul(const Nat& a, const Nat& b) {
  Nat r(a.size() + b.size() + 1, 0);
  for (size_t i = 0; i < a.size(); ++i) {
    uint64_t carry = 0;
    for (size_t j = 0; j < b.size(); ++j) {
      hm::u128 cur = (hm::u128)a[i] * b[j] + r[i + j] + carry;
      r[i + j] = (uint64_t)cur;
      carry = (uint64_t)(cur >> 64);
    }
    for (size_t j = i + b.size(); carry; ++j) {
      hm::u128 cur = (hm::u128)r[j] + carry;
      r[j] = (uint64_t)cur;
      carry = (uint64_t)(cur >> 64);
    }
  }
  trim(r);
  return r;
}
inline Nat add(const Nat& a, const Nat& b) {
  Nat r(std::max(a.size(), b.size()) + 1, 0);
  uint64_t carry = 0;
  for (size_t i = 0; i < r.size(); ++i) {
    hm::u128 cur = (hm::u128)(i < a.size() ? a[i] : 0) + (i < b.size() ? b[i] : 0) + carry;
    r[i] = (uint64_t)cur;
    carry = (uint64_t)(cur >> 64);
  }
  trim(r);
  return r;
}
inline Nat sub_small(Nat a, uint64_t v) {   // a >= v
  for (size_t i = 0; i < a.size() && v; ++i) {
    const uint64_t old = a[i];
    a[i] -= v;
    v = old < v ? 1 : 0;
  }
  trim(a);
  return a;
}
inline Nat half(Nat a) {   // floor(a / 2)
  for (size_t i = 0; i < a.size(); ++i) a[i] = (a[i] >> 1) | (i + 1 < a.size() ? a[i + 1] << 63 : 0);
  trim(a);
  return a;
}
inline int cmp(const Nat& a, const Nat& b) {
  if (a.size() != b.size()) return a.size() < b.size() ? -1 : 1;
  for (size_t i = a.size(); i-- > 0;)
    if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  return 0;
}
inline uint64_t mod_small(const Nat& a, uint64_t m) {
  hm::u128 r = 0;
  for (size_t i = a.size(); i-- > 0;) r = ((r << 64) | a[i]) % m;
  return (uint64_t)r;
}
inline Nat product(const uint64_t* p, uint32_t n) {
  Nat r = nat(1);
  for (uint32_t i = 0; i < n; ++i) r = mul(r, nat(p[i]));
  return r;
}

// The auxiliary base of a chain: the k + 2 largest primes == 1 (mod 2N) below 2^bits, bits = the size of the largest data
// prime, found descending, that are neither in the chain nor the special prime.  Returns 0, or a message: more than
// kCtmMaxQ data primes, not enough primes of that size, or a base too small for
//   Q B > 2 (t N (Q - 1)^2 / 2 + Q)   (t x + h does not wrap at Q B)   and   B > 2 (t N Q + 2)   (nor the quotient at B).
// terms = n > 1 (deferred rounding: x is a sum of up to n tensor products):
//   Q B > t n N (Q - 1)^2 + 2 Q   and   B > 2 (t n N Q + 2).
inline const char* plan(uint32_t N, uint32_t k, const uint64_t* q, uint64_t special, uint64_t t, uint64_t* aux,
                        uint64_t terms = 1) {
  if (k < 1 || k > (uint32_t)kCtmMaxQ) return "ciphertext multiplication serves at most 6 data primes (the auxiliary base of k + 2 primes must fit 8)";
  uint64_t qmax = 0;
  for (uint32_t j = 0; j < k; ++j) qmax = std::max(qmax, q[j]);
  if (qmax < 2 || N < 2 || (N & (N - 1)) || terms < 1) return "invalid chain";
  const uint32_t bits = 64 - (uint32_t)__builtin_clzll(qmax);
  uint32_t found = 0;
  for (uint64_t v = (1ull << bits) - 2ull * N + 1; found < k + 2 && v > (1ull << (bits - 1)); v -= 2ull * N) {
    bool taken = v == special;
    for (uint32_t j = 0; j < k; ++j) taken = taken || q[j] == v;
    if (!taken && hm::is_prime(v)) aux[found++] = v;
    if (v < 2ull * N) break;
  }
  if (found < k + 2) return "ciphertext multiplication: not enough NTT-friendly primes of the data primes' size for the auxiliary base";
  const Nat Q = product(q, k), B = product(aux, k + 2);
  const Nat Qm1 = sub_small(Q, 1);
  const Nat tN = mul(mul(nat(t), nat(terms)), nat(N));
  // 2 (t N (Q - 1)^2 / 2 + Q) = t N (Q - 1)^2 + 2 Q   ((Q - 1)^2 is a multiple of 4)
  const Nat need1 = add(mul(tN, mul(Qm1, Qm1)), add(Q, Q));
  const Nat need2 = add(mul(nat(2), mul(tN, Q)), nat(4));
  if (cmp(mul(Q, B), need1) <= 0 || cmp(B, need2) <= 0)
    return terms > 1 ? "ciphertext multiplication: the auxiliary base of k + 2 primes does not hold t n N Q for a sum of n "
                       "products (deferred rounding)"
                     : "ciphertext multiplication: the auxiliary base of k + 2 primes does not hold t N Q (plain modulus too large for this chain)";
  return nullptr;
}

// s: n source moduli, t: m target moduli
inline void fill_conv(CtmConv& c, const uint64_t* s, uint32_t n, const uint64_t* t, uint32_t m) {
  auto mc = [](uint64_t q) {
    ModConst r;
    r.q = q;
    hm::u128 ratio = (~(hm::u128)0) / q;
    r.br_lo = (uint64_t)ratio;
    r.br_hi = (uint64_t)(ratio >> 64);
    return r;
  };
  auto tw = [](uint64_t w, uint64_t q) { return Twiddle{w, hm::shoup(w, q)}; };
  const Nat P = product(s, n);
  const Nat H = half(sub_small(P, 1));
  uint64_t hres[kCtmMaxB];
  for (uint32_t j = 0; j < n; ++j) {
    c.s[j] = mc(s[j]);
    hres[j] = mod_small(H, s[j]);
    for (uint32_t i = 0; i < j; ++i) c.inv[i][j] = tw(hm::invmod_prime(s[i] % s[j], s[j]), s[j]);
  }
  for (uint32_t j = 0; j < n; ++j) {   // Garner on the residues of (P - 1) / 2
    uint64_t u = hres[j];
    for (uint32_t i = 0; i < j; ++i) {
      const uint64_t vi = c.half[i] % s[j];
      u = hm::mulmod(u >= vi ? u - vi : u + s[j] - vi, c.inv[i][j].w, s[j]);
    }
    c.half[j] = u;
  }
  for (uint32_t i = 0; i < m; ++i) {
    c.t[i] = mc(t[i]);
    c.P_mod_t[i] = mod_small(P, t[i]);
    for (uint32_t j = 0; j < n; ++j) c.s_mod_t[j][i] = tw(s[j] % t[i], t[i]);
  }
}

inline void fill_params(CtmParams& p, uint32_t N, uint32_t k, const uint64_t* q, const uint64_t* aux, uint64_t t) {
  p = CtmParams{};
  p.N = N;
  p.k = k;
  p.kb = k + 2;
  fill_conv(p.q2b, q, k, aux, k + 2);
  fill_conv(p.b2q, aux, k + 2, q, k);
  const Nat Q = product(q, k);
  const Nat H = half(sub_small(Q, 1));
  for (uint32_t j = 0; j < k; ++j) {
    p.t_q[j] = t % q[j];
    p.h_q[j] = mod_small(H, q[j]);
  }
  for (uint32_t i = 0; i < k + 2; ++i) {
    p.t_b[i] = t % aux[i];
    p.h_b[i] = mod_small(H, aux[i]);
    const uint64_t qi = hm::invmod_prime(mod_small(Q, aux[i]), aux[i]);
    p.qinv_b[i] = Twiddle{qi, hm::shoup(qi, aux[i])};
  }
}

}  // namespace ctm

// ---- launches (ctmult.hip).  A pair p = jj * nq + q multiplies ciphertext a + q * a_qstride + (j0 + jj) * 2kN with
// selector b + (q * dim + (j0 + jj) % dim) * 2kN; n pairs in all. ----
// xq [n][4][k][N] = (a0, a1, b0, b1) copied, xb [n][4][kb][N] = residues of their centred lifts at B
hipError_t launch_ctm_lift(hipStream_t st, const CtmParams* P, uint32_t k, uint32_t N, const uint64_t* a, uint64_t a_qstride,
                           const uint64_t* b, uint32_t dim, uint32_t nq, uint32_t j0, uint32_t n, uint64_t* xq, uint64_t* xb);
// dyadic tensor at the km "data primes" of P: x [n][4][km][N] (NTT form) -> y [n][3][km][N] = (x0, x1, x2)
hipError_t launch_ctm_tensor(hipStream_t st, const DevParams* P, uint32_t km, uint32_t N, const uint64_t* x, uint64_t* y,
                             uint32_t n);
// yq [n][3][k][N], yb [n][3][kb][N] (coefficient form) -> d [n][3][k][N] in the order (d0, d2, d1): the pair (d0, d2) is
// the ciphertext the key switch of the relinearisation reads
hipError_t launch_ctm_scale(hipStream_t st, const CtmParams* P, uint32_t k, uint32_t N, const uint64_t* yq, const uint64_t* yb,
                            uint64_t* d, uint32_t n);
// out[q][row] (+)= sum over the pairs of this block that are children of `row` of r[p] + (0, d[p].d1); rows whose first
// child lies before j0 add to what `out` holds.  r [n][2][k][N], d as above, out + q * out_qstride + row * 2kN.
hipError_t launch_ctm_accumulate(hipStream_t st, const DevParams* P, uint32_t k, uint32_t N, const uint64_t* r,
                                 const uint64_t* d, uint64_t* out, uint64_t out_qstride, uint32_t dim, uint32_t nq, uint32_t j0,
                                 uint32_t nj, uint32_t rows);
// Deferred rounding: the dyadic tensor summed over the children of a row, at the km "data primes" of P.  x [nj * nq][4][km][N]
// (NTT form, canonical) holds the children [j0, j0 + nj) of every query; acc [(row - j0 / dim) * nq + q][3][km][N] receives,
// for every row with a child in the block, the sum of (x0, x1, x2) over those children, canonical; a row whose first child
// lies before j0 adds to what its accumulator holds.  splits > 1 (<= nj): the block's children are shared out over that
// many workgroups per output word, whose partial sums go to acc + (s + 1) * rows * nq accumulators and are folded by a
// second launch: acc needs room for (splits + 1) * rows * nq accumulators then.
hipError_t launch_ctm_tensor_rowsum(hipStream_t st, const DevParams* P, uint32_t km, uint32_t N, const uint64_t* x,
                                    uint64_t* acc, uint32_t dim, uint32_t nq, uint32_t j0, uint32_t nj, uint32_t splits);
// the second launch of the above on its own: acc[slot] = (its own content if `carry` and slot < nq: the carried row is the
// block's first) + the `splits` partial sums behind the block's rows * nq accumulators
hipError_t launch_ctm_fold_partials(hipStream_t st, const DevParams* P, uint32_t km, uint32_t N, uint64_t* acc, uint32_t nq,
                                    uint32_t rows, uint32_t splits, bool carry);

// ---- shared selectors (ctmult_shared.hip, option CT_SHARED_SEL): the selector pair of pair p = jj * nq + q is read from
// sel.p[q] + ((j0 + jj) % dim) * 2 km N, NTT form at the km moduli of the launch: one array [dim][2][km][N] per query,
// lifted and transformed once per level. ----
constexpr int kCtmMaxSel = 8;   // queries of a group (kMaxMfmaQueries)
struct CtmSelPtrs {             // by-value kernel argument
  const uint64_t* p[kCtmMaxSel];
};
// centred lift of 2 n polynomials: ciphertext c < n is a + (c % nq) * a_qstride + (j0 + c / nq) * 2kN (launch_ctm_lift's
// ciphertext half; nq = 1, j0 = 0: n ciphertexts back to back) -> xb [n][2][kb][N]; xq [n][2][k][N] receives a copy unless null
hipError_t launch_ctm_lift_polys(hipStream_t st, const CtmParams* P, uint32_t k, uint32_t N, const uint64_t* a,
                                 uint64_t a_qstride, uint32_t nq, uint32_t j0, uint32_t n, uint64_t* xq, uint64_t* xb);
// launch_ctm_tensor with a from x [n][2][km][N]
hipError_t launch_ctm_tensor_sel(hipStream_t st, const DevParams* P, uint32_t km, uint32_t N, const uint64_t* x,
                                 const CtmSelPtrs& sel, uint32_t dim, uint32_t nq, uint32_t j0, uint64_t* y, uint32_t n);
// launch_ctm_tensor_rowsum with a from x [nj * nq][2][km][N]
hipError_t launch_ctm_tensor_rowsum_sel(hipStream_t st, const DevParams* P, uint32_t km, uint32_t N, const uint64_t* x,
                                        const CtmSelPtrs& sel, uint64_t* acc, uint32_t dim, uint32_t nq, uint32_t j0,
                                        uint32_t nj, uint32_t splits);

}  // namespace pirgpu
