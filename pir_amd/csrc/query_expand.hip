// query_expand.hip -- compact queries: the c0 half of a compact query ciphertext from its wire
// form to canonical u64 residues, on the device, right where the query is staged.  The inverse of reply_pack.hip; the
// host twin is rpk::unpack_poly (reply_pack.h).  The c1 half is re-sampled from the seed by seed_expand.hip.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "reply_pack.h"

namespace pirgpu {

// [query][ct][obj_words] u64 -> the c0 half of [query][ct][ct_stride].  A compact ciphertext is k polynomials, number j
// the little-endian bit stream of its N coefficients at w = args.w[j] bits each (N w / 64 words at args.off[j]; w = 64
// is the plain form), followed by the 8 words of its seed.  One thread owns one output coefficient: its bits start at
// stream bit i w, so it reads word i w / 64 and, when the coefficient straddles, the word behind it (w is uniform per
// polynomial and the division is by 64: a shift).  Lanes of a wave read a contiguous run of source words (neighbours
// share them: w / 64 of a new word per lane) and store consecutive 8-byte residues.  The workgroup of polynomial 0 that
// holds coefficient 0 also copies the ciphertext's seed to seeds[query][ct][8], the contiguous array seed_expand_kernel
// reads.  No LDS, no scratch.  grid = (N / 256, cts * k, queries).
__global__ void __launch_bounds__(256)
query_unpack_kernel(const uint64_t* __restrict__ in_all, uint64_t* __restrict__ out_all, uint64_t* __restrict__ seeds_all,
                    QueryUnpackArgs args, uint32_t n_cts, uint64_t ct_stride, uint64_t out_qstride) {
  const uint32_t k = args.k, N = args.N;
  const uint32_t j = blockIdx.y % k, ct = blockIdx.y / k;   // uniform per workgroup
  const uint32_t w = args.w[j];
  const size_t obj = (size_t)blockIdx.z * n_cts + ct;
  const uint64_t* src = in_all + obj * args.obj_words;
  if (j == 0 && blockIdx.x == 0 && threadIdx.x < 8) seeds_all[obj * 8 + threadIdx.x] = src[args.obj_words - 8 + threadIdx.x];
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  src += args.off[j];
  const uint32_t bit = i * w;                       // < 2^21: N w <= 32768 * 64
  const uint32_t m = bit >> 6, sh = bit & 63;
  uint64_t v = src[m] >> sh;
  if (sh + w > 64) v |= src[m + 1] << (64 - sh);    // sh > 0 here, and m + 1 < N w / 64: the stream ends on a word boundary
  if (w < 64) v &= (1ull << w) - 1;
  out_all[(size_t)blockIdx.z * out_qstride + (size_t)ct * ct_stride + (size_t)j * N + i] = v;
}

hipError_t launch_query_unpack(hipStream_t st, const QueryUnpackArgs& args, const uint64_t* in, uint64_t* out, uint64_t* seeds,
                               uint32_t n_cts, uint64_t ct_stride, uint32_t n_queries, uint64_t out_qstride) {
  if (!n_cts || !n_queries) return hipSuccess;
  if (args.k < 1 || args.k > (uint32_t)kMaxPrimes || args.N < 64 || args.N % 64 || args.N > 32768) return hipErrorInvalidValue;
  uint32_t at = 0;
  for (uint32_t j = 0; j < args.k; ++j) {           // the offsets must be the layout the widths define
    if (args.w[j] < 1 || args.w[j] > 64 || args.off[j] != at) return hipErrorInvalidValue;
    at += args.N / 64 * args.w[j];
  }
  if (args.obj_words != at + 8 || ct_stride < (uint64_t)args.k * args.N) return hipErrorInvalidValue;
  const uint64_t polys = (uint64_t)n_cts * args.k;
  if (polys > 65535 || n_queries > 65535) return hipErrorInvalidValue;
  const dim3 grid((args.N + 255) / 256, (uint32_t)polys, n_queries);
  hipLaunchKernelGGL(query_unpack_kernel, grid, dim3(256), 0, st, in, out, seeds, args, n_cts, ct_stride, out_qstride);
  return hipGetLastError();
}

QueryUnpackArgs query_unpack_args(uint32_t N, const uint64_t* q, uint32_t k, bool packed) {
  QueryUnpackArgs a{};
  a.N = N;
  a.k = k;
  uint32_t at = 0;
  for (uint32_t j = 0; j < k && j < (uint32_t)kMaxPrimes; ++j) {
    const uint32_t w = packed ? rpk::width(q[j]) : 64;   // the layout of reply_pack.h, the one the codec sizes by
    a.w[j] = (uint8_t)w;
    a.off[j] = at;
    at += (uint32_t)rpk::poly_words(N, w);
  }
  a.obj_words = at + 8;
  return a;
}

}  // namespace pirgpu
