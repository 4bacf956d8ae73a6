// reply_pack.hip -- packed replies (PIRGPU_CREATE_PACKED_REPLIES): canonical u64 residues to the
// bit width of their moduli, on the device, right where a reply is produced.  The host twin is reply_pack.h.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace pirgpu {

// [query][ct][2][in_r][N] u64 -> [query][ct][packed words].  Polynomial (c, j), j < r, of width w = args.w[j] becomes the
// little-endian bit stream of its N coefficients, w bits each, as N w / 64 words at args.off[j] (+ half a ciphertext for
// c = 1).  One thread owns one output word: stream bits [64 m, 64 m + 64) come from the coefficients floor(64 m / w) ..
// floor((64 m + 63) / w), at most ceil(64 / w) + 1 of them; the first is found with one 32-bit division per WORD (w is
// uniform per polynomial, so no coefficient is divided), the rest follow w bits apart.  Lanes of a wave store consecutive
// 8-byte words and read a contiguous run of coefficients (neighbouring lanes share the one that straddles their words:
// the second read hits the cache).  No LDS, no scratch: the loop keeps one word and one coefficient in registers.
// grid = (ceil(max words per polynomial / 256), cts * 2 * r, queries).
__global__ void __launch_bounds__(256)
reply_pack_kernel(const uint64_t* __restrict__ in_all, uint64_t* __restrict__ out_all, ReplyPackArgs args,
                  uint64_t in_qstride, uint64_t out_qstride) {
  const uint32_t r = args.r, N = args.N;
  const uint32_t poly = blockIdx.y;                 // (ct * 2 + c) * r + j
  const uint32_t j = poly % r, cc = poly / r;       // uniform per workgroup
  const uint32_t c = cc & 1, ct = cc >> 1;
  const uint32_t w = args.w[j];
  const uint32_t m = blockIdx.x * 256 + threadIdx.x;
  if (m >= N / 64 * w) return;
  const uint64_t* x = in_all + (size_t)blockIdx.z * in_qstride + ((size_t)(ct * 2 + c) * args.in_r + j) * N;
  uint64_t* out = out_all + (size_t)blockIdx.z * out_qstride + (size_t)ct * args.ct_words + (size_t)c * (args.ct_words / 2) +
                  args.off[j] + m;
  const uint32_t s0 = m * 64;                       // first stream bit of this word (< 2^21 * 64: N w <= 32768 * 64)
  uint32_t i = s0 / w;
  const uint32_t skip = s0 - i * w;                 // bits of coefficient i that belong to the word before, < w
  uint64_t word = x[i] >> skip;
  uint32_t have = w - skip;                         // 1 .. w
  while (have < 64) {                               // i + 1 < N here: the stream ends on a word boundary
    word |= x[++i] << have;
    have += w;
  }
  *out = word;
}

hipError_t launch_reply_pack(hipStream_t st, const ReplyPackArgs& args, const uint64_t* in, uint64_t* out, uint64_t n_cts,
                             uint32_t n_queries, uint64_t in_qstride, uint64_t out_qstride) {
  if (!n_cts || !n_queries) return hipSuccess;
  if (args.r < 1 || args.r > (uint32_t)kMaxPrimes || args.in_r < args.r || args.N < 64 || args.N % 64 || args.N > 32768)
    return hipErrorInvalidValue;
  uint32_t wmax = 0, at = 0;
  for (uint32_t j = 0; j < args.r; ++j) {           // the offsets must be the layout the widths define
    if (args.w[j] < 1 || args.w[j] > 64 || args.off[j] != at) return hipErrorInvalidValue;
    at += args.N / 64 * args.w[j];
    wmax = args.w[j] > wmax ? args.w[j] : wmax;
  }
  if (args.ct_words != 2 * at) return hipErrorInvalidValue;
  const uint64_t polys = n_cts * 2 * args.r;
  if (polys > 65535 || n_queries > 65535) return hipErrorInvalidValue;
  const dim3 grid((args.N / 64 * wmax + 255) / 256, (uint32_t)polys, n_queries);
  hipLaunchKernelGGL(reply_pack_kernel, grid, dim3(256), 0, st, in, out, args, in_qstride, out_qstride);
  return hipGetLastError();
}

ReplyPackArgs reply_pack_args(uint32_t N, const uint64_t* q, uint32_t r, uint32_t in_r) {
  ReplyPackArgs a{};
  a.N = N;
  a.r = r;
  a.in_r = in_r;
  uint32_t at = 0;
  for (uint32_t j = 0; j < r && j < (uint32_t)kMaxPrimes; ++j) {
    uint32_t w = 0;
    for (uint64_t v = q[j] - 1; v; v >>= 1) ++w;
    a.w[j] = w;
    a.off[j] = at;
    at += N / 64 * w;
  }
  a.ct_words = 2 * at;
  return a;
}

}  // namespace pirgpu
