// ctmult.hip -- gfx950 kernels of the ciphertext-multiplication mode (ctmult.h).
//
//   ctm_lift_kernel        centred lift of the four input polynomials of a product from Q to the auxiliary base B
//   ctm_tensor_kernel      (x0, x1, x2) = (a0 b0, a0 b1 + a1 b0, a1 b1), dyadic, at one base
//   ctm_scale_kernel       d = floor((t x + h) / Q): exact, through B and back
//   ctm_accumulate_kernel  sum of the relinearised products over the children of a row
// (deferred rounding sums the tensor over the children of a row instead: ctmult_rowsum.hip)
//
// All four are elementwise over coefficients, one thread per coefficient, 64-bit integer arithmetic (arith.h).  The
// per-modulus arrays are indexed by unrolled constants only (the kernels are instantiated per k), so they stay in
// registers; the constants are wave-uniform loads.  The transforms between them are the context's own ntt_batch.
#include <hip/hip_runtime.h>

#include "arith.h"
#include "ctmult.h"
#include "ctmult_convert.h"

namespace pirgpu {

namespace {

constexpr int kBlock = 256;

template <int K>
__global__ void __launch_bounds__(kBlock)
ctm_lift_kernel(const CtmParams* __restrict__ P, const uint64_t* __restrict__ a, uint64_t a_qstride,
                const uint64_t* __restrict__ b, uint32_t dim, uint32_t nq, uint32_t j0, uint64_t* __restrict__ xq,
                uint64_t* __restrict__ xb) {
  constexpr int KB = K + 2;
  const uint32_t N = P->N;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t pair = blockIdx.y >> 2, which = blockIdx.y & 3;
  const uint32_t q = pair % nq, j = j0 + pair / nq;
  const uint64_t* src = which < 2 ? a + (size_t)q * a_qstride + ((size_t)j * 2 + which) * K * N
                                  : b + (((size_t)q * dim + j % dim) * 2 + (which - 2)) * K * N;
  uint64_t x[K], y[KB];
#pragma unroll
  for (int m = 0; m < K; ++m) x[m] = src[(size_t)m * N + i];
  ctm_convert<K, KB>(x, y, P->q2b, true);
  uint64_t* oq = xq + (size_t)blockIdx.y * K * N;
  uint64_t* ob = xb + (size_t)blockIdx.y * KB * N;
#pragma unroll
  for (int m = 0; m < K; ++m) oq[(size_t)m * N + i] = x[m];
#pragma unroll
  for (int m = 0; m < KB; ++m) ob[(size_t)m * N + i] = y[m];
}

// grid (N / 256, km, pairs)
__global__ void __launch_bounds__(kBlock)
ctm_tensor_kernel(const DevParams* __restrict__ P, uint32_t km, uint32_t N, const uint64_t* __restrict__ x,
                  uint64_t* __restrict__ y) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x, m = blockIdx.y, pair = blockIdx.z;
  const ModConst mc = P->mod[m];
  const uint64_t* in = x + ((size_t)pair * 4 * km + m) * N + i;
  const size_t poly = (size_t)km * N;
  const uint64_t a0 = in[0], a1 = in[poly], b0 = in[2 * poly], b1 = in[3 * poly];
  uint64_t* out = y + ((size_t)pair * 3 * km + m) * N + i;
  out[0] = mul_mod(a0, b0, mc);
  out[poly] = add_mod(mul_mod(a0, b1, mc), mul_mod(a1, b0, mc), mc.q);
  out[2 * poly] = mul_mod(a1, b1, mc);
}

// grid (N / 256, pairs * 3)
// (the second bound asks for four waves per SIMD: 128 registers, the cap of the project's one-pass kernels -- K = 6, whose
// conversion back from eight auxiliary primes holds the most live words, took 137 without it)
template <int K>
__global__ void __launch_bounds__(kBlock, 4)
ctm_scale_kernel(const CtmParams* __restrict__ P, const uint64_t* __restrict__ yq, const uint64_t* __restrict__ yb,
                 uint64_t* __restrict__ d) {
  constexpr int KB = K + 2;
  const uint32_t N = P->N;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t pair = blockIdx.y / 3, comp = blockIdx.y % 3;
  const uint64_t* inq = yq + (size_t)blockIdx.y * K * N + i;
  const uint64_t* inb = yb + (size_t)blockIdx.y * KB * N + i;
  uint64_t wq[K], wb[KB], rb[KB], out[K];
  // w = t x + h at Q and at B
#pragma unroll
  for (int m = 0; m < K; ++m) {
    const ModConst mc = P->q2b.s[m];
    wq[m] = add_mod(mul_mod(inq[(size_t)m * N], P->t_q[m], mc), P->h_q[m], mc.q);
  }
#pragma unroll
  for (int m = 0; m < KB; ++m) {
    const ModConst mc = P->b2q.s[m];
    wb[m] = add_mod(mul_mod(inb[(size_t)m * N], P->t_b[m], mc), P->h_b[m], mc.q);
  }
  // r = w mod Q in [0, Q), exactly, at B;  y = (w - r) / Q at B;  y (centred) back to Q
  ctm_convert<K, KB>(wq, rb, P->q2b, false);
#pragma unroll
  for (int m = 0; m < KB; ++m) {
    const uint64_t bm = P->b2q.s[m].q;
    wb[m] = mul_shoup(sub_mod(wb[m], rb[m], bm), P->qinv_b[m].w, P->qinv_b[m].ws, bm);
  }
  ctm_convert<KB, K>(wb, out, P->b2q, true);
  // (d0, d2, d1): the key switch of the relinearisation reads (d0, d2) as one ciphertext
  const uint32_t slot = comp == 0 ? 0 : (comp == 2 ? 1 : 2);
  uint64_t* o = d + ((size_t)pair * 3 + slot) * K * N + i;
#pragma unroll
  for (int m = 0; m < K; ++m) o[(size_t)m * N] = out[m];
}

// grid (N / 256, 2 * k, nq * rows): one thread per word of the level's output
__global__ void __launch_bounds__(kBlock)
ctm_accumulate_kernel(const DevParams* __restrict__ P, uint32_t k, uint32_t N, const uint64_t* __restrict__ r,
                      const uint64_t* __restrict__ d, uint64_t* __restrict__ out, uint64_t out_qstride, uint32_t dim,
                      uint32_t nq, uint32_t j0, uint32_t nj, uint32_t rows) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t comp = blockIdx.y / k, m = blockIdx.y % k;
  const uint32_t q = blockIdx.z % nq, row = blockIdx.z / nq;
  const uint64_t first = (uint64_t)row * dim, last = first + dim;   // children [first, last) of this row
  const uint64_t lo = first > j0 ? first : j0, hi = last < (uint64_t)j0 + nj ? last : (uint64_t)j0 + nj;
  if (lo >= hi) return;
  const uint64_t qm = P->mod[m].q;
  uint64_t* o = out + (size_t)q * out_qstride + (((size_t)row * 2 + comp) * k + m) * N + i;
  uint64_t acc = first < j0 ? *o : 0;
  for (uint64_t j = lo; j < hi; ++j) {
    const size_t pair = (size_t)(j - j0) * nq + q;
    acc = add_mod(acc, r[((pair * 2 + comp) * k + m) * N + i], qm);
    if (comp == 1) acc = add_mod(acc, d[((pair * 3 + 2) * k + m) * N + i], qm);
  }
  *o = acc;
}

}  // namespace

#define PIRGPU_CTM_BY_K(k, EXPR)                          \
  switch (k) {                                            \
    case 1: { constexpr int K = 1; EXPR; } break;         \
    case 2: { constexpr int K = 2; EXPR; } break;         \
    case 3: { constexpr int K = 3; EXPR; } break;         \
    case 4: { constexpr int K = 4; EXPR; } break;         \
    case 5: { constexpr int K = 5; EXPR; } break;         \
    case 6: { constexpr int K = 6; EXPR; } break;         \
    default: return hipErrorInvalidValue;                 \
  }

hipError_t launch_ctm_lift(hipStream_t st, const CtmParams* P, uint32_t k, uint32_t N, const uint64_t* a, uint64_t a_qstride,
                           const uint64_t* b, uint32_t dim, uint32_t nq, uint32_t j0, uint32_t n, uint64_t* xq, uint64_t* xb) {
  if (!n) return hipSuccess;
  if (N % kBlock || n > 16383 || !nq || !dim) return hipErrorInvalidValue;
  const dim3 grid(N / kBlock, n * 4);
  PIRGPU_CTM_BY_K(k, hipLaunchKernelGGL(ctm_lift_kernel<K>, grid, dim3(kBlock), 0, st, P, a, a_qstride, b, dim, nq, j0, xq, xb));
  return hipGetLastError();
}

hipError_t launch_ctm_tensor(hipStream_t st, const DevParams* P, uint32_t km, uint32_t N, const uint64_t* x, uint64_t* y,
                             uint32_t n) {
  if (!n) return hipSuccess;
  if (N % kBlock || n > 65535 || km < 1 || km > (uint32_t)kMaxPrimes) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ctm_tensor_kernel, dim3(N / kBlock, km, n), dim3(kBlock), 0, st, P, km, N, x, y);
  return hipGetLastError();
}

hipError_t launch_ctm_scale(hipStream_t st, const CtmParams* P, uint32_t k, uint32_t N, const uint64_t* yq, const uint64_t* yb,
                            uint64_t* d, uint32_t n) {
  if (!n) return hipSuccess;
  if (N % kBlock || n > 21845) return hipErrorInvalidValue;
  const dim3 grid(N / kBlock, n * 3);
  PIRGPU_CTM_BY_K(k, hipLaunchKernelGGL(ctm_scale_kernel<K>, grid, dim3(kBlock), 0, st, P, yq, yb, d));
  return hipGetLastError();
}

hipError_t launch_ctm_accumulate(hipStream_t st, const DevParams* P, uint32_t k, uint32_t N, const uint64_t* r,
                                 const uint64_t* d, uint64_t* out, uint64_t out_qstride, uint32_t dim, uint32_t nq, uint32_t j0,
                                 uint32_t nj, uint32_t rows) {
  if (!nj || !rows) return hipSuccess;
  if (N % kBlock || (uint64_t)nq * rows > 65535 || !dim) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ctm_accumulate_kernel, dim3(N / kBlock, 2 * k, nq * rows), dim3(kBlock), 0, st, P, k, N, r, d, out,
                     out_qstride, dim, nq, j0, nj, rows);
  return hipGetLastError();
}

}  // namespace pirgpu
