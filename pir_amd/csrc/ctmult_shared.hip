// ctmult_shared.hip -- gfx950 kernels of the shared-selector path of the ciphertext-multiplication mode (ctmult.h, DESIGN.md
// section 6.6, option CT_SHARED_SEL): the selector pair of a product is the same for every row of a level, so it is lifted
// and transformed once per level and group instead of once per pair.
//
//   ctm_lift_polys_kernel         centred lift of single polynomials from Q to the auxiliary base B: the ciphertext halves of
//                                 a block's pairs, or the selectors of a level
//   ctm_tensor_sel_kernel         (x0, x1, x2) = (a0 b0, a0 b1 + a1 b0, a1 b1), dyadic, at one base: a from the block, b
//                                 from the level's selector array
//   ctm_tensor_rowsum_sel_kernel  the same summed over the children of a row (deferred rounding; twin of
//                                 ctm_tensor_rowsum_kernel, ctmult_rowsum.hip, whose fold of the partial sums it shares)
//
// Elementwise, one thread per coefficient, 64-bit integer arithmetic on canonical residues (arith.h): the same modular values
// as the four-polynomial path, bit for bit.  The tensor kernels take the modulus from blockIdx (one instantiation each); the
// lift is instantiated per k like ctm_lift_kernel.  No LDS.
#include <hip/hip_runtime.h>

#include "arith.h"
#include "ctmult.h"
#include "ctmult_convert.h"

namespace pirgpu {

namespace {

constexpr int kBlock = 256;

// grid (N / 256, 2 * n): polynomial `which` of ciphertext a + (c % nq) * a_qstride + (j0 + c / nq) * 2 K N, c < n (the
// addressing of ctm_lift_kernel's ciphertext half; nq = 1, j0 = 0: n ciphertexts back to back) -> xb [n][2][K + 2][N], and
// a copy -> xq [n][2][K][N] unless xq is null.
template <int K>
__global__ void __launch_bounds__(kBlock)
ctm_lift_polys_kernel(const CtmParams* __restrict__ P, const uint64_t* __restrict__ a, uint64_t a_qstride, uint32_t nq,
                      uint32_t j0, uint64_t* __restrict__ xq, uint64_t* __restrict__ xb) {
  constexpr int KB = K + 2;
  const uint32_t N = P->N;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t ct = blockIdx.y >> 1, which = blockIdx.y & 1;
  const uint32_t q = ct % nq, j = j0 + ct / nq;
  const uint64_t* src = a + (size_t)q * a_qstride + ((size_t)j * 2 + which) * K * N;
  uint64_t x[K], y[KB];
#pragma unroll
  for (int m = 0; m < K; ++m) x[m] = src[(size_t)m * N + i];
  ctm_convert<K, KB>(x, y, P->q2b, true);
  if (xq) {
    uint64_t* oq = xq + (size_t)blockIdx.y * K * N;
#pragma unroll
    for (int m = 0; m < K; ++m) oq[(size_t)m * N + i] = x[m];
  }
  uint64_t* ob = xb + (size_t)blockIdx.y * KB * N;
#pragma unroll
  for (int m = 0; m < KB; ++m) ob[(size_t)m * N + i] = y[m];
}

// grid (N / 256, km, pairs): pair p = jj * nq + q takes a from x [n][2][km][N] and b from sel.p[q] + ((j0 + jj) % dim) * 2 km N
__global__ void __launch_bounds__(kBlock)
ctm_tensor_sel_kernel(const DevParams* __restrict__ P, uint32_t km, uint32_t N, const uint64_t* __restrict__ x, CtmSelPtrs sel,
                      uint32_t dim, uint32_t nq, uint32_t j0, uint64_t* __restrict__ y) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x, m = blockIdx.y, pair = blockIdx.z;
  const uint32_t q = pair % nq, j = j0 + pair / nq;
  const ModConst mc = P->mod[m];
  const size_t poly = (size_t)km * N;
  const uint64_t* in = x + ((size_t)pair * 2 * km + m) * N + i;
  const uint64_t* s = sel.p[q] + ((size_t)(j % dim) * 2 * km + m) * N + i;
  const uint64_t a0 = in[0], a1 = in[poly], b0 = s[0], b1 = s[poly];
  uint64_t* out = y + ((size_t)pair * 3 * km + m) * N + i;
  out[0] = mul_mod(a0, b0, mc);
  out[poly] = add_mod(mul_mod(a0, b1, mc), mul_mod(a1, b0, mc), mc.q);
  out[2 * poly] = mul_mod(a1, b1, mc);
}

// ctm_tensor_rowsum_kernel (ctmult_rowsum.hip: grid, lazy sums, splits and partial accumulators are its) with a from
// x [nj * nq][2][km][N] and b from the selector array.
__global__ void __launch_bounds__(kBlock)
ctm_tensor_rowsum_sel_kernel(const DevParams* __restrict__ P, uint32_t km, uint32_t N, const uint64_t* __restrict__ x,
                             CtmSelPtrs sel, uint64_t* __restrict__ acc, uint32_t dim, uint32_t nq, uint32_t j0, uint32_t nj,
                             uint32_t row0, uint32_t rows, uint32_t splits, uint32_t cj) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x, m = blockIdx.y;
  const uint32_t slots = rows * nq;
  const uint32_t slot = blockIdx.z % slots, s = blockIdx.z / slots;
  const uint32_t q = slot % nq, row = row0 + slot / nq;
  const ModConst mc = P->mod[m];
  const uint32_t per = P->lazy_limit > 2 ? P->lazy_limit >> 1 : 1;   // children between two folds
  const uint64_t first = (uint64_t)row * dim, last = first + dim;    // children [first, last) of this row
  const uint64_t b_lo = splits > 1 ? (uint64_t)j0 + (uint64_t)s * cj : j0;
  const uint64_t b_hi = splits > 1 ? (b_lo + cj < (uint64_t)j0 + nj ? b_lo + cj : (uint64_t)j0 + nj) : (uint64_t)j0 + nj;
  uint64_t lo = first > b_lo ? first : b_lo;
  const uint64_t hi = last < b_hi ? last : b_hi;
  const size_t poly = (size_t)km * N;
  uint64_t* out = acc + (((size_t)(splits > 1 ? s + 1 : 0) * slots + slot) * 3 * km + m) * N + i;
  u128 s0 = 0, s1 = 0, s2 = 0;
  if (splits == 1 && first < j0) {
    s0 = out[0];
    s1 = out[poly];
    s2 = out[2 * poly];
  }
  const uint64_t* selq = sel.p[q] + (size_t)m * N + i;
  while (lo < hi) {
    const uint64_t stop = hi - lo > per ? lo + per : hi;
    const uint64_t* in = x + (((size_t)(lo - j0) * nq + q) * 2 * km + m) * N + i;
    const uint64_t* b = selq + (size_t)(lo - first) * 2 * poly;   // child j of the row reads selector j - first = j % dim
    const size_t step = (size_t)nq * 2 * poly;
#pragma unroll 2
    for (uint64_t j = lo; j < stop; ++j, in += step, b += 2 * poly) {
      const uint64_t a0 = in[0], a1 = in[poly], b0 = b[0], b1 = b[poly];
      s0 += (u128)a0 * b0;
      s1 += (u128)a0 * b1;
      s1 += (u128)a1 * b0;
      s2 += (u128)a1 * b1;
    }
    lo = stop;
    s0 = reduce128((uint64_t)s0, (uint64_t)(s0 >> 64), mc);
    s1 = reduce128((uint64_t)s1, (uint64_t)(s1 >> 64), mc);
    s2 = reduce128((uint64_t)s2, (uint64_t)(s2 >> 64), mc);
  }
  out[0] = (uint64_t)s0;
  out[poly] = (uint64_t)s1;
  out[2 * poly] = (uint64_t)s2;
}

}  // namespace

hipError_t launch_ctm_lift_polys(hipStream_t st, const CtmParams* P, uint32_t k, uint32_t N, const uint64_t* a,
                                 uint64_t a_qstride, uint32_t nq, uint32_t j0, uint32_t n, uint64_t* xq, uint64_t* xb) {
  if (!n) return hipSuccess;
  if (N % kBlock || n > 32767 || !nq) return hipErrorInvalidValue;
  const dim3 grid(N / kBlock, n * 2);
  switch (k) {
    case 1: hipLaunchKernelGGL(ctm_lift_polys_kernel<1>, grid, dim3(kBlock), 0, st, P, a, a_qstride, nq, j0, xq, xb); break;
    case 2: hipLaunchKernelGGL(ctm_lift_polys_kernel<2>, grid, dim3(kBlock), 0, st, P, a, a_qstride, nq, j0, xq, xb); break;
    case 3: hipLaunchKernelGGL(ctm_lift_polys_kernel<3>, grid, dim3(kBlock), 0, st, P, a, a_qstride, nq, j0, xq, xb); break;
    case 4: hipLaunchKernelGGL(ctm_lift_polys_kernel<4>, grid, dim3(kBlock), 0, st, P, a, a_qstride, nq, j0, xq, xb); break;
    case 5: hipLaunchKernelGGL(ctm_lift_polys_kernel<5>, grid, dim3(kBlock), 0, st, P, a, a_qstride, nq, j0, xq, xb); break;
    case 6: hipLaunchKernelGGL(ctm_lift_polys_kernel<6>, grid, dim3(kBlock), 0, st, P, a, a_qstride, nq, j0, xq, xb); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_ctm_tensor_sel(hipStream_t st, const DevParams* P, uint32_t km, uint32_t N, const uint64_t* x,
                                 const CtmSelPtrs& sel, uint32_t dim, uint32_t nq, uint32_t j0, uint64_t* y, uint32_t n) {
  if (!n) return hipSuccess;
  if (N % kBlock || n > 65535 || km < 1 || km > (uint32_t)kMaxPrimes || !dim || !nq || nq > (uint32_t)kCtmMaxSel)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(ctm_tensor_sel_kernel, dim3(N / kBlock, km, n), dim3(kBlock), 0, st, P, km, N, x, sel, dim, nq, j0, y);
  return hipGetLastError();
}

hipError_t launch_ctm_tensor_rowsum_sel(hipStream_t st, const DevParams* P, uint32_t km, uint32_t N, const uint64_t* x,
                                        const CtmSelPtrs& sel, uint64_t* acc, uint32_t dim, uint32_t nq, uint32_t j0,
                                        uint32_t nj, uint32_t splits) {
  if (!nj) return hipSuccess;
  if (N % kBlock || km < 1 || km > (uint32_t)kMaxPrimes || !dim || !nq || nq > (uint32_t)kCtmMaxSel || !splits || splits > nj)
    return hipErrorInvalidValue;
  const uint32_t row0 = j0 / dim, rows = (uint32_t)(((uint64_t)j0 + nj - 1) / dim) - row0 + 1;
  if ((uint64_t)rows * nq * splits > 65535) return hipErrorInvalidValue;
  const uint32_t cj = (nj + splits - 1) / splits;
  hipLaunchKernelGGL(ctm_tensor_rowsum_sel_kernel, dim3(N / kBlock, km, rows * nq * splits), dim3(kBlock), 0, st, P, km, N, x,
                     sel, acc, dim, nq, j0, nj, row0, rows, splits, cj);
  if (splits > 1)
    return launch_ctm_fold_partials(st, P, km, N, acc, nq, rows, splits, (uint64_t)row0 * dim < j0);
  return hipGetLastError();
}

}  // namespace pirgpu
