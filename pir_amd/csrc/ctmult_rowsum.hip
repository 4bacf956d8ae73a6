// ctmult_rowsum.hip -- gfx950 kernels of the deferred rounding of the ciphertext-multiplication mode (ctmult.h, DESIGN.md
// section 6.6, PIRGPU_CREATE_CT_DEFERRED):
//
//   ctm_tensor_rowsum_kernel   the dyadic tensor (a0 b0, a0 b1 + a1 b0, a1 b1) summed over the children of a row, at one base
//   ctm_fold_partials_kernel   the sum of the partial row sums when a row's children were shared out over workgroups
//
// 64-bit integer arithmetic (arith.h) on the canonical NTT-form residues ntt_batch leaves, whatever the flavour of the
// transforms.  The modulus comes from blockIdx: one instantiation serves every k.  No LDS.
#include <hip/hip_runtime.h>

#include "arith.h"
#include "ctmult.h"

namespace pirgpu {

namespace {

constexpr int kBlock = 256;

// Deferred rounding: acc[(row - row0) * nq + q][3][km][N] (+)= sum over the children j of `row` in this workgroup's share of
// the block [j0, j0 + nj) of (a0 b0, a0 b1 + a1 b0, a1 b1) mod the modulus, from x [nj * nq][4][km][N] (NTT form, canonical,
// pair = (j - j0) * nq + q).  grid (N / 256, km, rows * nq * splits): one thread per output word and split, looping over
// the children.  Products are summed unreduced in 128 bits and folded every lazy_limit PRODUCTS -- x1 takes two per child,
// so every lazy_limit / 2 children; a folded sum is carried on as a residue (AccWide's rule: lazy_limit (q - 1)^2 + q <
// 2^128).  splits = 1: the result goes to acc, and a row whose first child lies before j0 adds to what acc holds.
// splits > 1: split s takes the children [j0 + s * cj, j0 + (s + 1) * cj) and writes its partial sum (zero when that
// share holds none of the row) to acc + (s + 1) * rows * nq accumulators; ctm_fold_partials_kernel adds them up.
__global__ void __launch_bounds__(kBlock)
ctm_tensor_rowsum_kernel(const DevParams* __restrict__ P, uint32_t km, uint32_t N, const uint64_t* __restrict__ x,
                         uint64_t* __restrict__ acc, uint32_t dim, uint32_t nq, uint32_t j0, uint32_t nj, uint32_t row0,
                         uint32_t rows, uint32_t splits, uint32_t cj) {
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
  while (lo < hi) {
    const uint64_t stop = hi - lo > per ? lo + per : hi;
    const uint64_t* in = x + (((size_t)(lo - j0) * nq + q) * 4 * km + m) * N + i;
    const size_t step = (size_t)nq * 4 * poly;
#pragma unroll 2
    for (uint64_t j = lo; j < stop; ++j, in += step) {
      const uint64_t a0 = in[0], a1 = in[poly], b0 = in[2 * poly], b1 = in[3 * poly];
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

// grid (N / 256, 3 * km, rows * nq): acc[slot] = (carry of slot) + sum over the splits of their partial sums
__global__ void __launch_bounds__(kBlock)
ctm_fold_partials_kernel(const DevParams* __restrict__ P, uint32_t km, uint32_t N, uint64_t* __restrict__ acc, uint32_t nq,
                         uint32_t splits, uint32_t carry) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x, m = blockIdx.y % km, slot = blockIdx.z;
  const uint32_t slots = gridDim.z;
  const uint64_t qm = P->mod[m].q;
  const size_t word = ((size_t)slot * 3 * km + blockIdx.y) * N + i, part = (size_t)slots * 3 * km * N;
  uint64_t v = carry && slot < nq ? acc[word] : 0;   // the carried row is the block's first
  for (uint32_t s = 1; s <= splits; ++s) v = add_mod(v, acc[word + s * part], qm);
  acc[word] = v;
}

}  // namespace

hipError_t launch_ctm_tensor_rowsum(hipStream_t st, const DevParams* P, uint32_t km, uint32_t N, const uint64_t* x,
                                    uint64_t* acc, uint32_t dim, uint32_t nq, uint32_t j0, uint32_t nj, uint32_t splits) {
  if (!nj) return hipSuccess;
  if (N % kBlock || km < 1 || km > (uint32_t)kMaxPrimes || !dim || !nq || !splits || splits > nj) return hipErrorInvalidValue;
  const uint32_t row0 = j0 / dim, rows = (uint32_t)(((uint64_t)j0 + nj - 1) / dim) - row0 + 1;
  if ((uint64_t)rows * nq * splits > 65535) return hipErrorInvalidValue;
  const uint32_t cj = (nj + splits - 1) / splits;
  hipLaunchKernelGGL(ctm_tensor_rowsum_kernel, dim3(N / kBlock, km, rows * nq * splits), dim3(kBlock), 0, st, P, km, N, x,
                     acc, dim, nq, j0, nj, row0, rows, splits, cj);
  if (splits > 1) return launch_ctm_fold_partials(st, P, km, N, acc, nq, rows, splits, (uint64_t)row0 * dim < j0);
  return hipGetLastError();
}

hipError_t launch_ctm_fold_partials(hipStream_t st, const DevParams* P, uint32_t km, uint32_t N, uint64_t* acc, uint32_t nq,
                                    uint32_t rows, uint32_t splits, bool carry) {
  if (N % kBlock || km < 1 || km > (uint32_t)kMaxPrimes || !nq || !rows || (uint64_t)rows * nq > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ctm_fold_partials_kernel, dim3(N / kBlock, 3 * km, rows * nq), dim3(kBlock), 0, st, P, km, N, acc, nq,
                     splits, (uint32_t)carry);
  return hipGetLastError();
}

}  // namespace pirgpu
