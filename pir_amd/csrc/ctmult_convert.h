// ctmult_convert.h -- the exact base conversion of the ciphertext-multiplication mode (ctmult.h), shared
// by the translation units whose kernels lift polynomials to the auxiliary base (ctmult.hip, ctmult_shared.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "arith.h"
#include "ctmult.h"

namespace pirgpu {

// Exact base conversion (CtmConv): x[KS] canonical residues at the source moduli -> out[KT] canonical residues at the
// targets of the lift in [0, P), or (centred) of the lift in [-(P - 1) / 2, (P - 1) / 2].
template <int KS, int KT>
__device__ __forceinline__ void ctm_convert(const uint64_t (&x)[KS], uint64_t (&out)[KT], const CtmConv& C, bool centred) {
  uint64_t v[KS];
#pragma unroll
  for (int j = 0; j < KS; ++j) {
    const uint64_t sj = C.s[j].q;
    uint64_t u = x[j];
#pragma unroll
    for (int i = 0; i < j; ++i)
      u = mul_shoup(sub_mod(u, reduce64(v[i], C.s[j]), sj), C.inv[i][j].w, C.inv[i][j].ws, sj);
    v[j] = u;
  }
  // x > (P - 1) / 2: the most significant digit that differs decides
  bool above = false, decided = !centred;
#pragma unroll
  for (int j = KS - 1; j >= 0; --j) {
    const uint64_t hj = C.half[j];
    if (!decided && v[j] != hj) {
      above = v[j] > hj;
      decided = true;
    }
  }
#pragma unroll
  for (int i = 0; i < KT; ++i) {
    const ModConst m = C.t[i];
    uint64_t r = reduce64(v[KS - 1], m);
#pragma unroll
    for (int j = KS - 2; j >= 0; --j)
      r = add_mod(mul_shoup(r, C.s_mod_t[j][i].w, C.s_mod_t[j][i].ws, m.q), reduce64(v[j], m), m.q);
    out[i] = above ? sub_mod(r, C.P_mod_t[i], m.q) : r;
  }
}

}  // namespace pirgpu
