// scan_mfma_pair.hip -- the 8-wave digit-sliced scan (scan_mfma.hip) serving TWO groups of up to 8 queries per
// database read.
//
// scan_mfma_kernel<.., 8, ..> waits for its database tiles about half of the time and spends about
// a quarter of it on the matrix cores: a second group's digit products on the SAME A tiles fit under that wait.  A wave
// has no registers for a second set of selector tiles (226 of 256), so the second group's live in LDS: every wave keeps
// the KS * L expanded B tiles of its own slot there (KS * L KiB), written once per unit and read back as MFMA operands
// with one 16-byte read per tile and row tile -- lane l reads the 16 bytes lane l wrote (consecutive lanes, consecutive
// 16 bytes: no bank conflict, no barrier, no cross-lane traffic).
//
// Per row tile: group 0's KS k-steps (B in registers) into T, fold, stage, store; then group 1's KS k-steps (B from LDS)
// into the same T, fold, stage, store.  Ring slot ks of the A tiles is refilled after group 1 has used it, so the
// refill-to-use distance is a whole row tile as in the single kernel while the MFMA work per loaded tile doubles.
// Layouts, fold and result staging are those of scan_mfma.hip / scan_mfma_body.inc; the helpers below are their twins
// (that file's kernels must keep compiling to what they compile to, so nothing is moved out of it).
//
// One column chunk, the whole ring, group-major units only: every other geometry keeps the single kernel.
#include <hip/hip_runtime.h>

#include <stdlib.h>

#include <algorithm>

#include "arith.h"
#include "kernels.h"

namespace pirgpu {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v2i __attribute__((ext_vector_type(2)));

__host__ __device__ __forceinline__ constexpr uint32_t pair_tile_bytes(uint32_t L, bool top4) {
  return top4 ? (L - 1) * 256 + 128 : L * 256;
}
__device__ __forceinline__ uint32_t pair_sx4(uint32_t v) { return v | (((v >> 3) & 0x01010101u) * 0xF0u); }
__device__ __forceinline__ v4i pair_expand_top4(v2i w) {
  const uint32_t w0 = (uint32_t)w[0], w1 = (uint32_t)w[1];
  return v4i{(int)pair_sx4(w0 & 0x0F0F0F0Fu), (int)pair_sx4((w0 >> 4) & 0x0F0F0F0Fu), (int)pair_sx4(w1 & 0x0F0F0F0Fu),
              (int)pair_sx4((w1 >> 4) & 0x0F0F0F0Fu)};
}
__device__ __forceinline__ v4i pair_load_tile(const uint8_t* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const v4i*>(p));
}
__device__ __forceinline__ v2i pair_load_tile8(const uint8_t* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const v2i*>(p));
}
constexpr int kPairBiasBits = 59;   // scan_mfma.hip kBiasBits

}  // namespace

// grid = persistent workgroups; block = 8 waves (wave w <-> slot j0 + w).  Unit u = slot block u of the two groups grp[0]
// and grp[1].
template <int L, int KS, bool TOP4, bool F64F>
__global__ void __launch_bounds__(512)
scan_mfma_pair_kernel(const DevParams* __restrict__ P, const uint8_t* __restrict__ dbp, ScanGroups grp, uint32_t rows,
                      uint32_t RT, uint32_t KG, uint32_t nslots, uint64_t out_qstride) {
  constexpr int NW = 8;
  constexpr uint32_t TB = pair_tile_bytes(L, TOP4);
  constexpr int LF = TOP4 ? L - 1 : L;   // digits stored as full bytes
  constexpr int NS = 2 * L - 1;        // digit diagonals
  constexpr int NG = (NS + 4) / 5;     // groups of five diagonals (40 bits)
  // results of one row tile, [row][x][slot], a (row, x) run padded to 9 words (scan_mfma_body.inc)
  __shared__ __attribute__((aligned(16))) uint64_t stage[2][16][16][NW + 1];
  // group 1's expanded selector tiles, one private region per wave: tile (ks, b), lane l
  __shared__ __attribute__((aligned(16))) v4i selb[NW][KS * L][64];
  // the wave's index as a scalar: slot, slab and selector addresses then live in scalar registers
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), l = threadIdx.x & 63;
  const int g = l >> 4, i16 = l & 15;
  const uint32_t nunits = nslots >> 3;
  const size_t slab = (size_t)RT * KG * TB;                       // database bytes of one slot
  const size_t rt_stride = (size_t)KG * TB;
  const uint32_t lane16 = i16 * 16, lane8 = i16 * 8;              // the lane's bytes inside a full / a nibble tile
  v4i* const myb = &selb[w][0][l];                                // + (ks * L + b) * 64

  v4i B[KS][L], A[KS][LF];
  v2i A4[KS];                           // TOP4: the top digit's tiles, packed
  // group 0's selector tiles of slot jl, into registers
  auto load_B = [&](uint32_t gi, uint32_t jl) __attribute__((always_inline)) {
    const uint8_t* selp = grp.sel[gi];
    const uint32_t nx = 2u * grp.nq[gi];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const uint32_t kg = ks * 4 + g;
      const uint8_t* blk = selp + ((size_t)jl * KG + kg) * TB;
#pragma unroll
      for (int b = 0; b < L; ++b) {
        B[ks][b] = v4i{0, 0, 0, 0};   // columns beyond the group's queries stay zero and are neither packed nor read
        if (kg < KG && (uint32_t)i16 < nx) {
          if (TOP4 && b == L - 1) B[ks][b] = pair_expand_top4(*reinterpret_cast<const v2i*>(blk + b * 256 + lane8));
          else B[ks][b] = *reinterpret_cast<const v4i*>(blk + b * 256 + lane16);
        }
      }
    }
  };
  // group 1's selector tiles of k-step ks of slot jl: loaded as stored (N), expanded and written to LDS later
  v4i N[LF];
  v2i N4;
  auto load_N = [&](uint32_t gi, uint32_t jl, int ks) __attribute__((always_inline)) {
    const uint8_t* selp = grp.sel[gi];
    const uint32_t nx = 2u * grp.nq[gi];
    const uint32_t kg = ks * 4 + g;
    const uint8_t* blk = selp + ((size_t)jl * KG + kg) * TB;
    const bool in = kg < KG && (uint32_t)i16 < nx;
#pragma unroll
    for (int b = 0; b < LF; ++b) {
      N[b] = v4i{0, 0, 0, 0};
      if (in) N[b] = *reinterpret_cast<const v4i*>(blk + b * 256 + lane16);
    }
    N4 = v2i{0, 0};
    if (TOP4 && in) N4 = *reinterpret_cast<const v2i*>(blk + (L - 1) * 256 + lane8);
  };
  auto store_N = [&](int ks) __attribute__((always_inline)) {
#pragma unroll
    for (int b = 0; b < LF; ++b) myb[(ks * L + b) * 64] = N[b];
    if constexpr (TOP4) myb[(ks * L + L - 1) * 64] = pair_expand_top4(N4);
  };
  auto load_A = [&](int ks, const uint8_t* base, uint32_t kg) __attribute__((always_inline)) {
    const uint8_t* blk = base + (size_t)kg * TB;
#pragma unroll
    for (int a = 0; a < LF; ++a) A[ks][a] = pair_load_tile(blk + a * 256 + lane16);
    if constexpr (TOP4) A4[ks] = pair_load_tile8(blk + (L - 1) * 256 + lane8);
  };

  uint32_t u = blockIdx.x;
  if (u >= nunits) return;
  {
    const uint32_t blk = u;
    load_B(0, blk * NW + w);
    const uint8_t* abase = dbp + (size_t)(blk * NW + w) * slab;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const uint32_t kg = ks * 4 + g;
#pragma unroll
      for (int a = 0; a < LF; ++a) A[ks][a] = v4i{0, 0, 0, 0};
      A4[ks] = v2i{0, 0};
      if (kg < KG) load_A(ks, abase, kg);
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      load_N(1, blk * NW + w, ks);
      store_N(ks);
    }
  }

  for (; u < nunits; u += gridDim.x) {
    const uint32_t j0 = u * NW;            // slot of wave 0
    const uint32_t mi = (j0 + w) >> P->logN;
    const ModConst m = P->mod[mi];
    // multiple of q that makes every 40-bit group positive (scan_mfma.hip kBiasBits)
    const uint64_t bias = m.q << (kPairBiasBits - (64 - __builtin_clzll(m.q)));
    [[maybe_unused]] const F64Mod fm{P->tab[mi].qd, P->tab[mi].qinvd};
    [[maybe_unused]] const double fw0 = P->fold_w[mi][0], fw1 = P->fold_w[mi][1], fw2 = P->fold_w[mi][2];
    const uint8_t* abase = dbp + (size_t)(j0 + w) * slab;
    const uint32_t nu = u + gridDim.x;
    const bool has_next = nu < nunits;
    const uint32_t nblk = has_next ? nu : u;
    const uint8_t* nbase = dbp + (size_t)(nblk * NW + w) * slab;

    // fold the diagonals of one group's row tile, stage them and store the 64-byte runs (scan_mfma_body.inc)
    auto fold = [&](v4i (&T)[NS], int buf) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        uint64_t r = 0;
        if constexpr (F64F) {
          // chunks of four diagonals, exact in a double: C_c = ((T[4c+3] 256 + T[4c+2]) 256 + T[4c+1]) 256 + T[4c]
          constexpr int NC = (NS + 3) / 4;
          double acc = 0.0;
#pragma unroll
          for (int c = NC - 1; c >= 0; --c) {
            double C = 0.0;
#pragma unroll
            for (int s = (4 * c + 3 < NS ? 4 * c + 3 : NS - 1); s >= 4 * c; --s) C = __builtin_fma(C, 256.0, (double)T[s][i]);
            if (c == 0) acc += f64_norm(C, fm);
            else acc += f64_mulmod(C, c == 1 ? fw0 : (c == 2 ? fw1 : fw2), fm);
          }
          r = f64_to_u64(f64_canon(f64_norm(acc, fm), fm));
        } else {
#pragma unroll
          for (int gq = NG - 1; gq >= 0; --gq) {
            int64_t G = 0;
#pragma unroll
            for (int s = gq * 5; s < gq * 5 + 5 && s < NS; ++s) G += (int64_t)T[s][i] << (8 * (s - gq * 5));
            if (gq == NG - 1 && NG > 1) {
              r = (uint64_t)(G + (int64_t)bias);   // top group: reduced together with the next one (bias = 0 mod q)
            } else {
              const u128 v = ((u128)r << 40) + (uint64_t)(G + (int64_t)bias);
              r = reduce128((uint64_t)v, (uint64_t)(v >> 64), m);
            }
          }
        }
        stage[buf][g * 4 + i][i16][w] = r;
      }
    };
    auto store = [&](int buf, uint32_t rt, uint32_t nx, uint64_t* obase) __attribute__((always_inline)) {
      __syncthreads();
      // 256 (row, x) runs of 8 slots = 64 bytes each; 512 threads x 16 B, two rounds
#pragma unroll
      for (int round = 0; round < 2; ++round) {
        const int run = round * 128 + (threadIdx.x >> 2);
        const int part = threadIdx.x & 3;
        const int r16 = run >> 4, x = run & 15;
        const uint32_t r = rt * 16 + r16;
        if (x < (int)nx && r < rows) {
          typedef unsigned long long ull2 __attribute__((ext_vector_type(2)));
          const ull2 v = {stage[buf][r16][x][part * 2], stage[buf][r16][x][part * 2 + 1]};   // two 8-byte LDS reads
          uint64_t* dst = obase + (size_t)(x >> 1) * out_qstride + ((size_t)r * 2 + (x & 1)) * nslots + j0 + part * 2;
          *reinterpret_cast<ull2*>(dst) = v;
        }
      }
    };
    const uint32_t nx0 = 2u * grp.nq[0], nx1 = 2u * grp.nq[1];
    uint64_t* const obase0 = grp.out[0];
    uint64_t* const obase1 = grp.out[1];

    for (uint32_t rt = 0; rt < RT; ++rt) {
      v4i T[NS];
      const bool last = rt + 1 == RT;   // wave-uniform
      const uint8_t* next_tile = last ? nbase : abase + (size_t)(rt + 1) * rt_stride;
      const bool refill = !last || has_next;
      const bool next_sel = last && has_next;

      // ---- group 0: selectors in registers
#pragma unroll
      for (int s = 0; s < NS; ++s) T[s] = v4i{0, 0, 0, 0};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        [[maybe_unused]] v4i Atop;
        if constexpr (TOP4) Atop = pair_expand_top4(A4[ks]);
        // the L*L digit products, ordered so that consecutive MFMAs accumulate into different diagonals
#pragma unroll
        for (int off = 0; off < L; ++off)
#pragma unroll
          for (int a = 0; a < L; ++a) {
            const int b = (a + off) % L;
            if (TOP4 && a == L - 1)
              T[a + b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Atop, B[ks][b], T[a + b], 0, 0, 0);
            else
              T[a + b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[ks][a < LF ? a : 0], B[ks][b], T[a + b], 0, 0, 0);
          }
      }
      if (next_sel) load_B(0, nblk * NW + w);   // group 0's MFMAs of this unit are issued: B is free
      fold(T, 0);   // staging buffer 0 for group 0, 1 for group 1: a buffer is rewritten two barriers after it was read
      store(0, rt, nx0, obase0);

      // ---- group 1: selectors from LDS, one read per tile; the same diagonal recurs every L - 1 MFMAs
#pragma unroll
      for (int s = 0; s < NS; ++s) T[s] = v4i{0, 0, 0, 0};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        [[maybe_unused]] v4i Atop;
        if constexpr (TOP4) Atop = pair_expand_top4(A4[ks]);
#pragma unroll
        for (int b = 0; b < L; ++b) {
          const v4i Bt = myb[(ks * L + b) * 64];
#pragma unroll
          for (int a = 0; a < L; ++a) {
            if (TOP4 && a == L - 1) T[a + b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Atop, Bt, T[a + b], 0, 0, 0);
            else T[a + b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[ks][a < LF ? a : 0], Bt, T[a + b], 0, 0, 0);
          }
        }
        // the next unit's tiles of this k-step: in flight under the next k-step (the last k-step's follow the fold)
        if (next_sel) {
          if (ks > 0) store_N(ks - 1);
          if (ks < KS - 1) load_N(1, nblk * NW + w, ks);
        }
        const uint32_t kg = ks * 4 + g;
        if (refill && kg < KG) load_A(ks, next_tile, kg);
      }
      fold(T, 1);
      if (next_sel) load_N(1, nblk * NW + w, KS - 1);   // T is folded: its registers carry the last k-step's tiles
      store(1, rt, nx1, obase1);
      if (next_sel) store_N(KS - 1);
    }
  }
}

// ------------------------------------------------------------------ host side

// (the twin of scan_mfma.hip's static scan_wgs_all: that file's bytes stamp the recorded PMC traffic of the scan,
// bench.py scan_source_sha16, so the helper is not moved out of it)
static uint32_t scan_pair_wgs_all() {
  static const uint32_t wgs_all = [] {
    const char* v = pirgpu_env("PIRGPU_SCAN_MFMA_WGS");
    if (v && *v) return (uint32_t)strtoul(v, nullptr, 10);
    hipDeviceProp_t prop;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 256u;
    return (uint32_t)prop.multiProcessorCount;
  }();
  return wgs_all;
}

bool scan_mfma_pair_supported(const MfmaGeom& gm) {
  return gm.L == 5 && gm.NW == 8 && gm.nchunks == 1 && gm.KS >= 1 && gm.KS <= 3;
}

template <int L, int KS, bool TOP4, bool F64F>
static void launch_scan_mfma_pair_variant(hipStream_t st, const DevParams* P, const MfmaGeom& gm, const uint8_t* dbp,
                                          const ScanGroups& grp, uint32_t rows, uint32_t wgs_req, uint32_t nslots,
                                          uint64_t out_qstride) {
  const uint32_t all = scan_pair_wgs_all();
  const uint32_t wgs = wgs_req ? std::min(wgs_req, all) : all;
  const uint32_t units = nslots / 8;
  hipLaunchKernelGGL((scan_mfma_pair_kernel<L, KS, TOP4, F64F>), dim3(std::max(1u, std::min(units, wgs))), dim3(512), 0, st,
                     P, dbp, grp, rows, gm.RT, gm.KG, nslots, out_qstride);
}

hipError_t launch_scan_mfma_pair(hipStream_t st, const DevParams* P, const MfmaGeom& gm, const uint8_t* dbp,
                                 const ScanGroups& grp, uint32_t rows, uint64_t chunk_stride, uint32_t wgs, bool f64_fold,
                                 uint32_t slot0, uint32_t nslots, uint64_t out_qstride, uint32_t out_rstride, bool blk_major) {
  (void)chunk_stride;   // one chunk: no partial sums
  if (!scan_mfma_pair_supported(gm) || grp.n != 2 || slot0 != 0 ||
      nslots == 0 || nslots % 8 || out_rstride != nslots || blk_major)
    return hipErrorInvalidValue;
  for (uint32_t g = 0; g < grp.n; ++g)
    if (!grp.sel[g] || !grp.out[g] || grp.nq[g] == 0 || grp.nq[g] > kMaxMfmaQueries) return hipErrorInvalidValue;
#define PIRGPU_PAIR_ARGS st, P, gm, dbp, grp, rows, wgs, nslots, out_qstride
#define PIRGPU_PAIR_CASE(KS_)                                                            \
  if (gm.KS == KS_) {                                                                    \
    if (gm.top4) {                                                                       \
      if (f64_fold) launch_scan_mfma_pair_variant<5, KS_, true, true>(PIRGPU_PAIR_ARGS); \
      else launch_scan_mfma_pair_variant<5, KS_, true, false>(PIRGPU_PAIR_ARGS);         \
    } else {                                                                             \
      if (f64_fold) launch_scan_mfma_pair_variant<5, KS_, false, true>(PIRGPU_PAIR_ARGS); \
      else launch_scan_mfma_pair_variant<5, KS_, false, false>(PIRGPU_PAIR_ARGS);        \
    }                                                                                    \
    return hipGetLastError();                                                            \
  }
  PIRGPU_PAIR_CASE(1) PIRGPU_PAIR_CASE(2) PIRGPU_PAIR_CASE(3)
#undef PIRGPU_PAIR_CASE
#undef PIRGPU_PAIR_ARGS
  return hipErrorInvalidValue;
}

}  // namespace pirgpu
