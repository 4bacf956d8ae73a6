// ntt_ring32k.hip -- the kernels of ring degree N = 32768 (integer flavour only).
//
// One polynomial of N = 32768 residues is 256 KiB: more than the 160 KiB of LDS a CU has, so the one-workgroup-per-
// polynomial transforms of ntt_kernels.hip cannot hold it.  Here SEAL's own radix-2 network (ntt_negacyclic_harvey /
// inverse_ntt_negacyclic_harvey, reference database.cpp:190,222,252) is cut into two launches, each of which keeps
// what it works on in LDS and registers:
//
//   pass A  the 7 stages of butterfly distance 16384 .. 256.  They never mix index bits 0..7, so they act on the 256
//           strided columns {r + 256 c : c < 128} independently: a 128-thread workgroup loads 16 adjacent columns
//           (rows of 128 contiguous bytes), transforms each with 8 threads x 16 residues, writes them back in place.
//   pass B  the 8 stages of distance 128 .. 1, on contiguous blocks of 256: a 256-thread workgroup takes 16 blocks,
//           16 threads x 16 residues per block.
//
// The inverse runs the same cut the other way round (pass B's blocks first, then the columns, N^-1 folded into the
// last stage as NttTable::iw1n does).  Within a pass a thread runs 4 (or 3) stages in registers between two LDS
// exchanges with ntt_core.h's butterflies (fwd_stages / inv_stages): the twiddle of the stage at index bit p for
// element j is tw[2^(14 - p) + (j >> (p + 1))] -- the bit-reversed tables of build_tables, unchanged.
//
// Values between the passes stay lazy (forward < 4q, inverse < 2q; Harvey butterflies): q < 2^61 keeps them in 64 bits.
// The forward output lands in SEAL's order, which IS the device order at this degree (ntt_log_ept(15) = 0,
// device_params.h): no reordering anywhere.  Integer flavour only: the transforms leave 64-bit words in HBM between the
// passes, and the fp64 flavours' gain -- fused kernels that keep a polynomial on chip from load to store -- does not
// exist when the polynomial does not fit on chip.
//
// Every NttOps entry the integer flavour calls is an elementwise kernel plus the two-pass transform; the fp64-only
// entries are nullptr (ctx.hip forces kNttInt at this degree).  The upper recursion level goes through the split form
// (upper_ntt here: re-encode + lift into scratch and the batched transform; launch_upper_mac_int: integer MAC).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_params.h"
#include "kernels.h"
#include "ntt_core.h"

namespace pirgpu {
namespace ring32k {

constexpr int LOGN = 15;
constexpr uint32_t N = 1u << LOGN;
using A = Arith<kNttInt>;

// pass A: 256 columns of 128 rows; 16 columns per workgroup, 8 threads x 16 residues per column
constexpr int kColLog = 7;
constexpr uint32_t kRows = 1u << kColLog, kCols = N >> kColLog;
constexpr uint32_t kColsPerWg = 16, kColThreads = kRows / 16, kColWg = kColsPerWg * kColThreads;   // 128 threads
constexpr uint32_t kColWords = kRows + kRows / 16;      // one column in LDS, padded (lds_idx<4>)
// pass B: 128 blocks of 256; 16 blocks per workgroup, 16 threads x 16 residues per block
constexpr int kBlkLog = 8;
constexpr uint32_t kBlk = 1u << kBlkLog, kBlocks = N >> kBlkLog;
constexpr uint32_t kBlksPerWg = 16, kBlkThreads = kBlk / 16, kBlkWg = kBlksPerWg * kBlkThreads;    // 256 threads
constexpr uint32_t kBlkWords = kBlk + kBlk / 16;
static_assert(kCols % kColsPerWg == 0 && kBlocks % kBlksPerWg == 0, "whole workgroups per polynomial");

// Which polynomials a transform launch covers: polynomial p (p < grid / workgroups per polynomial) is read from
// src + p N (the first pass only) and transformed into dst_poly(p) -- dst + p N, or with B != 0 the selector buffer of
// query (p / k2) % B (ct_ntt_fwd_split's layout).  Modulus index: mod_base + (p / mod_div) % mod_period.
struct PolyMap {
  const uint64_t* src;
  uint64_t* dst;
  MfmaPtrs split;
  uint32_t B, k2;
  uint32_t mod_div, mod_period, mod_base;
};

__device__ __forceinline__ uint64_t* dst_poly(const PolyMap& mp, uint32_t p) {
  if (mp.B == 0) return mp.dst + (size_t)p * N;
  const uint32_t ct = p / mp.k2, rem = p % mp.k2;
  return (uint64_t*)mp.split.p[ct % mp.B] + ((size_t)(ct / mp.B) * mp.k2 + rem) * N;
}
__device__ __forceinline__ int mod_of(const PolyMap& mp, uint32_t p) {
  return (int)(mp.mod_base + (p / mp.mod_div) % mp.mod_period);
}

// The 15 twiddles of a register pass in fwd_stages / inv_stages order: for the sub-transform of size 2^LS whose element
// l is global index j = (base_hi << LS) | l of the same stages, relative bit rb of the pass with window LB is index bit
// p = LB + rb, and the twiddle is tab[(base << (LS - 1 - p)) + (l >> (p + 1))] with l >> (p + 1) = (outer << (3 - rb)) + g.
// base = 1 for the columns of pass A, 128 + block for pass B.
template <int LS, int LB, int RHI, int RLO>
__device__ __forceinline__ void load_tw(Twiddle (&W)[15], A::TWPtr tab, uint32_t base, uint32_t outer) {
#pragma unroll
  for (int rb = RHI; rb >= RLO; --rb) {
#pragma unroll
    for (int g = 0; g < (8 >> rb); ++g)
      W[(8 >> rb) - 1 + g] = A::load_tw(tab, (base << (LS - 1 - LB - rb)) + (outer << (3 - rb)) + (uint32_t)g);
  }
}

// ---- pass A: columns.  Column element c (row) is global index r + 256 c; a column's 8 threads are adjacent lanes.

// HBM <-> LDS: thread t moves rows c = (t >> 4) + 8 e of column t & 15 -- 16 lanes cover one 128-byte row segment.
__device__ __forceinline__ void cols_load(uint64_t* s, const uint64_t* base, uint32_t tid) {
  const uint32_t u = tid & 15, c0 = tid >> 4;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const uint32_t c = c0 + 8 * e;
    s[u * kColWords + lds_idx<4>(c)] = base[(size_t)c * kCols + u];
  }
}
__device__ __forceinline__ void cols_store(const uint64_t* s, uint64_t* base, uint32_t tid) {
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const uint32_t u = tid & 15, c = (tid >> 4) + 8 * e;
    base[(size_t)c * kCols + u] = s[u * kColWords + lds_idx<4>(c)];
  }
}

// grid = polynomials * 16: the first 7 stages of the forward transform, src -> dst_poly.
__global__ void __launch_bounds__(kColWg) ntt32k_fwd_cols_kernel(const DevParams* __restrict__ P, PolyMap mp) {
  __shared__ uint64_t s[kColsPerWg * kColWords];
  const uint32_t tid = threadIdx.x;
  const uint32_t p = blockIdx.x / (kCols / kColsPerWg), r0 = (blockIdx.x % (kCols / kColsPerWg)) * kColsPerWg;
  const int mi = mod_of(mp, p);
  const A::Mod m = A::mod(P, mi);
  const A::TWPtr tw = A::tw(P, mi);
  cols_load(s, mp.src + (size_t)p * N + r0, tid);
  __syncthreads();
  uint64_t* sc = s + (tid / kColThreads) * kColWords;
  const uint32_t tg = tid % kColThreads;
  uint64_t x[16];
  Twiddle W[15];
  // rows (e << 3) | tg: stages of distance 16384 .. 2048 (row bits 6..3)
#pragma unroll
  for (int e = 0; e < 16; ++e) x[e] = sc[lds_idx<4>((uint32_t)(e << 3) | tg)];
  load_tw<kColLog, 3, 3, 0>(W, tw, 1, 0);
  fwd_stages<A, 4, 3, 0>(x, W, m);
#pragma unroll
  for (int e = 0; e < 16; ++e) sc[lds_idx<4>((uint32_t)(e << 3) | tg)] = x[e];   // the words this thread read
  __syncthreads();
  // rows (tg << 4) | e: distance 1024 .. 256 (row bits 2..0)
#pragma unroll
  for (int e = 0; e < 16; ++e) x[e] = sc[lds_idx<4>((tg << 4) | (uint32_t)e)];
  load_tw<kColLog, 0, 2, 0>(W, tw, 1, tg);
  fwd_stages<A, 4, 2, 0>(x, W, m);
#pragma unroll
  for (int e = 0; e < 16; ++e) sc[lds_idx<4>((tg << 4) | (uint32_t)e)] = x[e];
  __syncthreads();
  cols_store(s, dst_poly(mp, p) + r0, tid);
}

// grid = polynomials * 16: the last 7 stages of the inverse transform (distance 256 .. 16384, N^-1 folded into the
// last), in place on dst_poly; canonical output.
__global__ void __launch_bounds__(kColWg) ntt32k_inv_cols_kernel(const DevParams* __restrict__ P, PolyMap mp) {
  __shared__ uint64_t s[kColsPerWg * kColWords];
  const uint32_t tid = threadIdx.x;
  const uint32_t p = blockIdx.x / (kCols / kColsPerWg), r0 = (blockIdx.x % (kCols / kColsPerWg)) * kColsPerWg;
  const int mi = mod_of(mp, p);
  const A::Mod m = A::mod(P, mi);
  const A::TWPtr itw = A::itw(P, mi);
  const Twiddle ninv = A::ninv(P, mi), iw1n = A::iw1n(P, mi);
  uint64_t* base = dst_poly(mp, p) + r0;
  cols_load(s, base, tid);
  __syncthreads();
  uint64_t* sc = s + (tid / kColThreads) * kColWords;
  const uint32_t tg = tid % kColThreads;
  uint64_t x[16];
  Twiddle W[15];
  // rows (tg << 4) | e: row bits 0..3
#pragma unroll
  for (int e = 0; e < 16; ++e) x[e] = sc[lds_idx<4>((tg << 4) | (uint32_t)e)];
  load_tw<kColLog, 0, 3, 0>(W, itw, 1, tg);
  inv_stages<A, 4, 0, false>(x, W, ninv, iw1n, m);
#pragma unroll
  for (int e = 0; e < 16; ++e) sc[lds_idx<4>((tg << 4) | (uint32_t)e)] = x[e];
  __syncthreads();
  // rows (e << 3) | tg: row bits 4..6, the last one the N^-1 stage
#pragma unroll
  for (int e = 0; e < 16; ++e) x[e] = sc[lds_idx<4>((uint32_t)(e << 3) | tg)];
  load_tw<kColLog, 3, 2, 1>(W, itw, 1, 0);
  inv_stages<A, 4, 1, true>(x, W, ninv, iw1n, m);
#pragma unroll
  for (int e = 0; e < 16; ++e) sc[lds_idx<4>((uint32_t)(e << 3) | tg)] = A::canon_inv(x[e], m);
  __syncthreads();
  cols_store(s, base, tid);
}

// ---- pass B: blocks of 256 contiguous residues.  Thread tg of a block holds l = (e << 4) | tg in the pass of window 4
// (HBM-coalesced: 16 lanes read 128 contiguous bytes) and l = (tg << 4) | e in the pass of window 0.

// grid = polynomials * 8: the last 8 stages of the forward transform, in place on dst_poly; canonical output.
__global__ void __launch_bounds__(kBlkWg) ntt32k_fwd_rows_kernel(const DevParams* __restrict__ P, PolyMap mp) {
  __shared__ uint64_t s[kBlksPerWg * kBlkWords];
  const uint32_t tid = threadIdx.x;
  const uint32_t p = blockIdx.x / (kBlocks / kBlksPerWg);
  const uint32_t b = (blockIdx.x % (kBlocks / kBlksPerWg)) * kBlksPerWg + tid / kBlkThreads, tg = tid % kBlkThreads;
  const int mi = mod_of(mp, p);
  const A::Mod m = A::mod(P, mi);
  const A::TWPtr tw = A::tw(P, mi);
  uint64_t* blk = dst_poly(mp, p) + (size_t)b * kBlk;
  uint64_t* sb = s + (tid / kBlkThreads) * kBlkWords;
  uint64_t x[16];
  Twiddle W[15];
#pragma unroll
  for (int e = 0; e < 16; ++e) x[e] = blk[(e << 4) | tg];
  load_tw<kBlkLog, 4, 3, 0>(W, tw, 128 + b, 0);
  fwd_stages<A, 4, 3, 0>(x, W, m);
#pragma unroll
  for (int e = 0; e < 16; ++e) sb[lds_idx<4>((uint32_t)(e << 4) | tg)] = x[e];
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 16; ++e) x[e] = sb[lds_idx<4>((tg << 4) | (uint32_t)e)];
  load_tw<kBlkLog, 0, 3, 0>(W, tw, 128 + b, tg);
  fwd_stages<A, 4, 3, 0>(x, W, m);
#pragma unroll
  for (int e = 0; e < 16; ++e) sb[lds_idx<4>((tg << 4) | (uint32_t)e)] = A::canon_fwd(x[e], m);
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 16; ++e) blk[(e << 4) | tg] = sb[lds_idx<4>((uint32_t)(e << 4) | tg)];
}

// grid = polynomials * 8: the first 8 stages of the inverse transform, src -> dst_poly (src may be dst).
__global__ void __launch_bounds__(kBlkWg) ntt32k_inv_rows_kernel(const DevParams* __restrict__ P, PolyMap mp) {
  __shared__ uint64_t s[kBlksPerWg * kBlkWords];
  const uint32_t tid = threadIdx.x;
  const uint32_t p = blockIdx.x / (kBlocks / kBlksPerWg);
  const uint32_t b = (blockIdx.x % (kBlocks / kBlksPerWg)) * kBlksPerWg + tid / kBlkThreads, tg = tid % kBlkThreads;
  const int mi = mod_of(mp, p);
  const A::Mod m = A::mod(P, mi);
  const A::TWPtr itw = A::itw(P, mi);
  const Twiddle ninv = A::ninv(P, mi), iw1n = A::iw1n(P, mi);
  const uint64_t* in = mp.src + (size_t)p * N + (size_t)b * kBlk;
  uint64_t* sb = s + (tid / kBlkThreads) * kBlkWords;
  uint64_t x[16];
  Twiddle W[15];
#pragma unroll
  for (int e = 0; e < 16; ++e) sb[lds_idx<4>((uint32_t)(e << 4) | tg)] = in[(e << 4) | tg];
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 16; ++e) x[e] = sb[lds_idx<4>((tg << 4) | (uint32_t)e)];
  load_tw<kBlkLog, 0, 3, 0>(W, itw, 128 + b, tg);
  inv_stages<A, 4, 0, false>(x, W, ninv, iw1n, m);
#pragma unroll
  for (int e = 0; e < 16; ++e) sb[lds_idx<4>((tg << 4) | (uint32_t)e)] = x[e];
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 16; ++e) x[e] = sb[lds_idx<4>((uint32_t)(e << 4) | tg)];
  load_tw<kBlkLog, 4, 3, 0>(W, itw, 128 + b, 0);
  inv_stages<A, 4, 0, false>(x, W, ninv, iw1n, m);
  uint64_t* blk = dst_poly(mp, p) + (size_t)b * kBlk;
#pragma unroll
  for (int e = 0; e < 16; ++e) blk[(e << 4) | tg] = x[e];
}

// The whole transform of n_polys polynomials: two launches.
static hipError_t transform(hipStream_t st, const DevParams* P, const PolyMap& mp, uint64_t n_polys, bool inverse) {
  if (!n_polys) return hipSuccess;
  if (n_polys > (1ull << 26)) return hipErrorInvalidValue;   // grid.x < 2^31
  const dim3 ga((uint32_t)n_polys * (kCols / kColsPerWg)), gb((uint32_t)n_polys * (kBlocks / kBlksPerWg));
  if (inverse) {
    hipLaunchKernelGGL(ntt32k_inv_rows_kernel, gb, dim3(kBlkWg), 0, st, P, mp);
    hipLaunchKernelGGL(ntt32k_inv_cols_kernel, ga, dim3(kColWg), 0, st, P, mp);
  } else {
    hipLaunchKernelGGL(ntt32k_fwd_cols_kernel, ga, dim3(kColWg), 0, st, P, mp);
    hipLaunchKernelGGL(ntt32k_fwd_rows_kernel, gb, dim3(kBlkWg), 0, st, P, mp);
  }
  return hipGetLastError();
}

static PolyMap contiguous(const uint64_t* src, uint64_t* dst, uint32_t mod_div, uint32_t mod_period, uint32_t mod_base) {
  PolyMap mp{};
  mp.src = src;
  mp.dst = dst;
  mp.mod_div = mod_div;
  mp.mod_period = mod_period;
  mp.mod_base = mod_base;
  return mp;
}

// ---- elementwise kernels: one thread per coefficient, 1-D grids (gid = polynomial * N + coefficient)

constexpr uint32_t kEw = 256;
static dim3 ew_grid(uint64_t polys) { return dim3((uint32_t)(polys * (N / kEw))); }

// ks_digit, part 1: dig[node][I][J] = sigma_g(c1)_J mod m_I in coefficient form (SEAL GaloisTool::apply_galois: source
// coefficient i goes to i g mod N, negated when i g mod 2N >= N); the batched forward transform follows.
__global__ void __launch_bounds__(kEw) galois_digits_kernel(const DevParams* __restrict__ P, const uint64_t* __restrict__ res_in,
                                                            uint32_t galois_elt, uint64_t* __restrict__ dig) {
  const uint64_t gid = (uint64_t)blockIdx.x * kEw + threadIdx.x;
  const uint32_t k = P->k, km = k + 1, i = (uint32_t)(gid & (N - 1));
  const uint64_t src_poly = gid >> LOGN;   // node * k + J
  const uint32_t J = (uint32_t)(src_poly % k);
  const uint64_t node = src_poly / k;
  uint64_t v = res_in[((node * 2 + 1) * k + J) * N + i];
  const uint32_t raw = (uint32_t)(((uint64_t)i * galois_elt) & (2 * N - 1));
  if (raw >= N) v = neg_mod(v, P->mod[J].q);
  const uint32_t to = raw & (N - 1);
  for (uint32_t I = 0; I < km; ++I) dig[((node * km + I) * k + J) * N + to] = reduce64(v, P->mod[I]);
}

// ks_mac_intt, part 1: prod[node][comp][I] = sum_J dig[node][I][J] (.) key[J][comp][I] (NTT form); the batched inverse
// transform follows.  k <= 8 products of two residues < 2^61 fit 128 bits.
__global__ void __launch_bounds__(kEw) ks_mac_kernel(const DevParams* __restrict__ P, const uint64_t* __restrict__ dig,
                                                     KeyPtrs keys, uint64_t* __restrict__ prod) {
  const uint64_t gid = (uint64_t)blockIdx.x * kEw + threadIdx.x;
  const uint32_t k = P->k, km = k + 1, i = (uint32_t)(gid & (N - 1));
  const uint64_t opoly = gid >> LOGN;      // (node * 2 + comp) * km + I
  const uint32_t I = (uint32_t)(opoly % km), comp = (uint32_t)((opoly / km) & 1);
  const uint64_t node = opoly / km / 2;
  const uint64_t* key = keys.p[node % keys.B];
  const uint64_t* d = dig + (node * km + I) * k * N + i;
  u128 acc = 0;
  for (uint32_t J = 0; J < k; ++J) acc += (u128)d[(size_t)J * N] * key[(((size_t)J * 2 + comp) * km + I) * N + i];
  prod[opoly * N + i] = reduce128((uint64_t)acc, (uint64_t)(acc >> 64), P->mod[I]);
}

// db_encode, part 1: bits-wide coefficients packed MSB-first from the item bytes (reference string_encoder.cpp:58-122)
// or pre-encoded ones, then the plain lift (Evaluator::transform_to_ntt_inplace(Plaintext)) into
// db[pt][j]; the batched forward transform follows.  Wide items: one launch per plane, which packs the bytes
// [src_off, src_off + src_len) of every source row (an item of bytes_per_pt bytes); otherwise 0, bytes_per_pt.
__global__ void __launch_bounds__(kEw) db_lift_kernel(const DevParams* __restrict__ P, const uint64_t* __restrict__ coeffs,
                                                      const uint8_t* __restrict__ bytes, uint64_t bytes_per_pt,
                                                      uint64_t total_bytes, uint32_t bits, uint64_t* __restrict__ db,
                                                      uint64_t src_off, uint64_t src_len) {
  const uint64_t gid = (uint64_t)blockIdx.x * kEw + threadIdx.x;
  const uint32_t k = P->k, c = (uint32_t)(gid & (N - 1));
  const uint64_t poly = gid >> LOGN, pt = poly / k;
  const uint32_t j = (uint32_t)(poly % k);
  const ModConst mc = P->mod[j];
  uint64_t v = 0;
  if (coeffs) {
    v = coeffs[pt * N + c];
  } else {
    const uint64_t start = pt * bytes_per_pt + src_off;
    const uint64_t L = start >= total_bytes ? 0 : (total_bytes - start < src_len ? total_bytes - start : src_len);
    const uint8_t* src = bytes + start;
    uint64_t bitpos = (uint64_t)c * bits, byte = bitpos >> 3;
    uint32_t off = (uint32_t)(bitpos & 7);
    int need = (int)bits;
    while (need > 0) {
      const uint32_t B = byte < L ? src[byte] : 0u;
      const int avail = 8 - (int)off, take = avail < need ? avail : need;
      v = (v << take) | ((B >> (avail - take)) & ((1u << take) - 1u));
      need -= take;
      off = 0;
      ++byte;
    }
  }
  const uint64_t inc = P->lift_inc[j] >= mc.q ? P->lift_inc[j] - mc.q : P->lift_inc[j];
  uint64_t r = reduce64(v, mc);
  if (v >= P->plain_thr) r = add_mod(r, inc, mc.q);
  db[gid] = r;
}

// split upper level, part 1a (the integer form of ntt_kernels.hip upper_ntt_kernel): Encode chunk e_idx of child
// b0 + iib of row r (CiphertextReencoder::Encode, reference ct_reencoder.cpp:49-69), lifted mod q_jt, into
// scratch[query][row][cc][child in block][chunk][jt][N]; zero beyond the database.  The batched forward transform follows.
__global__ void __launch_bounds__(kEw) upper_lift_kernel(const DevParams* __restrict__ P, const uint64_t* __restrict__ src_all,
                                                         uint64_t* __restrict__ scratch, uint32_t n_rows, uint32_t n_dim,
                                                         uint32_t n_children_total, uint32_t C, uint32_t b0, uint32_t blk,
                                                         uint64_t src_qstride) {
  const uint64_t gid = (uint64_t)blockIdx.x * kEw + threadIdx.x;
  const uint32_t k = P->k, E = P->enc_count, i = (uint32_t)(gid & (N - 1));
  uint64_t poly = gid >> LOGN;
  const uint32_t jt = (uint32_t)(poly % k);
  poly /= k;
  const uint32_t e_idx = (uint32_t)(poly % E);
  poly /= E;
  const uint32_t iib = (uint32_t)(poly % blk);
  poly /= blk;
  const uint32_t cc = (uint32_t)(poly % C);
  poly /= C;
  const uint32_t r = (uint32_t)(poly % n_rows);
  const uint32_t qi = (uint32_t)(poly / n_rows);
  const uint32_t ii = b0 + iib, child0 = r * n_dim;
  uint32_t nchild = n_children_total > child0 ? n_children_total - child0 : 0;
  if (nchild > n_dim) nchild = n_dim;
  uint64_t out = 0;
  if (ii < nchild) {
    const uint32_t sp = P->enc_poly[e_idx], sj = P->enc_res[e_idx], sh = P->enc_shift[e_idx];
    const uint64_t mask = (1ull << P->enc_bits) - 1;
    const ModConst mc = P->mod[jt];
    const uint64_t inc = P->lift_inc[jt] >= mc.q ? P->lift_inc[jt] - mc.q : P->lift_inc[jt];
    const uint64_t* in = src_all + (size_t)qi * src_qstride + ((((size_t)(child0 + ii) * C + cc) * 2 + sp) * k + sj) * N;
    const uint64_t v = (in[i] >> sh) & mask;
    out = reduce64(v, mc);
    if (v >= P->plain_thr) out = add_mod(out, inc, mc.q);
  }
  scratch[gid] = out;
}

// split upper level, part 2 (integer form of kernels.hip upper_mac_kernel): acc[query][slot][comp][jt][i] (+)= sum over
// the block's children of scratch (.) selector, as canonical residues; `last` writes to `out` instead of `acc`.
__global__ void __launch_bounds__(kEw) upper_mac_int_kernel(const DevParams* __restrict__ P, const uint64_t* __restrict__ scratch,
                                                            MfmaPtrs svq, uint64_t* __restrict__ acc_all,
                                                            uint64_t* __restrict__ out_all, uint32_t n_rows, uint32_t C,
                                                            uint32_t sv_first, uint32_t b0, uint32_t blk, uint32_t n_dim,
                                                            int first, int last, uint64_t acc_qstride, uint64_t out_qstride) {
  const uint64_t gid = (uint64_t)blockIdx.x * kEw + threadIdx.x;
  const uint32_t k = P->k, E = P->enc_count, i = (uint32_t)(gid & (N - 1));
  uint64_t poly = gid >> LOGN;            // ((query * n_rows + r) * C + cc) * E + e_idx) * k + jt
  const uint32_t jt = (uint32_t)(poly % k);
  poly /= k;
  const uint32_t e_idx = (uint32_t)(poly % E);
  poly /= E;
  const uint32_t cc = (uint32_t)(poly % C);
  poly /= C;
  const uint32_t r = (uint32_t)(poly % n_rows);
  const uint32_t qi = (uint32_t)(poly / n_rows);
  const ModConst mc = P->mod[jt];
  const uint64_t* sv = reinterpret_cast<const uint64_t*>(svq.p[qi]);
  const size_t child_stride = (size_t)E * k * N;
  const uint64_t* x = scratch + ((((size_t)qi * n_rows + r) * C + cc) * blk * E + e_idx) * k * N + (size_t)jt * N + i;
  const uint32_t n_here = b0 < n_dim ? (n_dim - b0 < blk ? n_dim - b0 : blk) : 0;
  u128 a0 = 0, a1 = 0;
  uint32_t since = 0;
  for (uint32_t iib = 0; iib < n_here; ++iib) {
    const uint64_t* s0 = sv + (((size_t)(sv_first + b0 + iib) * 2 + 0) * k + jt) * N + i;
    const uint64_t v = x[(size_t)iib * child_stride];
    a0 += (u128)v * s0[0];
    a1 += (u128)v * s0[(size_t)k * N];
    if (++since == P->lazy_limit) {
      since = 0;
      a0 = reduce128((uint64_t)a0, (uint64_t)(a0 >> 64), mc);
      a1 = reduce128((uint64_t)a1, (uint64_t)(a1 >> 64), mc);
    }
  }
  uint64_t s0 = reduce128((uint64_t)a0, (uint64_t)(a0 >> 64), mc), s1 = reduce128((uint64_t)a1, (uint64_t)(a1 >> 64), mc);
  uint64_t* acc = acc_all + (size_t)qi * acc_qstride;
  uint64_t* out = out_all + (size_t)qi * out_qstride;
  const size_t slot = ((size_t)r * C + cc) * E + e_idx;
  const size_t o0 = ((slot * 2 + 0) * k + jt) * N + i, o1 = ((slot * 2 + 1) * k + jt) * N + i;
  if (!first) {
    s0 = add_mod(s0, acc[o0], mc.q);
    s1 = add_mod(s1, acc[o1], mc.q);
  }
  uint64_t* dst = last ? out : acc;
  dst[o0] = s0;
  dst[o1] = s1;
}

// ------------------------------------------------------------------ NttOps

static hipError_t op_configure(int mode) { return mode == kNttInt ? hipSuccess : hipErrorInvalidValue; }

static hipError_t op_ntt_batch(hipStream_t st, int mode, const DevParams* P, uint64_t* data, uint64_t n_polys,
                               uint32_t mod_period, uint32_t mod_base, bool inverse) {
  if (mode != kNttInt) return hipErrorInvalidValue;
  return transform(st, P, contiguous(data, data, 1, mod_period, mod_base), n_polys, inverse);
}

static hipError_t op_ct_ntt_fwd_oop(hipStream_t st, int mode, const DevParams* P, uint32_t k, const uint64_t* src,
                                    uint64_t* dst, uint64_t n_cts, bool) {
  if (mode != kNttInt) return hipErrorInvalidValue;   // (the integer tree holds u64 residues: src_is_tree changes nothing)
  return transform(st, P, contiguous(src, dst, 1, k, 0), n_cts * 2 * k, false);
}

static hipError_t op_ct_ntt_fwd_split(hipStream_t st, int mode, const DevParams* P, uint32_t k, const uint64_t* src,
                                      const MfmaPtrs& dst, uint32_t B, uint64_t n_cts_total) {
  if (mode != kNttInt || B == 0 || B > (uint32_t)kMaxMfmaQueries) return hipErrorInvalidValue;
  PolyMap mp = contiguous(src, nullptr, 1, k, 0);
  mp.split = dst;
  mp.B = B;
  mp.k2 = 2 * k;
  return transform(st, P, mp, n_cts_total * 2 * k, false);
}

static hipError_t op_db_encode(hipStream_t st, int mode, const DevParams* P, uint32_t k, const uint64_t* coeffs,
                               const uint8_t* bytes, uint64_t bytes_per_pt, uint64_t total_bytes, uint32_t bits,
                               uint64_t n_pt, uint64_t* db, uint32_t planes, uint64_t plane_bytes,
                               uint64_t plane_stride) {
  if (mode != kNttInt) return hipErrorInvalidValue;
  if (planes < 1 || (planes > 1 && (coeffs || !plane_bytes || (uint64_t)(planes - 1) * plane_bytes >= bytes_per_pt)))
    return hipErrorInvalidValue;
  if (!n_pt) return hipSuccess;
  for (uint32_t pl = 0; pl < planes; ++pl) {   // plane pl of every item -> plaintexts pl * plane_stride + [0, n_pt)
    uint64_t* dst = db + (size_t)pl * plane_stride * k * N;
    const uint64_t off = planes > 1 ? pl * plane_bytes : 0;
    const uint64_t len = planes > 1 && bytes_per_pt - off > plane_bytes ? plane_bytes : bytes_per_pt - off;
    hipLaunchKernelGGL(db_lift_kernel, ew_grid(n_pt * k), dim3(kEw), 0, st, P, coeffs, bytes, bytes_per_pt, total_bytes,
                       bits, dst, off, len);
    if (hipError_t e = hipGetLastError()) return e;
    if (hipError_t e = transform(st, P, contiguous(dst, dst, 1, k, 0), n_pt * k, false)) return e;
  }
  return hipSuccess;
}

// u64 digits only: no packed intermediates (ctx.hip turns pack40 off at this degree), no 5-byte tree, no c0 products
static hipError_t op_ks_digit(hipStream_t st, int mode, const DevParams* P, uint32_t k, const uint64_t* res_in,
                              uint32_t galois_elt, uint32_t nodes, uint64_t* dig, bool pack40, uint64_t* c0_out,
                              bool tree40, bool) {
  if (mode != kNttInt || pack40 || c0_out || tree40) return hipErrorInvalidValue;
  if (!nodes) return hipSuccess;
  hipLaunchKernelGGL(galois_digits_kernel, ew_grid((uint64_t)nodes * k), dim3(kEw), 0, st, P, res_in, galois_elt, dig);
  if (hipError_t e = hipGetLastError()) return e;
  // dig[node][I][J]: modulus I = (p / k) % (k + 1)
  return transform(st, P, contiguous(dig, dig, k, k + 1, 0), (uint64_t)nodes * (k + 1) * k, false);
}

// all k + 1 key-level moduli at once (the integer flavour never asks for a subset)
static hipError_t op_ks_mac_intt(hipStream_t st, int mode, const DevParams* P, uint32_t k, const uint64_t* dig,
                                 const KeyPtrs& key, uint32_t nodes, uint64_t* prod, bool pack40, uint32_t I_base,
                                 uint32_t I_count) {
  if (mode != kNttInt || pack40 || I_base != 0 || I_count != k + 1 || key.B == 0) return hipErrorInvalidValue;
  if (!nodes) return hipSuccess;
  const uint64_t polys = (uint64_t)nodes * 2 * (k + 1);
  hipLaunchKernelGGL(ks_mac_kernel, ew_grid(polys), dim3(kEw), 0, st, P, dig, key, prod);
  if (hipError_t e = hipGetLastError()) return e;
  return transform(st, P, contiguous(prod, prod, 1, k + 1, 0), polys, true);
}

static hipError_t op_upper_ntt(hipStream_t st, int mode, const DevParams* P, uint32_t k, uint32_t enc_count,
                               const uint64_t* src, uint64_t* scratch, uint32_t n_rows, uint32_t n_dim,
                               uint32_t n_children_total, uint32_t C, uint32_t b0, uint32_t blk, uint32_t n_queries,
                               uint64_t src_qstride, bool) {
  if (mode != kNttInt) return hipErrorInvalidValue;
  const uint64_t polys = (uint64_t)n_queries * n_rows * C * blk * enc_count * k;
  if (!polys) return hipSuccess;
  hipLaunchKernelGGL(upper_lift_kernel, ew_grid(polys), dim3(kEw), 0, st, P, src, scratch, n_rows, n_dim,
                     n_children_total, C, b0, blk, src_qstride);
  if (hipError_t e = hipGetLastError()) return e;
  return transform(st, P, contiguous(scratch, scratch, 1, k, 0), polys, false);
}

// slot-sharded step: the separate assembly pass, then the in-place inverse transform
static hipError_t op_ntt_inv_gather(hipStream_t st, int mode, const DevParams* P, uint32_t k, const uint64_t* src,
                                    uint64_t* dst, const SliceMap& map, uint32_t RC, uint32_t nq, uint32_t nq_total,
                                    uint32_t q0) {
  if (mode != kNttInt) return hipErrorInvalidValue;
  const uint32_t kN = k * N;
  if (hipError_t e = launch_slots_assemble(st, src, dst, map, RC, kN, nq, (uint64_t)RC * kN, nq_total, q0)) return e;
  return transform(st, P, contiguous(dst, dst, 1, k, 0), (uint64_t)nq * RC * k, true);
}

}  // namespace ring32k

hipError_t launch_upper_mac_int(hipStream_t st, const DevParams* P, const uint64_t* scratch, const MfmaPtrs& svq,
                                uint64_t* acc, uint64_t* out, uint32_t n_queries, uint32_t n_rows, uint32_t C,
                                uint32_t enc_count, uint32_t k, uint32_t N, uint32_t sv_first, uint32_t b0, uint32_t blk,
                                uint32_t n_dim, bool first, bool last, uint64_t acc_qstride, uint64_t out_qstride) {
  using namespace ring32k;
  if (N != ring32k::N) return hipErrorInvalidValue;
  const uint64_t polys = (uint64_t)n_queries * n_rows * C * enc_count * k;
  if (!polys) return hipSuccess;
  hipLaunchKernelGGL(upper_mac_int_kernel, ew_grid(polys), dim3(kEw), 0, st, P, scratch, svq, acc, out, n_rows, C,
                     sv_first, b0, blk, n_dim, first ? 1 : 0, last ? 1 : 0, acc_qstride, out_qstride);
  return hipGetLastError();
}

// host-only accessor; the fp64-only entries are nullptr (ctx.hip never selects an fp64 flavour at N = 32768)
const NttOps* ntt_ops_15() {
  using namespace ring32k;
  static const NttOps ops = {op_configure, op_ntt_batch, op_ct_ntt_fwd_oop, op_ct_ntt_fwd_split, op_db_encode,
                             op_ks_digit,  op_ks_mac_intt, /*upper_fused*/ nullptr, /*ks_last_level*/ nullptr,
                             op_upper_ntt, /*ks_mac_combine*/ nullptr, /*ks_last_ntt*/ nullptr, op_ntt_inv_gather,
                             /*tree_c0_fwd*/ nullptr};
  return &ops;
}

}  // namespace pirgpu
