// scan_mfma.hip -- digit-sliced database scan on the int8 matrix cores (gfx950).
//
// Base case of PIRDatabase::multiply (reference database.cpp:185-194,238-247) for d >= 2: for every
// residue slot j (kN of them) and every database row r
//     out[query][r][comp][j] = sum_c  DB[r][c][j] * S[query][c][comp][j]   (mod q_j)
// i.e. per slot j an exact integer matrix product [rows x cols] * [cols x (2 * queries)].  The plain
// 64-bit multiply-accumulate kernels (kernels.hip) are HBM-bound for one query but VALU-bound as soon
// as several queries share a database pass (each 36x36-bit product costs four v_mad_u64_u32).  Here
// both operands are stored as balanced base-256 digits (signed bytes, L per residue) and the L*L
// digit products run on v_mfma_i32_16x16x64_i8:
//     A tile = 16 rows x 64 columns of digit a of the database      (one 16-byte load per lane)
//     B tile = 64 columns x 16 (query, comp) pairs of digit b of the selectors
//     T[a+b] += A_a * B_b      (the K accumulation and the digit diagonal share one int32 accumulator)
// then value = sum_s T[s] 2^(8 s) is folded and reduced modulo q_j exactly.  All arithmetic is integer
// and exact (|T| <= (L - 1) * 2^14 * 64 * KS < 2^25.2, see kBiasBits), so replies stay bit-identical to the reference.  The
// database is stored ONCE in the operand layout of the instruction, which also shrinks it from
// 8 to L bytes per residue (5 for the 36-bit moduli of N = 4096): the pass reads 0.74x the bytes of
// the u64 layout (incl. padding to 16 x 16 tiles) and serves up to 8 queries.
//
// Layouts (bytes):
//   database   [j][chunk][rt = r / 16][kg within the chunk][a][r % 16][c % 16]   (kg = c / 16; a chunk = the 4 * KS
//              column groups one launch row keeps selectors for; one chunk -> [j][rt][kg][a][..] as before)
//   selectors  [j][kg][b][x = 2 * query + comp][c % 16]
//   TOP4 (moduli below 2^(8 (L-1) + 4): 36 bits at L = 5, 44 at L = 6): the top digit's 16 x 16 tile is 128 bytes of
//   nibbles instead of 256 bytes (pack_top4 / expand_top4 below) -- L - 1/2 bytes per residue in both operands.
// A workgroup is 8 waves = 8 consecutive slots j (one per wave); results are staged through LDS so
// that each (row, x) is written as one 64-byte run of 8 slots.
#include <hip/hip_runtime.h>

#include <stdlib.h>

#include <algorithm>

#include "arith.h"
#include "kernels.h"

namespace pirgpu {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef unsigned __int128 u128;

#ifndef PIRGPU_SCAN_DIRECT
#define PIRGPU_SCAN_DIRECT 0
#endif
#ifndef PIRGPU_SCAN_PAD
#define PIRGPU_SCAN_PAD 1     // pad words per (row, x) run of the result staging: 1 = two 8-byte LDS reads per thread, 2 = one 16-byte read
#endif

// Byte offset of tile (slot j, row tile rt, column group kg, digit a) in the packed database.  Column chunks are
// the outer dimension inside a slot, so the part of a slot's slab one workgroup row streams is contiguous
// (a matrix wider than one chunk used to be read as 14-18 KB pieces with gaps: 3.8-4.2 TB/s instead of ~5.8).
// TB = bytes of the L digit tiles of one (row tile, column group): L * 256, or (L - 1) * 256 + 128 when the top digit is
// stored as nibbles (tile_bytes below); digit a starts a * 256 bytes into the block.
__host__ __device__ __forceinline__ size_t db_tile_offset(uint32_t j, uint32_t rt, uint32_t kg, uint32_t a, uint32_t TB,
                                                          uint32_t RT, uint32_t KG, uint32_t GC) {
  const uint32_t ch = kg / GC, kg0 = ch * GC;
  const uint32_t gc = KG - kg0 < GC ? KG - kg0 : GC;   // groups of this chunk
  return ((size_t)j * RT * KG + (size_t)RT * kg0 + (size_t)rt * gc + (kg - kg0)) * TB + (size_t)a * 256;
}

// Top digit as a NIBBLE (TOP4).  A residue below 2^(8 (L-1) + 4) -- 36 bits at L = 5, 44 at L = 6, 52 at L = 7: every
// BASELINE chain -- needs only 4 bits of its top digit if it is centred asymmetrically: v = x for x <= vmax, else x - q,
// with vmax = 7 * 256^(L-1) + 127 (256^(L-1) - 1) / 255 the largest value whose balanced low digits leave a top digit of
// 7; x - q then never goes below the value whose top digit is -8 (the two ranges together span exactly 2^(8 (L-1) + 4)).
// The top digit tile of 16 x 16 entries is stored in 128 bytes, 8 per row: byte i of the first word holds columns i
// (low nibble) and i + 4, byte i of the second word columns 8 + i and 12 + i, so that a row unpacks to its 16 signed
// bytes with shifts and masks only (expand_top4).  Database and packed selectors shrink from L to L - 1/2 bytes per
// residue: 10 % fewer bytes to stream per pass -- and to send to every GPU of a row-sharded job -- at L = 5.
template <int L>
__host__ __device__ __forceinline__ constexpr int64_t top4_vmax() {
  int64_t p = 1;
  for (int a = 0; a < L - 1; ++a) p *= 256;
  return 7 * p + 127 * ((p - 1) / 255);
}
__host__ __device__ __forceinline__ constexpr uint32_t tile_bytes(uint32_t L, bool top4) {
  return top4 ? (L - 1) * 256 + 128 : L * 256;
}
typedef int v2i __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t sx4(uint32_t v) {   // four nibbles (one per byte, 0..15) -> four signed bytes
  return v | (((v >> 3) & 0x01010101u) * 0xF0u);
}
__device__ __forceinline__ v4i expand_top4(v2i w) {
  const uint32_t w0 = (uint32_t)w[0], w1 = (uint32_t)w[1];
  return v4i{(int)sx4(w0 & 0x0F0F0F0Fu), (int)sx4((w0 >> 4) & 0x0F0F0F0Fu), (int)sx4(w1 & 0x0F0F0F0Fu),
              (int)sx4((w1 >> 4) & 0x0F0F0F0Fu)};
}
// 16 signed bytes of a row (each in [-8, 7]) -> the 8 bytes above
__device__ __forceinline__ v2i pack_top4(const uint8_t (&o)[16]) {
  uint32_t w[2] = {0, 0};
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      w[h] |= (uint32_t)((o[8 * h + i] & 0xF) | ((o[8 * h + 4 + i] & 0xF) << 4)) << (8 * i);
  return v2i{(int)w[0], (int)w[1]};
}

// centred residue -> L balanced base-256 digits (TOP4: centred so that the top digit lies in [-8, 7])
template <int L, bool TOP4 = false>
__device__ __forceinline__ void to_digits(uint64_t x, uint64_t q, int8_t (&d)[L]) {
  int64_t v = TOP4 ? ((int64_t)x > top4_vmax<L>() ? (int64_t)x - (int64_t)q : (int64_t)x)
                   : (x > (q >> 1) ? (int64_t)x - (int64_t)q : (int64_t)x);
#pragma unroll
  for (int a = 0; a < L; ++a) {
    d[a] = (int8_t)(v & 0xFF);
    v = (v - d[a]) >> 8;
  }
}

// A band of the database, u64 [rows][cols][kN] whose first row is matrix row 16 * rt0 -> the row tiles rt0 + blockIdx.y
// of the packed copy.  block = 16 rows x 16 slots; grid = (slots/16, row tiles of the band, KG): every thread stores
// the 16 bytes of one (slot, digit, row), the 16 rows of a slot forming one 256-byte run per digit.  The band holds
// `npts` plaintexts in row-major order (the whole matrix with rt0 = 0: launch_db_pack); plaintexts at or beyond npts --
// the rows past the band's last one, the rest of a partial last row -- and columns at or beyond cols read as zero, so
// every tile is stored whole and the kernel never reads dbp.
// slot0: first slot of the packed copy (a slot-sharded context packs only its own slots, local index j - slot0)
template <int L, bool TOP4>
__global__ void __launch_bounds__(256)
db_pack_band_kernel(const DevParams* __restrict__ P, const uint64_t* __restrict__ db, uint8_t* __restrict__ dbp,
                    uint64_t npts, uint32_t cols, uint32_t kN, uint32_t rt0, uint32_t RT, uint32_t KG, uint32_t GC,
                    uint32_t slot0) {
  constexpr uint32_t TB = tile_bytes(L, TOP4);
  const uint32_t j = slot0 + blockIdx.x * 16 + (threadIdx.x & 15);
  const uint32_t r16 = threadIdx.x >> 4;
  const uint32_t rt = rt0 + blockIdx.y, kg = blockIdx.z;
  const uint32_t r = blockIdx.y * 16 + r16;   // row inside the band
  const uint64_t q = P->mod[j >> P->logN].q;
  // the 16 loads of the row first (all in flight together), then the digits of column t straight into byte t of the
  // digit's 16-byte row / nibble t of the TOP4 row (pack_top4's order): L x 4 dwords, never a register per byte
  uint64_t x[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const uint32_t c = kg * 16 + t;
    const uint64_t pt = (uint64_t)r * cols + c;
    x[t] = 0;
    if (c < cols && pt < npts) x[t] = db[pt * kN + j];
  }
  constexpr int LF = TOP4 ? L - 1 : L;
  uint32_t w[LF][4] = {};
  uint32_t w4[2] = {0, 0};
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    int8_t d[L];
    to_digits<L, TOP4>(x[t], q, d);
#pragma unroll
    for (int a = 0; a < LF; ++a) w[a][t >> 2] |= (uint32_t)(uint8_t)d[a] << (8 * (t & 3));
    if constexpr (TOP4) w4[t >> 3] |= ((uint32_t)d[L - 1] & 0xFu) << (8 * (t & 3) + ((t & 4) ? 4 : 0));
  }
  uint8_t* blk = dbp + db_tile_offset(j - slot0, rt, kg, 0, TB, RT, KG, GC);
#pragma unroll
  for (int a = 0; a < LF; ++a)
    *reinterpret_cast<v4i*>(blk + (size_t)a * 256 + r16 * 16) = v4i{(int)w[a][0], (int)w[a][1], (int)w[a][2], (int)w[a][3]};
  if constexpr (TOP4) *reinterpret_cast<v2i*>(blk + (size_t)(L - 1) * 256 + r16 * 8) = v2i{(int)w4[0], (int)w4[1]};
}

// selectors (per query u64 [cols][2][kN], NTT form) -> packed.  block = 16 x * 16 slots; grid = (kN/16, KG).
// map (slot-sharded multi-GPU step): the packed buffer is cut by slot ranges -- slots [cut[r], cut[r+1]) (multiples of
// 16) start at byte off[r], local slot index inside -- so that every destination rank's slice is one contiguous piece
// of an all-to-all send buffer; n = 0: one piece, the plain layout.
template <int L, bool TOP4>
__global__ void __launch_bounds__(256)
sel_pack_kernel(const DevParams* __restrict__ P, MfmaPtrs sv, uint32_t nq, uint8_t* __restrict__ selp, uint32_t cols,
                uint32_t kN, uint32_t KG, int sel_f64, SliceMap map) {
  constexpr uint32_t TB = tile_bytes(L, TOP4);
  const uint32_t j = blockIdx.x * 16 + (threadIdx.x & 15);
  const uint32_t x = threadIdx.x >> 4;
  const uint32_t kg = blockIdx.y;
  const uint64_t q = P->mod[j >> P->logN].q;
  const uint32_t qi = x >> 1, comp = x & 1;
  if (qi >= nq) return;   // scan_mfma_kernel does not read the columns of absent queries
  const uint64_t* src = (const uint64_t*)sv.p[qi];
  uint8_t o[L][16];
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const uint32_t c = kg * 16 + t;
    uint64_t v = 0;
    if (c < cols) v = src[((size_t)c * 2 + comp) * kN + j];
    if (sel_f64) v = f64_to_u64(__longlong_as_double((long long)v));   // lane-internal selectors: exact doubles
    int8_t d[L];
    to_digits<L, TOP4>(v, q, d);
#pragma unroll
    for (int b = 0; b < L; ++b) o[b][t] = (uint8_t)d[b];
  }
  uint32_t jl = j;
  size_t piece = 0;
  if (map.n) {
    uint32_t r = 0;
    while (r + 1 < map.n && j >= map.cut[r + 1]) ++r;
    jl = j - map.cut[r];
    piece = map.off[r];
  }
  uint8_t* blk = selp + piece + ((size_t)jl * KG + kg) * TB;
#pragma unroll
  for (int b = 0; b < L; ++b) {
    if (TOP4 && b == L - 1) {
      *reinterpret_cast<v2i*>(blk + b * 256 + x * 8) = pack_top4(o[b]);
    } else {
      v4i v;
      __builtin_memcpy(&v, o[b], 16);
      *reinterpret_cast<v4i*>(blk + b * 256 + x * 16) = v;
    }
  }
}

// one plaintext (row r, column c) back from the operand layout: out[j] = residue in [0, q_j), device slot order
template <int L, bool TOP4>
__global__ void __launch_bounds__(256)
db_unpack_kernel(const DevParams* __restrict__ P, const uint8_t* __restrict__ dbp, uint64_t* __restrict__ out,
                 uint32_t r, uint32_t c, uint32_t kN, uint32_t RT, uint32_t KG, uint32_t GC) {
  constexpr uint32_t TB = tile_bytes(L, TOP4);
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= kN) return;
  const uint64_t q = P->mod[j >> P->logN].q;
  const uint8_t* blk = dbp + db_tile_offset(j, r >> 4, c >> 4, 0, TB, RT, KG, GC);
  const uint8_t* p = blk + (r & 15) * 16 + (c & 15);
  int64_t v = 0;
#pragma unroll
  for (int a = L - 1; a >= 0; --a) {
    if (TOP4 && a == L - 1) {
      const uint32_t cc = c & 15;
      const uint8_t byte = blk[(size_t)a * 256 + (r & 15) * 8 + (cc >> 3) * 4 + (cc & 3)];
      const int nib = (cc & 4) ? (byte >> 4) : (byte & 0xF);
      v = nib >= 8 ? nib - 16 : nib;
    } else {
      v = v * 256 + (int8_t)p[(size_t)a * 256];
    }
  }
  out[j] = v < 0 ? (uint64_t)(v + (int64_t)q) : (uint64_t)v;
}

// byte c (0..15) of a 16-byte digit row held as four dwords / nibble c of an 8-byte TOP4 row (pack_top4's order)
__device__ __forceinline__ int row_byte(const uint32_t (&w)[4], int c) { return (int8_t)(w[c >> 2] >> (8 * (c & 3))); }
__device__ __forceinline__ int row_nibble(const uint32_t (&w)[2], int c) {
  const int nib = (int)(w[c >> 3] >> (8 * (c & 3) + ((c & 4) ? 4 : 0))) & 0xF;
  return nib >= 8 ? nib - 16 : nib;
}

// Residue 0 of many plaintexts back from the operand layout (in-place updates with the staging copy released): one
// thread per (unit, slot j < N) reads the unit's L digit rows -- 16 bytes each, 8 for the TOP4 nibble row -- once and
// extracts every touched column from them (db_unpack_kernel reads one byte per digit and slot for ONE plaintext).
// grid = (N / 256, units); out[out0 + rank][j], rank = the column's place among the unit's touched columns.
template <int L, bool TOP4>
__global__ void __launch_bounds__(256)
db_gather_kernel(const DevParams* __restrict__ P, const uint8_t* __restrict__ dbp, const DbUnit* __restrict__ units,
                 uint64_t* __restrict__ out, uint32_t N, uint32_t RT, uint32_t KG, uint32_t GC) {
  constexpr uint32_t TB = tile_bytes(L, TOP4);
  constexpr int LF = TOP4 ? L - 1 : L;
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= N) return;
  const DbUnit u = units[blockIdx.y];
  const uint64_t q = P->mod[0].q;
  const uint8_t* blk = dbp + db_tile_offset(j, u.r >> 4, u.kg, 0, TB, RT, KG, GC);
  const uint32_t r16 = u.r & 15;
  uint32_t w[LF][4];
#pragma unroll
  for (int a = 0; a < LF; ++a) {
    const v4i v = *reinterpret_cast<const v4i*>(blk + (size_t)a * 256 + r16 * 16);
#pragma unroll
    for (int x = 0; x < 4; ++x) w[a][x] = (uint32_t)v[x];
  }
  uint32_t w4[2] = {0, 0};
  if constexpr (TOP4) {
    const v2i v = *reinterpret_cast<const v2i*>(blk + (size_t)(L - 1) * 256 + r16 * 8);
    w4[0] = (uint32_t)v[0];
    w4[1] = (uint32_t)v[1];
  }
  uint32_t rank = 0;
#pragma unroll
  for (int cc = 0; cc < 16; ++cc) {
    if (!((u.mask >> cc) & 1)) continue;
    int64_t v = TOP4 ? row_nibble(w4, cc) : row_byte(w[L - 1], cc);
#pragma unroll
    for (int a = L - 2; a >= 0; --a) v = v * 256 + row_byte(w[a], cc);
    out[(size_t)(u.out0 + rank) * N + j] = v < 0 ? (uint64_t)(v + (int64_t)q) : (uint64_t)v;
    ++rank;
  }
}

// The partial twin of db_pack_band_kernel: one thread per (unit, local slot) reads the unit's digit rows, replaces the
// touched columns with the digits of enc[out0 + rank][j] and writes the rows back.  A unit is one (row, column group) and
// a thread one slot, so no byte -- a TOP4 byte holds columns i and i + 4 -- is written by two threads.
// grid = (nslots / 256, units); slots [slot0, slot0 + nslots) at local index j - slot0.
template <int L, bool TOP4>
__global__ void __launch_bounds__(256)
db_pack_update_kernel(const DevParams* __restrict__ P, const uint64_t* __restrict__ enc, const DbUnit* __restrict__ units,
                      uint8_t* __restrict__ dbp, uint32_t kN, uint32_t slot0, uint32_t nslots, uint32_t RT, uint32_t KG,
                      uint32_t GC) {
  constexpr uint32_t TB = tile_bytes(L, TOP4);
  constexpr int LF = TOP4 ? L - 1 : L;
  const uint32_t jl = blockIdx.x * 256 + threadIdx.x;
  if (jl >= nslots) return;
  const uint32_t j = slot0 + jl;
  const DbUnit u = units[blockIdx.y];
  const uint64_t q = P->mod[j >> P->logN].q;
  uint8_t* blk = dbp + db_tile_offset(jl, u.r >> 4, u.kg, 0, TB, RT, KG, GC);
  const uint32_t r16 = u.r & 15;
  uint32_t w[LF][4];
#pragma unroll
  for (int a = 0; a < LF; ++a) {
    const v4i v = *reinterpret_cast<const v4i*>(blk + (size_t)a * 256 + r16 * 16);
#pragma unroll
    for (int x = 0; x < 4; ++x) w[a][x] = (uint32_t)v[x];
  }
  uint32_t w4[2] = {0, 0};
  if constexpr (TOP4) {
    const v2i v = *reinterpret_cast<const v2i*>(blk + (size_t)(L - 1) * 256 + r16 * 8);
    w4[0] = (uint32_t)v[0];
    w4[1] = (uint32_t)v[1];
  }
  uint32_t rank = 0;
#pragma unroll
  for (int cc = 0; cc < 16; ++cc) {
    if (!((u.mask >> cc) & 1)) continue;
    int8_t d[L];
    to_digits<L, TOP4>(enc[(size_t)(u.out0 + rank) * kN + j], q, d);
    ++rank;
    const uint32_t sh = 8 * (cc & 3);
#pragma unroll
    for (int a = 0; a < LF; ++a) w[a][cc >> 2] = (w[a][cc >> 2] & ~(0xFFu << sh)) | ((uint32_t)(uint8_t)d[a] << sh);
    if constexpr (TOP4) {
      const uint32_t ns = sh + ((cc & 4) ? 4 : 0);
      w4[cc >> 3] = (w4[cc >> 3] & ~(0xFu << ns)) | (((uint32_t)d[L - 1] & 0xFu) << ns);
    }
  }
#pragma unroll
  for (int a = 0; a < LF; ++a)
    *reinterpret_cast<v4i*>(blk + (size_t)a * 256 + r16 * 16) = v4i{(int)w[a][0], (int)w[a][1], (int)w[a][2], (int)w[a][3]};
  if constexpr (TOP4)
    *reinterpret_cast<v2i*>(blk + (size_t)(L - 1) * 256 + r16 * 8) = v2i{(int)w4[0], (int)w4[1]};
}

__device__ __forceinline__ v4i load_tile(const uint8_t* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const v4i*>(p));
}
__device__ __forceinline__ v2i load_tile8(const uint8_t* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const v2i*>(p));
}

// Workgroups per column chunk: first[c] .. first[c+1] run chunk c (equal shares of equal chunks).
struct ChunkPlan {
  uint32_t first[kMaxScanChunks + 1];
  uint32_t nchunks;
};

// The integer fold's magnitudes (tests/scan_fold_model.py restates the fold; tests/test_scan_fold_model.py asserts every
// figure here over the sign-coherent worst-case operands of every instantiated variant and modulus size):
//   |T[s]| <= (L - 1) 2^14 * 64 KS < 2^25.2   a top digit is at most 64 in magnitude (residues are centred and below
//             2^(8 L - 1); 8 as a nibble), so the two top-digit pairs of a diagonal weigh no more than one pair of low digits
//   |group| <= |T| (2^40 - 1) / 255 < 2^57.2  five diagonals, 8 bits apart
//   bias = q << (kBiasBits - bits(q)): a multiple of q with 2^58 <= bias < 2^59, so 0 < group + bias < 2^59.4 whatever
//             the size of q inside its bit count.  (One bit lower -- 2^57 <= bias -- a group of 6 digits over 412 or more
//             columns could reach -2^57.13 < -bias for a prime just above 2^(bits - 1): the cast wrapped.)
//   reduce128 takes any 128-bit value; what it is given here, (top group << 40) + group at the most, is < 2^99.5
constexpr int kBiasBits = 59;

// grid = sum of the plan's workgroups; block = NW waves (wave w <-> slot j0 + w).  NW = 8: two waves per SIMD, 256
// registers each -- selectors of up to 3 k-steps; NW = 4 ("wide"): one wave per SIMD with the whole 512-entry register
// file (VGPRs + AGPRs: MFMA operands may live in either), selectors of up to 7 k-steps = 28 column groups in registers,
// so the matrices of cfg 4 / 5 (27 / 21 column groups) are scanned in ONE chunk with all but the last k-step full.  A workgroup is persistent: it walks
// the units u = i, i + n_c, ... (i = its index among the n_c workgroups of its chunk; a unit = one slot block of one
// group of queries, u = group * nblocks + block) and, while it folds and stores the last row tile of one unit, the
// selector tiles and the first database tiles of its next unit are already in flight (one workgroup per CU at this
// register count, so nothing else would hide that latency).
// Chunk ch covers column groups [ch * GC, (ch + 1) * GC) with GC = ceil(KG / nchunks) <= 4 KS -- equal chunks, so
// that equal shares of the chip finish together (7 k-steps split 3/3/1 left a third of the CUs idle for two thirds
// of the pass) -- and writes to out + ch * chunk_stride (partial sums when nchunks > 1).
// Groups (ScanGroups): one launch serves up to kMaxScanGroups groups of <= 8 queries over the SAME database slots --
// group g reads its packed selectors at sel[g] and writes query q of the group to out[g] + q * out_qstride.  One group
// is the single-GPU pass; several are the slot-sharded multi-GPU step, where a rank scans its slots for every query of
// the step in one launch.
// Slots: the launch covers the slots [slot0, slot0 + nslots) of the ring's k N; database, packed selectors and output
// are indexed by the LOCAL slot j - slot0 (a slot-sharded context holds only its own slots of every plaintext), a row
// of the output is out_rstride slots long.  slot0 = 0, nslots = out_rstride = k N: the whole database.
// TOP4: the top digit of both operands is stored as nibbles (above): its database tiles stay packed in two registers per
// lane until their k-step is due; the selectors' are unpacked once per unit.
// F64F: the digit diagonals are folded in exact fp64 arithmetic (all data moduli < 2^50): four diagonals combine exactly
// in one double (|C| < 2^49.01), chunk c times 2^(32 c) mod q with the 6-operation exact product of arith.h --
// ~45 full-rate operations per value against ~170 mostly quarter-rate 64-bit integer ones.  Same canonical residues.
#define PIRGPU_SCAN_DB_OF(g_) dbp
template <int L, int KS, int NW, bool TOP4, bool F64F = false>
__global__ void __launch_bounds__(NW * 64)
scan_mfma_kernel(const DevParams* __restrict__ P, const uint8_t* __restrict__ dbp, ScanGroups grp, uint32_t rows,
                 uint32_t RT, uint32_t KG, uint64_t chunk_stride, ChunkPlan plan, uint32_t GC, uint32_t slot0,
                 uint32_t nslots, uint64_t out_qstride, uint32_t out_rstride, uint32_t blk_major) {
#include "scan_mfma_body.inc"
}
#undef PIRGPU_SCAN_DB_OF

// The same pass over several databases of one shape (a context with tables): group g -- a run of
// queries that named the same table -- multiplies its packed selectors with the operand layout at grp.db[g].  One
// launch for all runs of a batch group instead of one launch per run; the whole ring, group-major units.
#define PIRGPU_SCAN_DB_OF(g_) grp.db[g_]
template <int L, int KS, int NW, bool TOP4, bool F64F = false>
__global__ void __launch_bounds__(NW * 64)
scan_mfma_runs_kernel(const DevParams* __restrict__ P, ScanGroupsDb grp, uint32_t rows, uint32_t RT, uint32_t KG,
                      uint64_t chunk_stride, ChunkPlan plan, uint32_t GC, uint32_t nslots, uint64_t out_qstride) {
  constexpr uint32_t slot0 = 0, blk_major = 0;
  const uint32_t out_rstride = nslots;
#include "scan_mfma_body.inc"
}
#undef PIRGPU_SCAN_DB_OF

// Slot-sharded multi-GPU step: the row sums of a rank's own nq_total queries arrive from every rank h as
// [query][row, comp][slots of h] (the all-to-all's receive buffer; rank h's block starts at word nq_total * RC * cut[h]);
// this puts the queries q0 .. q0 + gridDim.z - 1 back into the [query][row, comp][k N] layout the inverse transform
// reads.  Two words per thread; cuts are multiples of 16.
__global__ void __launch_bounds__(256)
slots_assemble_kernel(const uint64_t* __restrict__ src, uint64_t* __restrict__ dst, SliceMap map, uint32_t RC, uint32_t kN,
                      uint64_t dst_qstride, uint32_t nq_total, uint32_t q0) {
  const uint32_t j = (blockIdx.x * 256 + threadIdx.x) * 2;
  const uint32_t rc = blockIdx.y, q = blockIdx.z;
  if (j >= kN) return;
  uint32_t h = 0;
  while (h + 1 < map.n && j >= map.cut[h + 1]) ++h;
  const uint32_t c0 = map.cut[h], width = map.cut[h + 1] - c0;
  typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
  const uint64_t* s = src + (size_t)nq_total * RC * c0 + ((size_t)(q0 + q) * RC + rc) * width + (j - c0);
  *reinterpret_cast<u64x2*>(dst + (size_t)q * dst_qstride + (size_t)rc * kN + j) =
      __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(s));
}

// ------------------------------------------------------------------ host side

MfmaGeom mfma_geometry(const DevParams& hp, uint32_t rows, uint32_t cols, int wide_override, bool allow_top4) {
  MfmaGeom gm{};
  uint32_t bits = 0;
  for (uint32_t i = 0; i < hp.k; ++i) bits = std::max<uint32_t>(bits, 64 - (uint32_t)__builtin_clzll(hp.mod[i].q));
  // L balanced digits cover |v| <= 127 (256^L - 1) / 255 > 2^(8L - 2); centred residues are < 2^(bits - 1)
  if (bits <= 39) gm.L = 5;
  else if (bits <= 47) gm.L = 6;
  else if (bits <= 55) gm.L = 7;
  else return gm;                       // L = 0: not applicable
  if (rows < 1 || cols < 1) { gm.L = 0; return gm; }
  gm.RT = (rows + 15) / 16;
  gm.KG = (cols + 15) / 16;
  // k-steps (64 columns) whose selectors a wave keeps in registers: 3 (L <= 6) / 2 (L = 7) with two waves per SIMD
  // (NW = 8), 7 / 6 with one wave per SIMD and the whole register file (NW = 4, "wide").  Matrices that fit the narrow
  // budget keep it (cfg 3: 11 column groups); wider ones take the wide kernel so that they are scanned in one chunk
  // (cfg 4: 27 groups = 7 k-steps, cfg 5: 21 = 6) instead of three chunks with a quarter-full last k-step each.
  const uint32_t steps = (gm.KG + 3) / 4;
  const uint32_t narrow_ks = gm.L <= 6 ? 3 : 2, wide_ks = gm.L <= 6 ? 7 : 6;
  bool wide = steps > narrow_ks;
  if (wide_override >= 0) wide = wide_override != 0;
  gm.NW = wide ? 4 : 8;
  const uint32_t max_ks = wide ? wide_ks : narrow_ks;
  gm.KS = std::min(max_ks, steps);
  gm.nchunks = (steps + gm.KS - 1) / gm.KS;
  if (gm.nchunks > (uint32_t)kMaxScanChunks) { gm.L = 0; return gm; }   // wider than 16 x 4 KS x 16 columns: 64-bit kernels
  gm.GC = (gm.KG + gm.nchunks - 1) / gm.nchunks;   // equal chunks (<= 4 KS groups each)
  gm.KS = (gm.GC + 3) / 4;
  if (wide && gm.KS < 3) gm.NW = 8;                // the wide kernel is instantiated for 3..7 k-steps
  // top digit as a nibble when every residue is below 2^(8 (L - 1) + 4) (36 / 44 bits at L = 5 / 6: cfg 2, 3 and 4).
  // Not at L = 7 (cfg 5, 49 bits < 2^52 would allow it): the 4-wave kernel with 6 k-steps is out of registers there and
  // the unpacking temporaries spill (scan 9.4 against 8.6 ms) -- the L = 7 variants are not even instantiated.
  gm.top4 = allow_top4 && gm.L <= 6 && bits <= 8 * (gm.L - 1) + 4 ? 1 : 0;
  gm.tile_bytes = tile_bytes(gm.L, gm.top4 != 0);
  const size_t kN = (size_t)hp.k * hp.N;
  gm.db_bytes = kN * gm.RT * gm.KG * gm.tile_bytes;
  gm.sel_bytes = kN * gm.KG * gm.tile_bytes;
  return gm;
}

hipError_t launch_db_pack(hipStream_t st, const DevParams* P, const MfmaGeom& gm, const uint64_t* db, uint8_t* dbp,
                          uint32_t rows, uint32_t cols, uint32_t kN, uint32_t slot0, uint32_t nslots) {
  return launch_db_pack_band(st, P, gm, db, dbp, 0, gm.RT, (uint64_t)rows * cols, cols, kN, slot0, nslots);
}

hipError_t launch_db_pack_band(hipStream_t st, const DevParams* P, const MfmaGeom& gm, const uint64_t* band, uint8_t* dbp,
                               uint32_t rt0, uint32_t n_rt, uint64_t npts, uint32_t cols, uint32_t kN, uint32_t slot0,
                               uint32_t nslots) {
  if (nslots == 0) nslots = kN - slot0;
  if (slot0 % 16 || nslots % 16 || slot0 + nslots > kN) return hipErrorInvalidValue;
  // the band stays inside the packed copy and holds no more than its row tiles
  if (!n_rt || n_rt > 65535 || rt0 > gm.RT || n_rt > gm.RT - rt0 || (cols + 15) / 16 != gm.KG ||
      npts > (uint64_t)n_rt * 16 * cols)
    return hipErrorInvalidValue;
  const dim3 grid(nslots / 16, n_rt, gm.KG);
#define PIRGPU_DBPACK(L_, T_)                                                                                      \
  hipLaunchKernelGGL((db_pack_band_kernel<L_, T_>), grid, dim3(256), 0, st, P, band, dbp, npts, cols, kN, rt0, gm.RT, \
                     gm.KG, gm.GC, slot0)
  switch (gm.L) {
    case 5:
      if (gm.top4) PIRGPU_DBPACK(5, true);
      else PIRGPU_DBPACK(5, false);
      break;
    case 6:
      if (gm.top4) PIRGPU_DBPACK(6, true);
      else PIRGPU_DBPACK(6, false);
      break;
    case 7: PIRGPU_DBPACK(7, false); break;
    default: return hipErrorInvalidValue;
  }
#undef PIRGPU_DBPACK
  return hipGetLastError();
}

hipError_t launch_db_unpack(hipStream_t st, const DevParams* P, const MfmaGeom& gm, const uint8_t* dbp, uint64_t* out,
                            uint32_t row, uint32_t col, uint32_t kN) {
  const dim3 grid((kN + 255) / 256);
  switch (gm.L) {
    case 5:
      if (gm.top4) hipLaunchKernelGGL((db_unpack_kernel<5, true>), grid, dim3(256), 0, st, P, dbp, out, row, col, kN, gm.RT, gm.KG, gm.GC);
      else hipLaunchKernelGGL((db_unpack_kernel<5, false>), grid, dim3(256), 0, st, P, dbp, out, row, col, kN, gm.RT, gm.KG, gm.GC);
      break;
    case 6:
      if (gm.top4) hipLaunchKernelGGL((db_unpack_kernel<6, true>), grid, dim3(256), 0, st, P, dbp, out, row, col, kN, gm.RT, gm.KG, gm.GC);
      else hipLaunchKernelGGL((db_unpack_kernel<6, false>), grid, dim3(256), 0, st, P, dbp, out, row, col, kN, gm.RT, gm.KG, gm.GC);
      break;
    case 7: hipLaunchKernelGGL((db_unpack_kernel<7, false>), grid, dim3(256), 0, st, P, dbp, out, row, col, kN, gm.RT, gm.KG, gm.GC); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_db_gather(hipStream_t st, const DevParams* P, const MfmaGeom& gm, const uint8_t* dbp,
                            const DbUnit* units, uint32_t n_units, uint64_t* out, uint32_t N) {
  if (!n_units) return hipSuccess;
  if (n_units > 65535) return hipErrorInvalidValue;
  const dim3 grid((N + 255) / 256, n_units);
#define PIRGPU_DBGATHER(L_, T_) \
  hipLaunchKernelGGL((db_gather_kernel<L_, T_>), grid, dim3(256), 0, st, P, dbp, units, out, N, gm.RT, gm.KG, gm.GC)
  switch (gm.L) {
    case 5:
      if (gm.top4) PIRGPU_DBGATHER(5, true);
      else PIRGPU_DBGATHER(5, false);
      break;
    case 6:
      if (gm.top4) PIRGPU_DBGATHER(6, true);
      else PIRGPU_DBGATHER(6, false);
      break;
    case 7: PIRGPU_DBGATHER(7, false); break;
    default: return hipErrorInvalidValue;
  }
#undef PIRGPU_DBGATHER
  return hipGetLastError();
}

hipError_t launch_db_pack_update(hipStream_t st, const DevParams* P, const MfmaGeom& gm, const uint64_t* enc,
                                 const DbUnit* units, uint32_t n_units, uint8_t* dbp, uint32_t kN, uint32_t slot0,
                                 uint32_t nslots) {
  if (!n_units) return hipSuccess;
  if (nslots == 0) nslots = kN - slot0;
  if (n_units > 65535 || slot0 % 16 || nslots % 16 || slot0 + nslots > kN) return hipErrorInvalidValue;
  const dim3 grid((nslots + 255) / 256, n_units);
#define PIRGPU_DBPACKUPD(L_, T_)                                                                                    \
  hipLaunchKernelGGL((db_pack_update_kernel<L_, T_>), grid, dim3(256), 0, st, P, enc, units, dbp, kN, slot0, nslots, \
                     gm.RT, gm.KG, gm.GC)
  switch (gm.L) {
    case 5:
      if (gm.top4) PIRGPU_DBPACKUPD(5, true);
      else PIRGPU_DBPACKUPD(5, false);
      break;
    case 6:
      if (gm.top4) PIRGPU_DBPACKUPD(6, true);
      else PIRGPU_DBPACKUPD(6, false);
      break;
    case 7: PIRGPU_DBPACKUPD(7, false); break;
    default: return hipErrorInvalidValue;
  }
#undef PIRGPU_DBPACKUPD
  return hipGetLastError();
}

hipError_t launch_sel_pack(hipStream_t st, const DevParams* P, const MfmaGeom& gm, const MfmaPtrs& sv, uint32_t nq,
                           uint8_t* selp, uint32_t cols, uint32_t kN, bool sel_f64, const SliceMap* map) {
  const int f = sel_f64 ? 1 : 0;
  const dim3 grid(kN / 16, gm.KG);
  SliceMap m{};
  if (map) {
    m = *map;
    if (m.n > (uint32_t)kMaxSlices || m.cut[0] != 0 || m.cut[m.n] != kN) return hipErrorInvalidValue;
    for (uint32_t r = 0; r <= m.n; ++r)
      if (m.cut[r] % 16) return hipErrorInvalidValue;
  }
#define PIRGPU_SELPACK(L_, T_) \
  hipLaunchKernelGGL((sel_pack_kernel<L_, T_>), grid, dim3(256), 0, st, P, sv, nq, selp, cols, kN, gm.KG, f, m)
  switch (gm.L) {
    case 5:
      if (gm.top4) PIRGPU_SELPACK(5, true);
      else PIRGPU_SELPACK(5, false);
      break;
    case 6:
      if (gm.top4) PIRGPU_SELPACK(6, true);
      else PIRGPU_SELPACK(6, false);
      break;
    case 7: PIRGPU_SELPACK(7, false); break;
    default: return hipErrorInvalidValue;
  }
#undef PIRGPU_SELPACK
  return hipGetLastError();
}

hipError_t launch_slots_assemble(hipStream_t st, const uint64_t* src, uint64_t* dst, const SliceMap& map, uint32_t RC,
                                 uint32_t kN, uint32_t nq, uint64_t dst_qstride, uint32_t nq_total, uint32_t q0) {
  if (map.n == 0 || map.n > (uint32_t)kMaxSlices || map.cut[0] != 0 || map.cut[map.n] != kN || q0 + nq > nq_total)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(slots_assemble_kernel, dim3((kN / 2 + 255) / 256, RC, nq), dim3(256), 0, st, src, dst, map, RC, kN,
                     dst_qstride, nq_total, q0);
  return hipGetLastError();
}

static uint32_t scan_wgs_all() {
  // persistent workgroups: one per CU and chunk (at most), each walking its share of the kN/8 slot blocks
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

template <int L, int KS, int NW, bool TOP4, bool F64F>
static void launch_scan_mfma_variant(hipStream_t st, const DevParams* P, const MfmaGeom& gm, const uint8_t* dbp,
                                     const ScanGroups& grp, uint32_t rows, uint64_t chunk_stride, uint32_t wgs_req,
                                     uint32_t slot0, uint32_t nslots, uint64_t out_qstride, uint32_t out_rstride,
                                     bool blk_major) {
  // wgs_req (batch pipeline): a workgroup takes a CU's whole register file, so a launch on fewer CUs leaves the others
  // to the VALU-bound kernels of the other lane -- the HBM-bound pass and the transforms then really overlap
  const uint32_t wgs = wgs_req ? std::min(wgs_req, scan_wgs_all()) : scan_wgs_all();
  // equal shares of the chip for the (equal) column chunks
  ChunkPlan plan{};
  plan.nchunks = gm.nchunks;
  const uint32_t units = nslots / NW * std::max<uint32_t>(grp.n, 1);
  const uint32_t share = std::min<uint32_t>(units, std::max<uint32_t>(1, wgs / std::min<uint32_t>(gm.nchunks, wgs)));
  for (uint32_t c = 0; c <= gm.nchunks; ++c) plan.first[c] = c * share;   // share >= 1: no chunk without workgroups
  hipLaunchKernelGGL((scan_mfma_kernel<L, KS, NW, TOP4, F64F>), dim3(gm.nchunks * share), dim3(NW * 64), 0, st, P, dbp, grp,
                     rows, gm.RT, gm.KG, chunk_stride, plan, gm.GC, slot0, nslots, out_qstride, out_rstride,
                     blk_major ? 1u : 0u);
}

hipError_t launch_scan_mfma_groups(hipStream_t st, const DevParams* P, const MfmaGeom& gm, const uint8_t* dbp,
                                   const ScanGroups& grp, uint32_t rows, uint64_t chunk_stride, uint32_t wgs, bool f64_fold,
                                   uint32_t slot0, uint32_t nslots, uint64_t out_qstride, uint32_t out_rstride, bool blk_major) {
  if (grp.n == 0 || grp.n > (uint32_t)kMaxScanGroups || nslots == 0 || nslots % gm.NW) return hipErrorInvalidValue;
#define PIRGPU_MFMA_ARGS st, P, gm, dbp, grp, rows, chunk_stride, wgs, slot0, nslots, out_qstride, out_rstride, blk_major
#define PIRGPU_MFMA_CASE(L_, KS_, NW_)                                                                    \
  if (gm.L == L_ && gm.KS == KS_ && gm.NW == NW_) {                                                                 \
    if constexpr (L_ <= 6) {                                                                                         \
      if (gm.top4) {                                                                                                 \
        if (f64_fold) launch_scan_mfma_variant<L_, KS_, NW_, true, true>(PIRGPU_MFMA_ARGS);                          \
        else launch_scan_mfma_variant<L_, KS_, NW_, true, false>(PIRGPU_MFMA_ARGS);                                  \
        return hipGetLastError();                                                                                    \
      }                                                                                                              \
    }                                                                                                                \
    if (gm.top4) return hipErrorInvalidValue;                                                                        \
    if (f64_fold) launch_scan_mfma_variant<L_, KS_, NW_, false, true>(PIRGPU_MFMA_ARGS);                             \
    else launch_scan_mfma_variant<L_, KS_, NW_, false, false>(PIRGPU_MFMA_ARGS);                                     \
    return hipGetLastError();                                                                                        \
  }
  PIRGPU_MFMA_CASE(5, 1, 8) PIRGPU_MFMA_CASE(5, 2, 8) PIRGPU_MFMA_CASE(5, 3, 8)
  PIRGPU_MFMA_CASE(6, 1, 8) PIRGPU_MFMA_CASE(6, 2, 8) PIRGPU_MFMA_CASE(6, 3, 8)
  PIRGPU_MFMA_CASE(7, 1, 8) PIRGPU_MFMA_CASE(7, 2, 8)
  PIRGPU_MFMA_CASE(5, 3, 4) PIRGPU_MFMA_CASE(5, 4, 4) PIRGPU_MFMA_CASE(5, 5, 4) PIRGPU_MFMA_CASE(5, 6, 4) PIRGPU_MFMA_CASE(5, 7, 4)
  PIRGPU_MFMA_CASE(6, 3, 4) PIRGPU_MFMA_CASE(6, 4, 4) PIRGPU_MFMA_CASE(6, 5, 4) PIRGPU_MFMA_CASE(6, 6, 4) PIRGPU_MFMA_CASE(6, 7, 4)
  PIRGPU_MFMA_CASE(7, 3, 4) PIRGPU_MFMA_CASE(7, 4, 4) PIRGPU_MFMA_CASE(7, 5, 4) PIRGPU_MFMA_CASE(7, 6, 4)
#undef PIRGPU_MFMA_CASE
#undef PIRGPU_MFMA_ARGS
  return hipErrorInvalidValue;
}

// Runs of a batch group over their own tables (8-wave geometries: the narrow matrices many small tables have; a matrix
// wide enough for the 4-wave kernel scans long enough per run that the launches do not matter, and keeps them).
// (<6, 3, 8> -- only reachable with the 4-wave kernel forced off -- spills and is not built for runs either)
bool scan_mfma_runs_supported(const MfmaGeom& gm) {
  return gm.L >= 5 && gm.L <= 7 && gm.NW == 8 && gm.KS >= 1 && gm.KS <= (gm.L == 5 ? 3u : 2u);
}

template <int L, int KS, bool TOP4, bool F64F>
static void launch_scan_mfma_runs_variant(hipStream_t st, const DevParams* P, const MfmaGeom& gm, const ScanGroupsDb& grp,
                                          uint32_t rows, uint64_t chunk_stride, uint32_t wgs_req, uint32_t kN,
                                          uint64_t out_qstride) {
  constexpr int NW = 8;
  const uint32_t wgs = wgs_req ? std::min(wgs_req, scan_wgs_all()) : scan_wgs_all();
  ChunkPlan plan{};
  plan.nchunks = gm.nchunks;
  const uint32_t units = kN / NW * grp.n;
  const uint32_t share = std::min<uint32_t>(units, std::max<uint32_t>(1, wgs / std::min<uint32_t>(gm.nchunks, wgs)));
  for (uint32_t c = 0; c <= gm.nchunks; ++c) plan.first[c] = c * share;
  hipLaunchKernelGGL((scan_mfma_runs_kernel<L, KS, NW, TOP4, F64F>), dim3(gm.nchunks * share), dim3(NW * 64), 0, st, P, grp,
                     rows, gm.RT, gm.KG, chunk_stride, plan, gm.GC, kN, out_qstride);
}

hipError_t launch_scan_mfma_runs(hipStream_t st, const DevParams* P, const MfmaGeom& gm, const ScanGroupsDb& grp,
                                 uint32_t rows, uint32_t kN, uint64_t chunk_stride, uint32_t wgs, bool f64_fold,
                                 uint64_t out_qstride) {
  if (grp.n == 0 || grp.n > (uint32_t)kMaxScanGroups || kN == 0 || kN % 8 || !scan_mfma_runs_supported(gm))
    return hipErrorInvalidValue;
  for (uint32_t g = 0; g < grp.n; ++g)
    if (!grp.db[g] || !grp.sel[g] || !grp.out[g] || grp.nq[g] == 0 || grp.nq[g] > kMaxMfmaQueries) return hipErrorInvalidValue;
#define PIRGPU_RUNS_ARGS st, P, gm, grp, rows, chunk_stride, wgs, kN, out_qstride
#define PIRGPU_RUNS_CASE(L_, KS_)                                                          \
  if (gm.L == L_ && gm.KS == KS_) {                                                        \
    if constexpr (L_ <= 6) {                                                               \
      if (gm.top4) {                                                                       \
        if (f64_fold) launch_scan_mfma_runs_variant<L_, KS_, true, true>(PIRGPU_RUNS_ARGS); \
        else launch_scan_mfma_runs_variant<L_, KS_, true, false>(PIRGPU_RUNS_ARGS);        \
        return hipGetLastError();                                                          \
      }                                                                                    \
    }                                                                                      \
    if (gm.top4) return hipErrorInvalidValue;                                              \
    if (f64_fold) launch_scan_mfma_runs_variant<L_, KS_, false, true>(PIRGPU_RUNS_ARGS);   \
    else launch_scan_mfma_runs_variant<L_, KS_, false, false>(PIRGPU_RUNS_ARGS);           \
    return hipGetLastError();                                                              \
  }
  PIRGPU_RUNS_CASE(5, 1) PIRGPU_RUNS_CASE(5, 2) PIRGPU_RUNS_CASE(5, 3)
  PIRGPU_RUNS_CASE(6, 1) PIRGPU_RUNS_CASE(6, 2)
  PIRGPU_RUNS_CASE(7, 1) PIRGPU_RUNS_CASE(7, 2)
#undef PIRGPU_RUNS_CASE
#undef PIRGPU_RUNS_ARGS
  return hipErrorInvalidValue;
}

// One group of up to 8 queries over the whole ring (the single-GPU pass): query q writes to out + q * out_qstride.
hipError_t launch_scan_mfma(hipStream_t st, const DevParams* P, const MfmaGeom& gm, const uint8_t* dbp,
                            const uint8_t* selp, uint64_t* out, uint64_t out_qstride, uint32_t nq, uint32_t rows,
                            uint32_t kN, uint64_t chunk_stride, uint32_t wgs, bool f64_fold) {
  ScanGroups grp{};
  grp.n = 1;
  grp.sel[0] = selp;
  grp.out[0] = out;
  grp.nq[0] = (uint8_t)nq;
  return launch_scan_mfma_groups(st, P, gm, dbp, grp, rows, chunk_stride, wgs, f64_fold, 0, kN, out_qstride, kN, false);
}

}  // namespace pirgpu
