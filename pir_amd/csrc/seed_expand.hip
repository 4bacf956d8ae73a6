// seed_expand.hip -- gfx950 kernel that re-samples the c1 half of seed-compressed key objects:
//
//   seed_expand_kernel   out[o][n_mod][N] = sample_poly_uniform(BlakePRNG(seed_o), moduli), bit for bit what
//                        wire::sample_poly_uniform (wire_codec.cpp) and tests/seal_wire.py compute on the host
//
// The definition, restated.  BlakePRNG is counter mode: refill r of a seed is the 4096 bytes
// blake2xb(4096, le64(r), key = seed), i.e. a root hash H0(r) -- BLAKE2b-512 over the 128-byte key block and the 8-byte
// counter with xof_length = 4096 in the parameter block, two compressions -- and 64 output blocks
// B(r, b) = BLAKE2b-512(H0(r)) with node_offset = b, one compression each.  Every little-endian u64 word w of that
// stream is one CANDIDATE rand = (lo32(w) << 31) | (hi32(w) >> 1); modulus j accepts it iff rand < max_multiple_j =
// (2^63 - 1) - ((2^63 - 1) mod q_j) - 1 and then stores rand mod q_j.  Modulus j + 1 starts at the candidate after the
// N-th accepted one of modulus j, wherever that falls.
//
// One workgroup per object walks the moduli in order.  A chunk is kSeedThreads / 64 whole refills from the refill the
// current position lies in: one thread per 64-byte block (8 candidates), candidates in front of the position masked
// off, a workgroup prefix sum over the accept counts, accepted candidate number c of the modulus stored at out[j][c]
// while c < N.  The thread that stores number N - 1 publishes the position behind it; the block that straddles the
// boundary is recomputed by the next modulus.  Root hashes are computed once per refill, a window of them at a time
// (one thread per refill), and shared through the LDS.  One code path, exact for every modulus below 2^63; 64-bit
// integer adds, xors and rotates only, the twelve rounds written out with the message schedule as literals.
#include <hip/hip_runtime.h>

#include "arith.h"
#include "kernels.h"

namespace pirgpu {

namespace {

// Workgroup of kSeedThreads = 512 (kernels.h): the build reports 81 VGPRs, no scratch and 5 waves per SIMD for this
// kernel, so two workgroups fit a CU and the size is not register bound.  8 waves (two per SIMD, eight refills per
// chunk) cover a modulus of N = 4096 in one chunk and keep the LDS window (32 KB) and the prefix sum small.
constexpr uint32_t kBlockWords = 8;      // candidates per 64-byte output block
constexpr uint32_t kRefillBlocks = 64;   // output blocks per 4096-byte refill
constexpr uint32_t kRefillWords = kBlockWords * kRefillBlocks;
constexpr uint32_t kChunkRefills = kSeedThreads / kRefillBlocks;

constexpr uint64_t kIV0 = 0x6a09e667f3bcc908ULL, kIV1 = 0xbb67ae8584caa73bULL, kIV2 = 0x3c6ef372fe94f82bULL,
                   kIV3 = 0xa54ff53a5f1d36f1ULL, kIV4 = 0x510e527fade682d1ULL, kIV5 = 0x9b05688c2b3e6c1fULL,
                   kIV6 = 0x1f83d9abfb41bd6bULL, kIV7 = 0x5be0cd19137e2179ULL;

__device__ __forceinline__ uint64_t rotr64(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }

#define B2G(a, b, c, d, x, y)       \
  v[a] = v[a] + v[b] + (x);         \
  v[d] = rotr64(v[d] ^ v[a], 32);   \
  v[c] = v[c] + v[d];               \
  v[b] = rotr64(v[b] ^ v[c], 24);   \
  v[a] = v[a] + v[b] + (y);         \
  v[d] = rotr64(v[d] ^ v[a], 16);   \
  v[c] = v[c] + v[d];               \
  v[b] = rotr64(v[b] ^ v[c], 63);
#define B2ROUND(s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15) \
  B2G(0, 4, 8, 12, m[s0], m[s1])                                                       \
  B2G(1, 5, 9, 13, m[s2], m[s3])                                                       \
  B2G(2, 6, 10, 14, m[s4], m[s5])                                                      \
  B2G(3, 7, 11, 15, m[s6], m[s7])                                                      \
  B2G(0, 5, 10, 15, m[s8], m[s9])                                                      \
  B2G(1, 6, 11, 12, m[s10], m[s11])                                                    \
  B2G(2, 7, 8, 13, m[s12], m[s13])                                                     \
  B2G(3, 4, 9, 14, m[s14], m[s15])

// BLAKE2b compression (RFC 7693) of the block m into h; t0 = bytes hashed so far, this block included.  Always inlined
// with literal indices: words of m that a call site sets to zero fold away.
template <bool kLast>
__device__ __forceinline__ void b2_compress(uint64_t (&h)[8], const uint64_t (&m)[16], uint64_t t0) {
  uint64_t v[16] = {h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], kIV0, kIV1, kIV2, kIV3, kIV4 ^ t0, kIV5,
                    kLast ? ~kIV6 : kIV6, kIV7};
  B2ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
  B2ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3)
  B2ROUND(11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4)
  B2ROUND(7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8)
  B2ROUND(9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13)
  B2ROUND(2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9)
  B2ROUND(12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11)
  B2ROUND(13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10)
  B2ROUND(6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5)
  B2ROUND(10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0)
  B2ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
  B2ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3)
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] ^= v[i] ^ v[i + 8];
}
#undef B2ROUND
#undef B2G

// H0 of refill `counter`: BLAKE2b-512, key_length = 64, fanout = depth = 1, xof_length = 4096, over the key block
// (seed, zero padded to 128 bytes) and le64(counter).
__device__ __forceinline__ void b2x_root(const uint64_t (&seed)[8], uint64_t counter, uint64_t (&h)[8]) {
  h[0] = kIV0 ^ (64ULL | (64ULL << 8) | (1ULL << 16) | (1ULL << 24));
  h[1] = kIV1 ^ (4096ULL << 32);
  h[2] = kIV2; h[3] = kIV3; h[4] = kIV4; h[5] = kIV5; h[6] = kIV6; h[7] = kIV7;
  {
    const uint64_t m[16] = {seed[0], seed[1], seed[2], seed[3], seed[4], seed[5], seed[6], seed[7], 0, 0, 0, 0, 0, 0, 0, 0};
    b2_compress<false>(h, m, 128);
  }
  {
    const uint64_t m[16] = {counter, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    b2_compress<true>(h, m, 136);
  }
}

// Output block `node` of a refill: BLAKE2b-512 of H0 with fanout = depth = 0, leaf_length = inner_length = 64,
// node_offset = node, xof_length = 4096.
__device__ __forceinline__ void b2x_block(const uint64_t* h0, uint32_t node, uint64_t (&h)[8]) {
  h[0] = kIV0 ^ (64ULL | (64ULL << 32));
  h[1] = kIV1 ^ ((uint64_t)node | (4096ULL << 32));
  h[2] = kIV2 ^ (64ULL << 8);
  h[3] = kIV3; h[4] = kIV4; h[5] = kIV5; h[6] = kIV6; h[7] = kIV7;
  const uint64_t m[16] = {h0[0], h0[1], h0[2], h0[3], h0[4], h0[5], h0[6], h0[7], 0, 0, 0, 0, 0, 0, 0, 0};
  b2_compress<true>(h, m, 64);
}

}  // namespace

// seeds [n_obj][64] bytes; object o writes out + o * obj_stride, [n_mod][N] words.  stats[0] += rejected draws;
// stats[1] is set when an object ran into max_refills (never for a prime modulus: the acceptance rate is above 1/2).
__global__ void __launch_bounds__(kSeedThreads)
seed_expand_kernel(SeedExpandArgs A, const uint8_t* __restrict__ seeds, uint64_t* __restrict__ out, uint64_t obj_stride,
                   unsigned long long* __restrict__ stats) {
  __shared__ uint64_t s_h0[kSeedThreads][8];   // root hashes of the refills [wbase, wbase + n_win)
  __shared__ uint32_t s_wave[kSeedThreads / 64];
  __shared__ unsigned long long s_next;        // the position behind the N-th accepted candidate of a modulus
  __shared__ uint32_t s_rej;
  const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint32_t N = A.N;
  uint64_t seed[8];
  {
    const uint8_t* sp = seeds + (size_t)blockIdx.x * 64;   // any alignment: assembled from bytes
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      uint64_t w = 0;
#pragma unroll
      for (int b = 0; b < 8; ++b) w |= (uint64_t)sp[8 * i + b] << (8 * b);
      seed[i] = w;
    }
  }
  uint64_t* dst = out + (size_t)blockIdx.x * obj_stride;
  if (t == 0) s_rej = 0;
  uint64_t pos = 0;                 // stream position in candidates (u64 words); workgroup uniform
  uint64_t wbase = 0;
  uint32_t n_win = 0;               // nothing computed yet
  uint32_t rejected = 0;
  bool overrun = false;
  for (uint32_t j = 0; j < A.n_mod && !overrun; ++j) {
    const ModConst mc = A.mod[j];
    const uint64_t max_multiple = A.max_multiple[j];
    uint32_t written = 0;
    while (written < N) {
      const uint64_t r0 = pos / kRefillWords;
      if (r0 + kChunkRefills > A.max_refills) {
        overrun = true;
        break;
      }
      if (r0 < wbase || r0 + kChunkRefills > wbase + n_win) {
        // a new window of root hashes from r0 on: what the remaining residues need without a rejection plus one
        // refill of slack, at least a chunk, at most one per thread
        const uint64_t left = (uint64_t)(A.n_mod - j) * N - written;
        uint64_t want = (pos % kRefillWords + left + kRefillWords - 1) / kRefillWords + 1;
        want = (want + kChunkRefills - 1) / kChunkRefills * kChunkRefills;
        __syncthreads();            // every reader of the old window is done
        wbase = r0;
        n_win = (uint32_t)(want < kSeedThreads ? want : kSeedThreads);
        if (t < n_win) {
          uint64_t h[8];
          b2x_root(seed, wbase + t, h);
#pragma unroll
          for (int i = 0; i < 8; ++i) s_h0[t][i] = h[i];
        }
        __syncthreads();
      }
      // one output block per thread
      uint64_t h[8];
      b2x_block(s_h0[(uint32_t)(r0 - wbase) + wave], lane, h);
      const uint64_t first = (r0 + wave) * kRefillWords + (uint64_t)lane * kBlockWords;   // position of h[0]
      uint64_t rnd[8];
      uint32_t cnt = 0, acc_mask = 0, valid_mask = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const uint64_t lo = h[i] & 0xffffffffULL, hi = h[i] >> 32;
        rnd[i] = (lo << 31) | (hi >> 1);
        const bool valid = first + i >= pos;
        const bool acc = valid && rnd[i] < max_multiple;
        valid_mask |= (uint32_t)valid << i;
        acc_mask |= (uint32_t)acc << i;
        cnt += acc;
      }
      // exclusive prefix sum of cnt over the workgroup
      uint32_t incl = cnt;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (lane >= (uint32_t)d) incl += up;
      }
      if (lane == 63) s_wave[wave] = incl;
      if (t == 0) s_next = ~0ULL;
      __syncthreads();
      uint32_t before = 0, total = 0;
#pragma unroll
      for (uint32_t w = 0; w < kSeedThreads / 64; ++w) {
        const uint32_t c = s_wave[w];
        before += w < wave ? c : 0;
        total += c;
      }
      uint32_t run = written + before + (incl - cnt);   // accepted candidates of this modulus in front of h[0]
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (((valid_mask >> i) & 1) && run < N) {       // consumed by this modulus
          if ((acc_mask >> i) & 1) {
            dst[(size_t)j * N + run] = reduce64(rnd[i], mc);
            ++run;
            if (run == N) s_next = first + i + 1;
          } else {
            ++rejected;
          }
        }
      }
      __syncthreads();
      if (written + total >= N) {
        pos = s_next;
        written = N;
      } else {
        pos = (r0 + kChunkRefills) * kRefillWords;
        written += total;
      }
      __syncthreads();              // s_next and s_wave are rewritten by the next chunk
    }
  }
  if (rejected) atomicAdd(&s_rej, rejected);
  __syncthreads();
  if (t == 0) {
    if (s_rej) atomicAdd(&stats[0], (unsigned long long)s_rej);
    if (overrun) atomicExch(&stats[1], 1ULL);
  }
}

hipError_t launch_seed_expand(hipStream_t st, const SeedExpandArgs& args, const uint8_t* seeds, uint32_t n_obj, uint64_t* out,
                              uint64_t obj_stride, uint64_t* stats) {
  if (!n_obj) return hipSuccess;
  hipLaunchKernelGGL(seed_expand_kernel, dim3(n_obj), dim3(kSeedThreads), 0, st, args, seeds, out, obj_stride,
                     reinterpret_cast<unsigned long long*>(stats));
  return hipGetLastError();
}

}  // namespace pirgpu
