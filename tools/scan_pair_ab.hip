// scan_pair_ab -- the paired database pass (pir_amd/csrc/scan_mfma_pair.hip) alone: one launch_scan_mfma_pair against two
// launch_scan_mfma launches on the same database and selectors (hashed bytes, two 36-bit moduli, N = 4096), HIP events on
// one stream, outputs of the two forms compared word for word.  The source of profiles/scan_pair_ab.txt's first table.
// build (from the repository root):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -x hip pir_amd/csrc/scan_mfma.hip pir_amd/csrc/scan_mfma_pair.hip \
//         tools/scan_pair_ab.hip -o tools/scan_pair_ab
// usage: tools/scan_pair_ab rows cols top4 fp64_fold nq0 nq1 workgroups(0 = all CUs) reps
//   e.g. tools/scan_pair_ab 171 171 1 1 8 8 128 10     (cfg 3's 11 x 11 tiles; exit status 3 if the outputs differ)
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include "../pir_amd/csrc/kernels.h"

using namespace pirgpu;
typedef unsigned __int128 u128;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

// 16 bytes per thread of hashed bytes; top_lo/top_hi: byte range inside a TB block whose bytes are clamped to [-8, 7]
__global__ void fill_kernel(uint8_t* p, size_t n16, uint64_t seed, uint32_t TB, uint32_t top_lo) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n16) return;
  uint32_t w[4];
  for (int k = 0; k < 4; ++k) {
    uint64_t x = (i * 4 + k + 1) * 0x9E3779B97F4A7C15ull + seed;
    x ^= x >> 31; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 29; x *= 0x94D049BB133111EBull; x ^= x >> 32;
    w[k] = (uint32_t)x;
  }
  const uint32_t in_blk = (uint32_t)((i * 16) % TB);
  if (top_lo && in_blk >= top_lo)
    for (int k = 0; k < 4; ++k) { uint32_t v = w[k] & 0x0F0F0F0Fu; w[k] = v | (((v >> 3) & 0x01010101u) * 0xF0u); }
  reinterpret_cast<uint4*>(p)[i] = make_uint4(w[0], w[1], w[2], w[3]);
}

int main(int argc, char** argv) {
  if (argc < 9) { printf("usage: %s rows cols top4 fp64_fold nq0 nq1 workgroups reps\n", argv[0]); return 1; }
  const uint32_t rows = atoi(argv[1]), cols = atoi(argv[2]);
  const bool top4 = atoi(argv[3]) != 0, f64 = atoi(argv[4]) != 0;
  const uint32_t nq0 = atoi(argv[5]), nq1 = atoi(argv[6]), wgs = atoi(argv[7]);
  const int reps = atoi(argv[8]);
  const uint32_t N = 4096, logN = 12, k = 2, kN = k * N;
  static DevParams hp;
  memset(&hp, 0, sizeof(hp));
  hp.N = N; hp.logN = logN; hp.k = k;
  const uint64_t qs[2] = {68719403009ull, 68719230977ull};   // 36-bit primes (any odd 36-bit value would do here)
  for (uint32_t i = 0; i < k; ++i) {
    const uint64_t q = qs[i];
    hp.mod[i].q = q;
    // floor(2^128 / q)
    u128 hi = ((u128)1 << 64) / q, rem = ((u128)1 << 64) % q;
    u128 lo = (rem << 64) / q;
    hp.mod[i].br_hi = (uint64_t)hi; hp.mod[i].br_lo = (uint64_t)lo;
    hp.tab[i].qd = (double)q; hp.tab[i].qinvd = 1.0 / (double)q;
    uint64_t w = (1ull << 32) % q, acc = w;
    for (int e = 0; e < 3; ++e) {
      hp.fold_w[i][e] = acc > q / 2 ? -(double)(q - acc) : (double)acc;
      acc = (uint64_t)(((u128)acc * w) % q);
    }
  }
  MfmaGeom gm = mfma_geometry(hp, rows, cols, -1, top4);
  printf("geom L=%u RT=%u KG=%u KS=%u nchunks=%u NW=%u top4=%u db=%zu sel=%zu pair_supported=%d\n", gm.L, gm.RT, gm.KG, gm.KS,
         gm.nchunks, gm.NW, gm.top4, gm.db_bytes, gm.sel_bytes, (int)scan_mfma_pair_supported(gm));
  if (!scan_mfma_pair_supported(gm) || (gm.top4 != 0) != top4) { printf("unsupported\n"); return 1; }
  DevParams* dP; CK(hipMalloc(&dP, sizeof(hp))); CK(hipMemcpy(dP, &hp, sizeof(hp), hipMemcpyHostToDevice));
  uint8_t *db, *sel[2];
  CK(hipMalloc(&db, gm.db_bytes));
  const uint32_t top_lo = top4 ? 0 : (gm.L - 1) * 256;
  fill_kernel<<<(gm.db_bytes / 16 + 255) / 256, 256>>>(db, gm.db_bytes / 16, 1, gm.tile_bytes, top_lo);
  for (int s = 0; s < 2; ++s) {
    CK(hipMalloc(&sel[s], gm.sel_bytes));
    fill_kernel<<<(gm.sel_bytes / 16 + 255) / 256, 256>>>(sel[s], gm.sel_bytes / 16, 77 + s, gm.tile_bytes, top_lo);
  }
  const size_t qwords = (size_t)rows * 2 * kN;
  const uint32_t nq[2] = {nq0, nq1};
  uint64_t *outS[2], *outP[2];
  for (int s = 0; s < 2; ++s) {
    CK(hipMalloc(&outS[s], nq[s] * qwords * 8)); CK(hipMalloc(&outP[s], nq[s] * qwords * 8));
    CK(hipMemset(outS[s], 0xA5, nq[s] * qwords * 8)); CK(hipMemset(outP[s], 0x5A, nq[s] * qwords * 8));
  }
  CK(hipDeviceSynchronize());
  hipStream_t st; CK(hipStreamCreate(&st));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  ScanGroups gp{}; gp.n = 2;
  for (int s = 0; s < 2; ++s) { gp.sel[s] = sel[s]; gp.out[s] = outP[s]; gp.nq[s] = (uint8_t)nq[s]; }
  std::vector<float> tS, tP;
  for (int r = 0; r < reps + 1; ++r) {
    CK(hipEventRecord(e0, st));
    for (int s = 0; s < 2; ++s)
      CK(launch_scan_mfma(st, dP, gm, db, sel[s], outS[s], qwords, nq[s], rows, kN, 0, wgs, f64));
    CK(hipEventRecord(e1, st)); CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1)); if (r) tS.push_back(ms);
    CK(hipEventRecord(e0, st));
    CK(launch_scan_mfma_pair(st, dP, gm, db, gp, rows, 0, wgs, f64, 0, kN, qwords, kN, false));
    CK(hipEventRecord(e1, st)); CK(hipEventSynchronize(e1));
    CK(hipEventElapsedTime(&ms, e0, e1)); if (r) tP.push_back(ms);
  }
  CK(hipDeviceSynchronize());
  size_t bad = 0, nonzero = 0;
  for (int s = 0; s < 2; ++s) {
    std::vector<uint64_t> a(nq[s] * qwords), b(nq[s] * qwords);
    CK(hipMemcpy(a.data(), outS[s], a.size() * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(b.data(), outP[s], b.size() * 8, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < a.size(); ++i) { bad += a[i] != b[i]; nonzero += a[i] != 0 && a[i] != 0xA5A5A5A5A5A5A5A5ull; }
  }
  auto stat = [](std::vector<float>& v, float& mn, float& mean) { mn = 1e9; mean = 0; for (float x : v) { mn = std::min(mn, x); mean += x; } mean /= v.size(); };
  float mnS, meS, mnP, meP; stat(tS, mnS, meS); stat(tP, mnP, meP);
  printf("RESULT rows=%u cols=%u top4=%d f64=%d nq=%u+%u wgs=%u  two_singles_us min=%.1f mean=%.1f  pair_us min=%.1f mean=%.1f  ratio_min=%.3f ratio_mean=%.3f  mismatches=%zu nontrivial=%zu\n",
         rows, cols, (int)top4, (int)f64, nq0, nq1, wgs, mnS * 1e3, meS * 1e3, mnP * 1e3, meP * 1e3, mnP / mnS, meP / meS, bad, nonzero);
  return bad ? 3 : 0;
}
