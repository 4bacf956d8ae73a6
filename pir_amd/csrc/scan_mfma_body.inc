// scan_mfma_body.inc -- the body of scan_mfma_kernel (scan_mfma.hip), included once per kernel that shares it.
// PIRGPU_SCAN_DB_OF(g) names the operand layout group g scans: `dbp` for every group (scan_mfma_kernel: the tokens the
// compiler sees are the ones it saw before this file existed), or grp.db[g] (scan_mfma_runs_kernel: a table per group,
// read from the by-value kernel argument with a workgroup-uniform index -- scalar loads, never a divergent one; past the
// last unit the next unit names no group, so the current one is named and nothing is loaded from it).
// scan_mfma_pair.hip holds a hand copy of the loaders, the fold and the result staging below (its kernel serves two groups
// per unit and must not change what the kernels here compile to): a fix to any of them belongs in both places.
  constexpr uint32_t TB = tile_bytes(L, TOP4);
  constexpr int LF = TOP4 ? L - 1 : L;   // digits stored as full bytes
  constexpr int NS = 2 * L - 1;        // digit diagonals
  constexpr int NG = (NS + 4) / 5;     // groups of five diagonals (40 bits)
  // results of one row tile, [row][x][slot]: a (row, x) run is padded to 9 words so that the 16 lanes of a row (x = 0..15,
  // 72 bytes apart) hit 16 different 8-byte bank pairs when a wave stores its slot (64 bytes apart they hit two)
  // kDirect (-DPIRGPU_SCAN_DIRECT=1): no staging and no workgroup barrier -- every lane stores its four values itself
  // (8 bytes each; the eight waves' stores to a (row, x) run of eight slots merge in L2) and the waves run decoupled.
  constexpr bool kDirect = PIRGPU_SCAN_DIRECT != 0;
  __shared__ __attribute__((aligned(16))) uint64_t stage[kDirect ? 1 : 2][kDirect ? 1 : 16][kDirect ? 1 : 16][NW + PIRGPU_SCAN_PAD];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  const int g = l >> 4, i16 = l & 15;
  constexpr int LOGNW = NW == 8 ? 3 : 2;
  const uint32_t nblocks = nslots >> LOGNW;
  const uint32_t nunits = nblocks * grp.n;
  uint32_t ch = 0;
  while (ch + 1 < plan.nchunks && blockIdx.x >= plan.first[ch + 1]) ++ch;
  const uint32_t wg_in_chunk = blockIdx.x - plan.first[ch], wgs_in_chunk = plan.first[ch + 1] - plan.first[ch];
  const uint32_t kg0 = ch * GC;                                   // GC <= 4 KS column groups per chunk
  const uint32_t gc = KG - kg0 < GC ? KG - kg0 : GC;              // column groups of this chunk
  const size_t slab = (size_t)RT * KG * TB;                       // database bytes of one slot
  const size_t chunk_base = (size_t)RT * kg0 * TB;                // this chunk inside a slot
  const size_t rt_stride = (size_t)gc * TB;
  const uint32_t lane16 = i16 * 16, lane8 = i16 * 8;              // the lane's bytes inside a full / a nibble tile

  v4i B[KS][L], A[KS][LF];
  v2i A4[KS];                           // TOP4: the top digit's tiles, packed
  // selector tiles of (local) slot jl of group gi
  auto load_B = [&](uint32_t gi, uint32_t jl) {
    const uint8_t* selp = grp.sel[gi];
    const uint32_t nx = 2u * grp.nq[gi];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const uint32_t gl = ks * 4 + g, kg = kg0 + gl;
      const uint8_t* blk = selp + ((size_t)jl * KG + kg) * TB;
#pragma unroll
      for (int b = 0; b < L; ++b) {
        B[ks][b] = v4i{0, 0, 0, 0};   // columns beyond the group's queries stay zero and are neither packed nor read
        if (gl < gc && (uint32_t)i16 < nx) {
          if (TOP4 && b == L - 1) B[ks][b] = expand_top4(*reinterpret_cast<const v2i*>(blk + b * 256 + lane8));
          else B[ks][b] = *reinterpret_cast<const v4i*>(blk + b * 256 + lane16);
        }
      }
    }
  };
  // the L tiles of column group gl (inside the chunk) of one row tile, from `base` = that row tile's first byte
  auto load_A = [&](int ks, const uint8_t* base, uint32_t gl) {
    const uint8_t* blk = base + (size_t)gl * TB;
#pragma unroll
    for (int a = 0; a < LF; ++a) A[ks][a] = load_tile(blk + a * 256 + lane16);
    if constexpr (TOP4) A4[ks] = load_tile8(blk + (L - 1) * 256 + lane8);
  };

  // unit -> (group, slot block): group-major (u = group * nblocks + block: the launch sweeps the slots once per group) or
  // block-major (u = block * groups + group: the workgroups running side by side read the SAME database tiles for
  // different groups, so all but the first reader of a tile can be served by the memory-side cache)
  // (plain scalar arithmetic at each use: a helper taking references made the compiler keep the pair in scratch)
#define PIRGPU_UNIT_OF(uu, gi_, blk_)                                  \
  const uint32_t gi_ = blk_major ? (uu) % grp.n : (uu) / nblocks;      \
  const uint32_t blk_ = blk_major ? (uu) / grp.n : (uu) - gi_ * nblocks;
  uint32_t u = wg_in_chunk;
  if (u >= nunits) return;
  {
    PIRGPU_UNIT_OF(u, gi, blk)
    load_B(gi, blk * NW + w);
    const uint8_t* abase = PIRGPU_SCAN_DB_OF(gi) + (size_t)(blk * NW + w) * slab + chunk_base;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const uint32_t gl = ks * 4 + g;   // column group inside the chunk
#pragma unroll
      for (int a = 0; a < LF; ++a) A[ks][a] = v4i{0, 0, 0, 0};
      A4[ks] = v2i{0, 0};
      if (gl < gc) load_A(ks, abase, gl);
    }
  }

  uint32_t parity = 0;
  for (; u < nunits; u += wgs_in_chunk) {
    PIRGPU_UNIT_OF(u, gi, blk)
    const uint32_t j0 = blk * NW;            // local slot of wave 0
    const uint32_t j = slot0 + j0 + w;       // this wave's slot of the ring
    const uint32_t mi = j >> P->logN;
    const ModConst m = P->mod[mi];
    const uint32_t nx = 2u * grp.nq[gi];
    uint64_t* const obase = grp.out[gi] + ch * chunk_stride;
    // multiple of q that makes every 40-bit group positive: 2^58 <= bias < 2^59, |group| < 2^57.2 (kBiasBits)
    const uint64_t bias = m.q << (kBiasBits - (64 - __builtin_clzll(m.q)));
    [[maybe_unused]] const F64Mod fm{P->tab[mi].qd, P->tab[mi].qinvd};
    [[maybe_unused]] const double fw0 = P->fold_w[mi][0], fw1 = P->fold_w[mi][1], fw2 = P->fold_w[mi][2];
    const uint8_t* abase = PIRGPU_SCAN_DB_OF(gi) + (size_t)(j0 + w) * slab + chunk_base;
    const uint32_t nu = u + wgs_in_chunk;
    const bool has_next = nu < nunits;
    PIRGPU_UNIT_OF(nu, ngi, nblk)
    const uint8_t* nbase = PIRGPU_SCAN_DB_OF(has_next ? ngi : gi) + (size_t)(nblk * NW + w) * slab + chunk_base;

    for (uint32_t rt = 0; rt < RT; ++rt) {
      v4i T[NS];
#pragma unroll
      for (int s = 0; s < NS; ++s) T[s] = v4i{0, 0, 0, 0};
      const bool last = rt + 1 == RT;   // wave-uniform
      // ring of KS k-steps of A tiles: slot ks is refilled right after use with the same step of the next
      // row tile (or of the next unit's first row tile)
      const uint8_t* next_tile = last ? nbase : abase + (size_t)(rt + 1) * rt_stride;
      const bool refill = !last || has_next;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        [[maybe_unused]] v4i Atop;
        if constexpr (TOP4) Atop = expand_top4(A4[ks]);
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
        const uint32_t gl = ks * 4 + g;
        if (refill && gl < gc) load_A(ks, next_tile, gl);
      }
      if (last && has_next) load_B(ngi, nblk * NW + w);   // all MFMAs of this unit are issued: B is free
      // lane (g, i16) holds rows rt*16 + g*4 + i (i < 4) of column x = i16:  value = sum_s T[s] 2^(8 s)
      const int buf = parity;
      parity ^= 1;
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
              r = (uint64_t)(G + (int64_t)bias);   // top group: < 2^59.4, reduced together with the next one (bias = 0 mod q)
            } else {
              const u128 v = ((u128)r << 40) + (uint64_t)(G + (int64_t)bias);
              r = reduce128((uint64_t)v, (uint64_t)(v >> 64), m);
            }
          }
        }
        if constexpr (kDirect) {
          const uint32_t row = rt * 16 + g * 4 + i;
          if ((uint32_t)i16 < nx && row < rows)
            obase[(size_t)(i16 >> 1) * out_qstride + ((size_t)row * 2 + (i16 & 1)) * out_rstride + j0 + w] = r;
        } else {
          stage[buf][g * 4 + i][i16][w] = r;
        }
      }
      if constexpr (kDirect) continue;
      __syncthreads();
      // 256 (row, x) runs of NW slots = 8 NW bytes each; 64 NW threads x 16 B, two rounds
#pragma unroll
      for (int round = 0; round < 2; ++round) {
        const int run = round * 128 + (threadIdx.x >> (LOGNW - 1));
        const int part = threadIdx.x & (NW / 2 - 1);
        const int r16 = run >> 4, x = run & 15;
        const uint32_t r = rt * 16 + r16;
        if (x < (int)nx && r < rows) {
          typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
#if PIRGPU_SCAN_PAD == 2
          const u64x2 v = *reinterpret_cast<const u64x2*>(&stage[buf][r16][x][part * 2]);     // runs 80 bytes apart: one 16-byte read
#else
          const u64x2 v = {stage[buf][r16][x][part * 2], stage[buf][r16][x][part * 2 + 1]};   // two 8-byte LDS reads
#endif
          uint64_t* dst = obase + (size_t)(x >> 1) * out_qstride + ((size_t)r * 2 + (x & 1)) * out_rstride + j0 + part * 2;
          *reinterpret_cast<u64x2*>(dst) = v;
        }
      }
    }
  }
#undef PIRGPU_UNIT_OF
