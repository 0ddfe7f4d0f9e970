// K4x, the exact search on the matrix cores: the fp4 expansion, the 32 x 32 accumulator blocks and their tests (whole and split),
// the 32-row step, hamming_topk_mfma and its <= 32-query form hamming_topk_mfma_q32. TOD_K4X_ABLATE / TOD_K4X_COUNT_WALKS are
// diagnostics builds (tools/k4x_ablate.sh, tools/k4x_walks.sh). The radius bound restates DescriptorMatcher.cpp:212-220.
// Included by match.hip inside its anonymous namespace, after match_keys.h.
//
// K4x  hamming_topk_mfma   the same exact search on the matrix cores. With every descriptor bit b written as the
//                          MX-fp4 (E2M1) value 1 - 2b, the dot product of two descriptors is 256 - 2 * hamming: products
//                          are +-1, the f32 accumulator holds integers <= 256, so the result is EXACT.
//                          v_mfma_f32_32x32x64_f8f6f4 (fp4 x fp4, unit scales) takes 64 bit positions of 32 DB rows x 32
//                          queries per issue: 4 MFMAs = 1024 complete distances in 128 matrix-pipe cycles (8 pairs per
//                          clock and SIMD; the VALU form above peaks at 1, or ~2 when its elimination fires) and the
//                          rate does not depend on the data.
//                          One WAVE = (DB tile, 32 QT queries). The query fragments stay in registers (16 VGPRs per
//                          32 queries); every lane loads 16 packed bytes of one DB row per 32-row step (a wave load = 32
//                          rows = 1 KB contiguous, served by L2: all query waves of a tile read the same lines), expands
//                          them to fp4 with 7 VALU ops per 32 bits, no LDS, no barrier. A and B use the same
//                          (lane, register, nibble) -> bit assignment, so the sum runs over matching bit positions whatever
//                          the hardware's internal k order is.
//                          Accumulator layout (dtype independent): lane = query column (l & 31), 16 registers = 16 DB
//                          rows (i & 3) + 8 (i >> 2) + 4 (l >> 5). A lane keeps its k best keys in registers exactly as
//                          K4 does; the test per 32 x 32 block is max over the 16 registers > threshold (8 v_max3 + 1
//                          compare, in the shadow of the next block's MFMAs) and only a block with a hit walks its registers.
//                          Bounds are exchanged between tiles through the same per-query word as K4 (loaded one period
//                          ahead, so the latency of the load is never waited for). Output = K4's partial-key layout.
typedef int mfma_i32x8 __attribute__((ext_vector_type(8)));
typedef float mfma_f32x16 __attribute__((ext_vector_type(16)));

// 32 descriptor bits -> 32 fp4 values (4 dwords): nibble i of out[j] = 0x2 | (bit (4 i + j) << 3)  (+1.0 / -1.0 in E2M1).
// The two constants live in registers (gfx9 VOP3 takes no literal), so each dword is one shift + one v_and_or_b32.
struct Fp4Consts { uint32_t sign, one; };
__device__ __forceinline__ Fp4Consts fp4_consts() {
  Fp4Consts k;
  asm volatile("s_mov_b32 %0, 0x88888888" : "=s"(k.sign));
  asm volatile("v_mov_b32 %0, 0x22222222" : "=v"(k.one));
  return k;
}
__device__ __forceinline__ mfma_i32x8 expand_word(uint32_t x, const Fp4Consts& k) {
  const int a = (int)(((x << 3) & k.sign) | k.one), b = (int)(((x << 2) & k.sign) | k.one),
            c = (int)(((x << 1) & k.sign) | k.one), d = (int)((x & k.sign) | k.one);
  return mfma_i32x8{a, b, c, d, 0, 0, 0, 0};
}

struct Fp4Row { mfma_i32x8 s[4]; };   // the lane's 128 bits of one row: 4 MFMA steps x 4 dwords (upper halves unused by fp4)

__device__ __forceinline__ void expand_row(const uint4& p, Fp4Row& f, const Fp4Consts& k) {
  f.s[0] = expand_word(p.x, k); f.s[1] = expand_word(p.y, k); f.s[2] = expand_word(p.z, k); f.s[3] = expand_word(p.w, k);
}

__device__ __forceinline__ float thr_of_limit(uint32_t limit) { return 256.f - 2.f * (float)limit; }   // dot > thr <=> d < limit

// 256 bit positions of 32 DB rows (A) x 32 queries (B): acc[i] of lane l = dot(row (i & 3) + 8 (i >> 2) + 4 (l >> 5), query l & 31)
__device__ __forceinline__ mfma_f32x16 dot_block(const Fp4Row& a, const Fp4Row& b) {
  mfma_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a.s[s], b.s[s], acc, 4, 4, 0, 0, 0, 0);
  return acc;
}

// The test of one accumulator block: nothing to do unless some lane's best dot product beats its threshold (rare: the
// thresholds follow the k-th best distance found so far, anywhere in the DB); then walk the block's 16 rows. MASK: rows at
// or beyond n_lim do not exist (the last, partial step of the DB). IMAX: thresholds are >= 0 (radius < 128; they only rise),
// so the 16-way maximum may be taken on the raw bits as integers -- among non-negative floats the order is the same, and a
// negative dot product can never beat a non-negative threshold -- which spares the float maximum's NaN-quieting moves.
#ifdef TOD_K4X_COUNT_WALKS                                   // diagnostics build only (tools/k4x_walks.sh): blocks tested / blocks that walked
__device__ unsigned long long g_k4x_blocks[2];
#endif
template <int K, bool MASK, bool IMAX>
__device__ __forceinline__ void mfma_block_test(const mfma_f32x16& acc, float& thr, uint32_t r_lane, uint32_t n_lim,
                                                uint32_t (&best)[K]) {
#ifdef TOD_K4X_COUNT_WALKS
  if (!MASK && (threadIdx.x & 63u) == 0u) atomicAdd(&g_k4x_blocks[0], 1ull);
#endif
  if (!MASK) {
    bool any;
    if (IMAX) {                                            // (a tree: see mfma_block_test_part)
      int g[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) g[j] = max(max(__float_as_int(acc[3 * j]), __float_as_int(acc[3 * j + 1])), __float_as_int(acc[3 * j + 2]));
      const int m = max(max(max(g[0], g[1]), g[2]), max(max(g[3], g[4]), __float_as_int(acc[15])));
      any = m > __float_as_int(thr);
    } else {
      float m = fmaxf(fmaxf(acc[0], acc[1]), acc[2]);
#pragma unroll
      for (int i = 3; i < 15; i += 2) m = fmaxf(fmaxf(m, acc[i]), acc[i + 1]);
      m = fmaxf(m, acc[15]);
      any = m > thr;
    }
    if (__builtin_amdgcn_ballot_w64(any) == 0ull) return;
#ifdef TOD_K4X_COUNT_WALKS
    if ((threadIdx.x & 63u) == 0u) atomicAdd(&g_k4x_blocks[1], 1ull);
#endif
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    // the block's row i = r_lane | ((i & 3) + 8 (i >> 2)): r_lane = 32 step + 4 (lane >> 5) leaves bits 0, 1, 3, 4 free
    const uint32_t ri = (uint32_t)((i & 3) + 8 * (i >> 2));
    const bool hit = MASK ? (acc[i] > thr && (r_lane | ri) < n_lim) : (acc[i] > thr);
    if (__builtin_amdgcn_ballot_w64(hit) != 0ull) {
      // key = distance << 22 | row: (256 - dot) * 2^21 is an exact integer below 2^31. A stale (looser) threshold only
      // lets more rows try: the list keeps its k smallest keys whatever is offered
      const uint32_t key = (uint32_t)((256.f - acc[i]) * 2097152.f) | r_lane | ri;
      topk_insert<K>(best, hit ? key : 0xFFFFFFFFu);
    }
  }
  thr = fmaxf(thr, thr_of_limit(best[K - 1] >> kLocalBits));       // thresholds only ever tighten
}

// The same in two parts: the first SPLIT (2 or 3) of the block's 4 MFMAs, the rest behind a test (mfma_block_test_part)
template <int SPLIT>
__device__ __forceinline__ mfma_f32x16 dot_part0(const Fp4Row& a, const Fp4Row& b) {
  mfma_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < SPLIT; ++s) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a.s[s], b.s[s], acc, 4, 4, 0, 0, 0, 0);
  return acc;
}
// Partial-distance elimination on the matrix cores (K4's idea, a block at a time): after P = 64 SPLIT of the 256 bit positions the
// accumulator holds P - 2 dP with dP <= d, so a pair whose partial dot product is not above thr - (256 - P) (dP >= limit) cannot
// be a hit whatever the other positions say -- exact for any data. On independent bits d128 of a non-match is 64 +- 5.7 and
// the radius 35: one block in five thousand goes on to its other two MFMAs (SPLIT 2). Real rBRIEF bits are biased and correlated
// (mean distance ~100 of 256 on this library's ORB descriptors of rendered views): there almost every block survives 128 positions
// and SPLIT 3 is the form that prunes (d192 ~ 75 +- 9.5). Needs thr - (256 - P) >= 0 for the integer maximum (limits up to 64 for
// SPLIT 2, up to 96 for SPLIT 3; thresholds only tighten). rows / q: the fragments the block's first part was computed from.
template <int K, int SPLIT>
__device__ __forceinline__ bool mfma_block_test_part(mfma_f32x16& acc, const Fp4Row& rows, const Fp4Row& q, float& thr, float& thrp,
                                                     uint32_t r_lane, uint32_t n_lim, uint32_t (&best)[K]) {
  // the 16-way maximum as a tree (5 independent max3, then 2 + 1): in this form the kernel is bound by vector issue, not by the matrix
  // pipe (tools/mfma_valu_overlap.hip: 2 MFMAs + chain + expansion 113 cycles per block and SIMD, + tree 103), and the tree's
  // independent operations fill the issue slots a chain leaves to its own latency. The part thresholds (thrp = thr - 64 (4 - SPLIT))
  // live in registers of their own beside the whole ones: one instruction less per block (1.82 -> 1.73 ms in the pipeline) for six
  // registers, 218 -> 224, still inside the budget that lets the other stages' kernels start beside the matcher's waves
  // (launch_topk_mfma; tests/test_build_checks.py holds the line). Keeping ONLY the part form -- no extra registers on paper -- made
  // hipcc allocate 243.
  int g[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) g[j] = max(max(__float_as_int(acc[3 * j]), __float_as_int(acc[3 * j + 1])), __float_as_int(acc[3 * j + 2]));
  const int m = max(max(max(g[0], g[1]), g[2]), max(max(g[3], g[4]), __float_as_int(acc[15])));
  if (__builtin_amdgcn_ballot_w64(m > __float_as_int(thrp)) == 0ull) return false;
#pragma unroll
  for (int s = SPLIT; s < 4; ++s) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(rows.s[s], q.s[s], acc, 4, 4, 0, 0, 0, 0);
  mfma_block_test<K, false, true>(acc, thr, r_lane, n_lim, best);
  thrp = thr - 64.f * (float)(4 - SPLIT);
  return true;
}

// One 32-row step: QT x 4 MFMAs against the resident query fragments. The test of block t-1 (and, in the first four
// blocks, the fp4 expansion of the NEXT step's packed rows) sits in the same basic block as the MFMAs of block t, so the
// vector ALU works in the matrix pipe's shadow; the last block's test is carried into the next step: QT is even, so it
// waits in acc_odd while block 0 of the next step fills acc_even.
// SPLIT 2 / 3 (never with MASK; 0 = whole blocks): every block starts with its first SPLIT MFMAs (dot_part0) and only completes
// behind mfma_block_test_part; the block carried in from the previous step (t == 0) completes with that step's rows, which are
// a_next's registers 2 and 3 until this step's expansion overwrites them at t == 2, 3.
template <int K, int QT, bool MASK, bool IMAX, int SPLIT = 0>
__device__ __forceinline__ uint32_t mfma_step(const Fp4Row& a, Fp4Row& a_next, const uint4& p_next, const Fp4Row (&qb)[QT],
                                              float (&thr)[QT], float (&thrp)[QT], uint32_t (&best)[QT][K], mfma_f32x16& acc_even,
                                              mfma_f32x16& acc_odd, uint32_t r_lane, uint32_t n_lim, const Fp4Consts& kc) {
  constexpr bool HALF = SPLIT != 0;
  uint32_t n_pass = 0;                                     // SPLIT: blocks that went on to their second part (wave-uniform)
  static_assert(!(HALF && MASK) && !(HALF && !IMAX) && !(HALF && QT < 4), "split blocks: unmasked steps, integer maximum, >= 4 query blocks");
  static_assert(SPLIT == 0 || SPLIT == 2 || SPLIT == 3, "2 or 3 of the 4 MFMAs first");
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    if (HALF) { if (t & 1) acc_odd = dot_part0<HALF ? SPLIT : 2>(a, qb[t]); else acc_even = dot_part0<HALF ? SPLIT : 2>(a, qb[t]); }
    else { if (t & 1) acc_odd = dot_block(a, qb[t]); else acc_even = dot_block(a, qb[t]); }
#if defined(TOD_K4X_ABLATE) && TOD_K4X_ABLATE == 3           // diagnostics build only: no fp4 expansion (the packed words are "used")
    if (t == 0) { a_next = a; asm volatile("" :: "v"(p_next.x), "v"(p_next.y), "v"(p_next.z), "v"(p_next.w)); }
#else
    if (QT >= 4) {
      if (t == 0) a_next.s[0] = expand_word(p_next.x, kc);
      if (t == 1) a_next.s[1] = expand_word(p_next.y, kc);
      if (t == 2) a_next.s[2] = expand_word(p_next.z, kc);
      if (t == 3) a_next.s[3] = expand_word(p_next.w, kc);
    } else {                                             // two blocks per step: two words each
      if (t == 0) { a_next.s[0] = expand_word(p_next.x, kc); a_next.s[1] = expand_word(p_next.y, kc); }
      if (t == 1) { a_next.s[2] = expand_word(p_next.z, kc); a_next.s[3] = expand_word(p_next.w, kc); }
    }
#endif
#if defined(TOD_K4X_ABLATE) && TOD_K4X_ABLATE == 2           // diagnostics build only: no block test (the MFMAs stay: their results are "used")
    if (t == 0) asm volatile("" :: "v"(acc_odd)); else if (t & 1) asm volatile("" :: "v"(acc_even)); else asm volatile("" :: "v"(acc_odd));
#else
    if (HALF) {
      if (t == 0) n_pass += mfma_block_test_part<K, HALF ? SPLIT : 2>(acc_odd, a_next, qb[QT - 1], thr[QT - 1], thrp[QT - 1], r_lane - 32u, n_lim, best[QT - 1]) ? 1u : 0u;   // previous step's last block, its rows
      else n_pass += mfma_block_test_part<K, HALF ? SPLIT : 2>((t & 1) ? acc_even : acc_odd, a, qb[t - 1], thr[t - 1], thrp[t - 1], r_lane, n_lim, best[t - 1]) ? 1u : 0u;
    } else {
      if (t == 0) mfma_block_test<K, MASK, IMAX>(acc_odd, thr[QT - 1], r_lane - 32u, n_lim, best[QT - 1]);   // previous step's last block
      else mfma_block_test<K, MASK, IMAX>((t & 1) ? acc_even : acc_odd, thr[t - 1], r_lane, n_lim, best[t - 1]);
    }
#endif
  }
  return n_pass;
}

// MODE 0: float maximum in the block test (any radius); 1: integer maximum (cut <= 128: thresholds >= 0); 2 / 3: integer maximum and
// blocks split after 2 / 3 of their 4 MFMAs (cut <= 64 / <= 96: mfma_block_test_part)
template <int K, int QT, int MODE, bool PF2>
__global__ __launch_bounds__(kBlock, 2) void hamming_topk_mfma(const uint32_t* __restrict__ db,
                                                               const uint32_t* __restrict__ q, uint32_t n_rows,
                                                               uint32_t nq, uint32_t nq_pad, uint32_t rows_per_tile,
                                                               uint32_t n_tiles, uint32_t n_qw, uint32_t n_qw64,
                                                               uint32_t blocks_per_xcd, uint32_t tiles_per_xcd, uint32_t cut,
                                                               uint32_t share_period,
                                                               uint32_t* __restrict__ part, uint32_t* bound,
                                                               uint8_t* __restrict__ stored, uint32_t* half_stats) {
  static_assert(QT % 2 == 0 && QT >= 2, "two query blocks share a 64-query flag byte");
  constexpr bool IMAX = MODE >= 1;
  constexpr int HALF = (MODE >= 2 && QT >= 4) ? MODE : 0;           // the split (0: whole blocks)
  constexpr float kPartOff = HALF ? 64.f * (float)(4 - HALF) : 0.f;   // what the positions behind the split can still add to a dot product
  const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3;
  uint32_t tile, qw;
  if (tiles_per_xcd) {
    const uint32_t local = __builtin_amdgcn_readfirstlane(slot * kWavesPerBlock + (threadIdx.x >> 6));
    if (local >= tiles_per_xcd * n_qw) return;
    tile = xcd * tiles_per_xcd + local / n_qw; qw = local % n_qw;
  } else {
    const uint32_t vblock = xcd * blocks_per_xcd + slot;
    const uint32_t item = __builtin_amdgcn_readfirstlane(vblock * kWavesPerBlock + (threadIdx.x >> 6));
    tile = item / n_qw; qw = item % n_qw;
  }
  if (tile >= n_tiles) return;
  const uint32_t lane = threadIdx.x & 63u, c = lane & 31u, h = lane >> 5;
  const uint32_t q0 = qw * (32u * QT);

  const Fp4Consts kc = fp4_consts();
  // query blocks beyond nq repeat the last query: their results are never stored
  Fp4Row qb[QT];
  uint32_t best[QT][K];
  float thr[QT], thrp[QT];                                         // thrp: the part thresholds of the split blocks (mfma_block_test_part)
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const uint32_t qi = q0 + 32u * t + c;
    const uint4 p = *reinterpret_cast<const uint4*>(q + (size_t)(qi < nq ? qi : nq - 1u) * kWords + 4u * h);
    expand_row(p, qb[t], kc);
#pragma unroll
    for (int j = 0; j < K; ++j) best[t][j] = 0xFFFFFFFFu;
    // cut = radius + 1: a row beyond the radius is dropped by the truncation (DescriptorMatcher.cpp:212-220) whatever its rank
    thr[t] = thr_of_limit(cut);
    thrp[t] = thr[t] - kPartOff;
  }

  const uint32_t row0 = tile * rows_per_tile;
  const uint32_t row_end = min(n_rows, row0 + rows_per_tile);
  const uint32_t n_local = row_end - row0;                          // > 0: tile < n_tiles
  const uint32_t n_full = n_local / 32u, n_steps = (n_local + 31u) / 32u;   // the DB's last step may be partial
  // this lane's 16 bytes of DB row (row0 + 32 step + c). No per-lane clamp: the DB's last step may reach up to 31 rows past its end
  // -- into the slack todhip_db_load leaves behind the descriptors (kDbSlackBytes), rows that are masked, never used -- and the
  // address stays a wave-uniform base plus a constant lane offset (no vector instruction per load: the kernel is bound by those)
  const uint32_t lane_off = (c * kWords + 4u * h) * 4u;              // bytes from the step's first row
  auto load_step = [&](uint32_t step) -> uint4 {
    const uint32_t first = row0 + 32u * min(step, n_steps - 1u);    // wave-uniform
#if defined(TOD_K4X_ABLATE) && TOD_K4X_ABLATE == 1           // diagnostics build only (tools/k4x_ablate.sh): no DB loads
    const uint32_t r = first + c;
    return uint4{r * 2654435761u, r ^ step, r + h, r * 40503u};
#else
    const char* base = reinterpret_cast<const char*>(db) + (size_t)first * (kWords * 4u);
    return *reinterpret_cast<const uint4*>(base + lane_off);
#endif
  };
  Fp4Row a0, a1;
  {
    const uint4 p = load_step(0);
    expand_row(p, a0, kc);
  }
  // packed rows in flight: of steps + 1 and + 2 (PF2), or of step + 1 only (4 registers less: what lets QT = 8 fit)
  uint4 pa = load_step(1), pb = PF2 ? load_step(2) : pa;
  mfma_f32x16 acc_even, acc_odd;                                    // acc_odd: pending block of the previous step -- none yet
#pragma unroll
  for (int i = 0; i < 16; ++i) acc_odd[i] = -4096.f;                      // below every threshold (256 - 2 * 1023 at the least)
  uint32_t seen[QT];
#pragma unroll
  for (int t = 0; t < QT; ++t) seen[t] = 0xFFFFFFFFu;              // "nothing published"
  uint32_t next_share = 2u;                                         // first exchange after 64 rows, as K4

  uint32_t step = 0;
  // HALF: every block of the unmasked steps starts as a half; the wave counts the blocks that went on to their second half, and
  // the HOST decides from the launch's totals whether the next launches use this mode at all (launch_topk_mfma_qt: on self-similar
  // texture most blocks go on and the half test only adds work). An in-kernel switch between the two loop bodies was tried: 79
  // spilled registers at the 256 this kernel lives on, 2.1 ms instead of 1.64.
  uint32_t n_pass = 0;
  for (; step + 2u <= n_full; step += 2u) {
    // two steps per trip: the expanded rows ping-pong between a0 and a1, the packed ones between pa and pb
    n_pass += mfma_step<K, QT, false, IMAX, HALF>(a0, a1, pa, qb, thr, thrp, best, acc_even, acc_odd, 32u * step + 4u * h, n_local, kc);
    if (PF2) {
      pa = load_step(step + 3u);
      n_pass += mfma_step<K, QT, false, IMAX, HALF>(a1, a0, pb, qb, thr, thrp, best, acc_even, acc_odd, 32u * step + 32u + 4u * h, n_local, kc);
      pb = load_step(step + 4u);
    } else {
      pa = load_step(step + 2u);
      n_pass += mfma_step<K, QT, false, IMAX, HALF>(a1, a0, pa, qb, thr, thrp, best, acc_even, acc_odd, 32u * step + 32u + 4u * h, n_local, kc);
      pa = load_step(step + 3u);
    }
    if (step + 2u >= next_share) {                                  // wave-uniform
      next_share += share_period;
      // take the bounds loaded one period ago (a published bound stays valid: bounds only fall), publish a full list's
      // bound if it improves on what was seen, start the loads of the next period
#pragma unroll
      for (int t = 0; t < QT; ++t) {
        const uint32_t qi = q0 + 32u * t + c;
        uint32_t* my_bound = bound + (qi < nq ? qi : nq - 1u);
        const uint32_t worst_d = best[t][K - 1] >> kLocalBits;
        if (worst_d < (0xFFFFFFFFu >> kLocalBits) && worst_d < seen[t]) atomicMin(my_bound, worst_d);
        // a foreign bound is applied with <=: a smaller row index elsewhere may still win a tie
        if (seen[t] != 0xFFFFFFFFu) { thr[t] = fmaxf(thr[t], thr_of_limit(seen[t] + 1u)); thrp[t] = thr[t] - kPartOff; }
        seen[t] = __hip_atomic_load(my_bound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  // the last unmasked step's last block is still a half: it completes here, with that step's rows (a1: the second step of the
  // loop's last trip ran on them) -- the masked steps and the drain below work on whole blocks
  if (HALF && step > 0u) {
    n_pass += mfma_block_test_part<K, HALF ? HALF : 2>(acc_odd, a1, qb[QT - 1], thr[QT - 1], thrp[QT - 1], 32u * (step - 1u) + 4u * h, n_local, best[QT - 1]) ? 1u : 0u;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc_odd[i] = -4096.f;
    if (lane == 0 && half_stats) { atomicAdd(half_stats, n_pass); atomicAdd(half_stats + 1, step * (uint32_t)QT); }
  }
  // at most one full and one partial step are left: the masked form serves both
  for (; step < n_steps; ++step) {
    mfma_step<K, QT, true, IMAX>(a0, a1, pa, qb, thr, thrp, best, acc_even, acc_odd, 32u * step + 4u * h, n_local, kc);
    a0 = a1;
    pa = PF2 ? pb : load_step(step + 2u);
  }
  mfma_block_test<K, true, IMAX>(acc_odd, thr[QT - 1], 32u * (n_steps - 1u) + 4u * h, n_local, best[QT - 1]);   // drain

  // lanes l and l + 32 hold the two halves of a query's rows: merge the partner's list, then K4's output format
  // (partial keys + one flag byte per (tile, 64 queries); two query blocks share a flag, so both are stored when
  // either kept something)
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    uint32_t other[K];
#pragma unroll
    for (int j = 0; j < K; ++j) other[j] = __shfl_xor(best[t][j], 32);
#pragma unroll
    for (int j = 0; j < K; ++j) topk_insert<K>(best[t], other[j]);
  }
#pragma unroll
  for (int u = 0; u < QT / 2; ++u) {
    const uint32_t qa = q0 + 64u * u + c, qb2 = qa + 32u;
    const bool any_a = qa < nq && best[2 * u][0] != 0xFFFFFFFFu, any_b = qb2 < nq && best[2 * u + 1][0] != 0xFFFFFFFFu;
    if (__builtin_amdgcn_ballot_w64(any_a || any_b) != 0ull) {
      if (h == 0u) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
          if (qa < nq) part[((size_t)tile * K + j) * nq_pad + qa] = best[2 * u][j];
          if (qb2 < nq) part[((size_t)tile * K + j) * nq_pad + qb2] = best[2 * u + 1][j];
        }
      }
      if (lane == 0) stored[(size_t)tile * n_qw64 + (q0 >> 6) + u] = 0;
    }
  }
}

// K4x for at most 32 queries: ONE query block per wave, so a 32-row step (1 KB of the DB) costs 4 MFMAs -- the matrix pipe
// could take 16 TB/s of rows at that rate, and the pass is bound by HBM alone (BASELINE.json's "achieved HBM GB/s on
// BF-matcher"; tools/k4_small_q.py). Same exact arithmetic, same per-lane lists, same output format as hamming_topk_mfma; the
// accumulators of consecutive steps alternate so that the test of step s runs beside the MFMAs of step s + 1, and four
// steps' packed rows are in flight per wave.
template <int K, bool IMAX>
__global__ __launch_bounds__(kBlock) void hamming_topk_mfma_q32(const uint32_t* __restrict__ db, const uint32_t* __restrict__ q,
                                                                uint32_t n_rows, uint32_t nq, uint32_t nq_pad, uint32_t rows_per_tile,
                                                                uint32_t n_tiles, uint32_t n_qw64, uint32_t cut, uint32_t share_period,
                                                                uint32_t* __restrict__ part, uint32_t* bound,
                                                                uint8_t* __restrict__ stored) {
  const uint32_t tile = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
  if (tile >= n_tiles) return;
  const uint32_t lane = threadIdx.x & 63u, c = lane & 31u, h = lane >> 5;
  const Fp4Consts kc = fp4_consts();
  Fp4Row qb;
  {
    const uint4 p = *reinterpret_cast<const uint4*>(q + (size_t)(c < nq ? c : nq - 1u) * kWords + 4u * h);
    expand_row(p, qb, kc);
  }
  uint32_t best[K];
#pragma unroll
  for (int j = 0; j < K; ++j) best[j] = 0xFFFFFFFFu;
  float thr = thr_of_limit(cut);
  const uint32_t row0 = tile * rows_per_tile;
  const uint32_t n_local = min(n_rows, row0 + rows_per_tile) - row0;
  const uint32_t n_full = n_local / 32u, n_steps = (n_local + 31u) / 32u;
  const uint32_t last_row = n_rows - 1u;
  auto load_step = [&](uint32_t step) -> uint4 {
    const uint32_t r = min(row0 + 32u * min(step, n_steps - 1u) + c, last_row);
    return *reinterpret_cast<const uint4*>(db + (size_t)r * kWords + 4u * h);
  };
  uint4 p0 = load_step(0), p1 = load_step(1), p2 = load_step(2), p3 = load_step(3);
  mfma_f32x16 acc_a, acc_b;                                          // acc_b: pending block of the previous step -- none yet
#pragma unroll
  for (int i = 0; i < 16; ++i) acc_b[i] = -4096.f;                        // below every threshold (256 - 2 * 1023 at the least)
  uint32_t* my_bound = bound + (c < nq ? c : nq - 1u);
  uint32_t seen = 0xFFFFFFFFu, next_share = 2u, step = 0;
  for (; step + 4u <= n_full; step += 4u) {                          // four steps per trip: p0..p3 rotate by name, nothing is copied
    Fp4Row a;
    expand_row(p0, a, kc); p0 = load_step(step + 4u);
    acc_a = dot_block(a, qb);
    mfma_block_test<K, false, IMAX>(acc_b, thr, 32u * step - 32u + 4u * h, n_local, best);
    expand_row(p1, a, kc); p1 = load_step(step + 5u);
    acc_b = dot_block(a, qb);
    mfma_block_test<K, false, IMAX>(acc_a, thr, 32u * step + 4u * h, n_local, best);
    expand_row(p2, a, kc); p2 = load_step(step + 6u);
    acc_a = dot_block(a, qb);
    mfma_block_test<K, false, IMAX>(acc_b, thr, 32u * step + 32u + 4u * h, n_local, best);
    expand_row(p3, a, kc); p3 = load_step(step + 7u);
    acc_b = dot_block(a, qb);
    mfma_block_test<K, false, IMAX>(acc_a, thr, 32u * step + 64u + 4u * h, n_local, best);
    if (step + 4u >= next_share) {                                   // wave-uniform; as hamming_topk_mfma
      next_share += share_period;
      const uint32_t worst_d = best[K - 1] >> kLocalBits;
      if (worst_d < (0xFFFFFFFFu >> kLocalBits) && worst_d < seen) atomicMin(my_bound, worst_d);
      if (seen != 0xFFFFFFFFu) thr = fmaxf(thr, thr_of_limit(seen + 1u));
      seen = __hip_atomic_load(my_bound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  // the pending block of the last full trip, then up to three full and one partial step, one at a time (masked form)
  mfma_block_test<K, true, IMAX>(acc_b, thr, 32u * step - 32u + 4u * h, step ? n_local : 0u, best);
  for (; step < n_steps; ++step) {
    Fp4Row a;
    expand_row(p0, a, kc);
    p0 = p1; p1 = p2; p2 = p3; p3 = load_step(step + 4u);
    acc_a = dot_block(a, qb);
    mfma_block_test<K, true, IMAX>(acc_a, thr, 32u * step + 4u * h, n_local, best);
  }
  uint32_t other[K];
#pragma unroll
  for (int j = 0; j < K; ++j) other[j] = __shfl_xor(best[j], 32);
#pragma unroll
  for (int j = 0; j < K; ++j) topk_insert<K>(best, other[j]);
  // nq <= 32: this block is the only one of its 64-query group, so the flag byte is this wave's alone
  if (__builtin_amdgcn_ballot_w64(c < nq && best[0] != 0xFFFFFFFFu) != 0ull) {
    if (h == 0u && c < nq) {
#pragma unroll
      for (int j = 0; j < K; ++j) part[((size_t)tile * K + j) * nq_pad + c] = best[j];
    }
    if (lane == 0) stored[(size_t)tile * n_qw64] = 0;
  }
}
