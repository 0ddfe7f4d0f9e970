// K4x, the exact top-k search on the matrix cores: the tests of the 32 x 32 accumulator blocks (whole and split), the 32-row step,
// hamming_topk_mfma and its <= 32-query form hamming_topk_mfma_q32, on match_fp4.h's arithmetic, layout and block primitives: the
// pass over the PACKED rows, which expands them as it goes. The same pass over the resident fp4 copy of the rows is match_fp4rows.h,
// which uses this header's block tests.
// TOD_K4X_ABLATE / TOD_K4X_COUNT_WALKS are diagnostics builds (tools/k4x_ablate.sh, tools/k4x_walks.sh). The radius bound restates
// DescriptorMatcher.cpp:212-220. Included by match.hip inside its anonymous namespace, after match_keys.h and match_fp4.h.
// A lane keeps its k best keys in registers exactly as K4 does, and the threshold of its block test follows the list's k-th entry.
// Bounds are exchanged between tiles through the same per-query word as K4 (loaded one period ahead, so the latency of the load is
// never waited for). Output = K4's partial-key layout.
// The test of one accumulator block: nothing to do unless some lane's best dot product beats its threshold (rare: the
// thresholds follow the k-th best distance found so far, anywhere in the DB); then walk the block's 16 rows. MASK: rows at
// or beyond n_lim do not exist (the last, partial step of the DB). IMAX: thresholds are >= 0 (block_reaches).
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
    if (__builtin_amdgcn_ballot_w64(block_reaches<IMAX, false>(acc, thr)) == 0ull) return;
#ifdef TOD_K4X_COUNT_WALKS
    if ((threadIdx.x & 63u) == 0u) atomicAdd(&g_k4x_blocks[1], 1ull);
#endif
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t ri = block_row(i);                      // r_lane = lane_row_base(step): r_lane | ri is the tile-local row
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

// The same in two parts (dot_part0, then the rest behind this test). Partial-distance elimination on the matrix cores (K4's idea, a block at a time): after P = 64 SPLIT of the 256 bit positions the
// accumulator holds P - 2 dP with dP <= d, so a pair whose partial dot product is not above thr - (256 - P) (dP >= limit) cannot
// be a hit whatever the other positions say -- exact for any data. On independent bits d128 of a non-match is 64 +- 5.7 and
// the radius 35: one block in five thousand goes on to its other two MFMAs (SPLIT 2). Real rBRIEF bits are biased and correlated
// (mean distance ~100 of 256 on this library's ORB descriptors of rendered views): there almost every block survives 128 positions
// and SPLIT 3 is the form that prunes (d192 ~ 75 +- 9.5). Needs thr - (256 - P) >= 0 for the integer maximum (limits up to 64 for
// SPLIT 2, up to 96 for SPLIT 3; thresholds only tighten). rows / q: the fragments the block's first part was computed from.
template <int K, int SPLIT>
__device__ __forceinline__ bool mfma_block_test_part(mfma_f32x16& acc, const Fp4Row& rows, const Fp4Row& q, float& thr, float& thrp,
                                                     uint32_t r_lane, uint32_t n_lim, uint32_t (&best)[K]) {
  // The part thresholds (thrp = thr - 64 (4 - SPLIT)) live in registers of their own beside the whole ones: one instruction less
  // per block (1.82 -> 1.73 ms in the pipeline) for six registers, 218 -> 224, still inside the budget that lets the other stages'
  // kernels start beside the matcher's waves (launch_topk_mfma; tests/test_build_checks.py holds the line). Keeping ONLY the part
  // form -- no extra registers on paper -- made hipcc allocate 243.
  if (__builtin_amdgcn_ballot_w64(block_reaches<true, false>(acc, thrp)) == 0ull) return false;
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
  Fp4Row qb[QT];
  uint32_t best[QT][K];
  float thr[QT], thrp[QT];                                         // thrp: the part thresholds of the split blocks (mfma_block_test_part)
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    load_query_block(q, q0 + 32u * t + c, nq, h, qb[t], kc);
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
  const StepLoader rows(db, row0, n_steps, c, h);
#if defined(TOD_K4X_ABLATE) && TOD_K4X_ABLATE == 1           // diagnostics build only (tools/k4x_ablate.sh): no DB loads
  auto load_step = [&](uint32_t step) -> uint4 {
    const uint32_t r = rows.first_row(step) + c;
    return uint4{r * 2654435761u, r ^ step, r + h, r * 40503u};
  };
#else
  const StepLoader& load_step = rows;
#endif
  Fp4Row a0, a1;
  {
    const uint4 p = load_step(0);
    expand_row(p, a0, kc);
  }
  // packed rows in flight: of steps + 1 and + 2 (PF2), or of step + 1 only (4 registers less: what lets QT = 8 fit)
  uint4 pa = load_step(1), pb = PF2 ? load_step(2) : pa;
  mfma_f32x16 acc_even, acc_odd;                                    // acc_odd: pending block of the previous step -- none yet
#pragma unroll
  for (int i = 0; i < 16; ++i) acc_odd[i] = kNoBlock;
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
    n_pass += mfma_step<K, QT, false, IMAX, HALF>(a0, a1, pa, qb, thr, thrp, best, acc_even, acc_odd, lane_row_base(step, h), n_local, kc);
    if (PF2) {
      pa = load_step(step + 3u);
      n_pass += mfma_step<K, QT, false, IMAX, HALF>(a1, a0, pb, qb, thr, thrp, best, acc_even, acc_odd, lane_row_base(step, h) + 32u, n_local, kc);
      pb = load_step(step + 4u);
    } else {
      pa = load_step(step + 2u);
      n_pass += mfma_step<K, QT, false, IMAX, HALF>(a1, a0, pa, qb, thr, thrp, best, acc_even, acc_odd, lane_row_base(step, h) + 32u, n_local, kc);
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
    n_pass += mfma_block_test_part<K, HALF ? HALF : 2>(acc_odd, a1, qb[QT - 1], thr[QT - 1], thrp[QT - 1], lane_row_base(step - 1u, h), n_local, best[QT - 1]) ? 1u : 0u;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc_odd[i] = kNoBlock;
    if (lane == 0 && half_stats) { atomicAdd(half_stats, n_pass); atomicAdd(half_stats + 1, step * (uint32_t)QT); }
  }
  // at most one full and one partial step are left: the masked form serves both
  for (; step < n_steps; ++step) {
    mfma_step<K, QT, true, IMAX>(a0, a1, pa, qb, thr, thrp, best, acc_even, acc_odd, lane_row_base(step, h), n_local, kc);
    a0 = a1;
    pa = PF2 ? pb : load_step(step + 2u);
  }
  mfma_block_test<K, true, IMAX>(acc_odd, thr[QT - 1], lane_row_base(n_steps - 1u, h), n_local, best[QT - 1]);   // drain

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
  load_query_block(q, c, nq, h, qb, kc);
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
  for (int i = 0; i < 16; ++i) acc_b[i] = kNoBlock;
  uint32_t* my_bound = bound + (c < nq ? c : nq - 1u);
  uint32_t seen = 0xFFFFFFFFu, next_share = 2u, step = 0;
  for (; step + 4u <= n_full; step += 4u) {                          // four steps per trip: p0..p3 rotate by name, nothing is copied
    Fp4Row a;
    expand_row(p0, a, kc); p0 = load_step(step + 4u);
    acc_a = dot_block(a, qb);
    mfma_block_test<K, false, IMAX>(acc_b, thr, lane_row_base(step - 1u, h), n_local, best);
    expand_row(p1, a, kc); p1 = load_step(step + 5u);
    acc_b = dot_block(a, qb);
    mfma_block_test<K, false, IMAX>(acc_a, thr, lane_row_base(step, h), n_local, best);
    expand_row(p2, a, kc); p2 = load_step(step + 6u);
    acc_a = dot_block(a, qb);
    mfma_block_test<K, false, IMAX>(acc_b, thr, lane_row_base(step, h) + 32u, n_local, best);
    expand_row(p3, a, kc); p3 = load_step(step + 7u);
    acc_b = dot_block(a, qb);
    mfma_block_test<K, false, IMAX>(acc_a, thr, lane_row_base(step, h) + 64u, n_local, best);
    if (step + 4u >= next_share) {                                   // wave-uniform; as hamming_topk_mfma
      next_share += share_period;
      const uint32_t worst_d = best[K - 1] >> kLocalBits;
      if (worst_d < (0xFFFFFFFFu >> kLocalBits) && worst_d < seen) atomicMin(my_bound, worst_d);
      if (seen != 0xFFFFFFFFu) thr = fmaxf(thr, thr_of_limit(seen + 1u));
      seen = __hip_atomic_load(my_bound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  // the pending block of the last full trip, then up to three full and one partial step, one at a time (masked form)
  mfma_block_test<K, true, IMAX>(acc_b, thr, lane_row_base(step - 1u, h), step ? n_local : 0u, best);
  for (; step < n_steps; ++step) {
    Fp4Row a;
    expand_row(p0, a, kc);
    p0 = p1; p1 = p2; p2 = p3; p3 = load_step(step + 4u);
    acc_a = dot_block(a, qb);
    mfma_block_test<K, true, IMAX>(acc_a, thr, lane_row_base(step, h), n_local, best);
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
