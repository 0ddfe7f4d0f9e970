// Host planning of the 32-byte matcher's launches: the environment knobs and the launchers of both engines. Each engine keeps its
// own, measured policy for how many tiles to ask for; what follows that policy is shared (match_plan.h: tiling, workspaces, merge
// launch). The k of the reference's knnMatch is DescriptorMatcher.cpp:211, its radius cut :212-220.
// Included by match.hip inside its anonymous namespace, after match_keys.h, match_valu.h, match_fp4.h, match_mfma.h, match_fp4rows.h
// (expand_rows_fp4_kernel, hamming_topk_fp4rows), match_merge.h and match_plan.h.

int k4_engine(const todhip_ctx* ctx, uint32_t nq);   // match.hip, behind this header

// Tuning and diagnostics knobs, read once per process (tools/README.md has the same table).
struct MatchEnv {
  char engine;          // TODHIP_K4_ENGINE=valu|mfma      the engine while the context says "auto" (the first letter decides)
  int k4_mode;          // TODHIP_K4_MODE=0..3             K4's elimination schedule (default -1: by radius)
  int k4_wpc;           // TODHIP_K4_WAVES_PER_CU=n        K4 tiling: n waves per CU instead of the oversubscribed default (0)
  int k4x_wpc;          // TODHIP_K4X_WAVES_PER_CU=n       K4x tiling: n waves per CU instead of 8 / 16 / 32 by launch shape (0)
  int k4x_share;        // TODHIP_K4X_SHARE=n              K4x: steps between two exchanges of the distance bounds (16; each launcher has a floor). The paired split-2 step ignores it: it exchanges where a block goes on (fp4rows_pair_complete)
  int k4x_qt;           // TODHIP_K4X_QT=2|4|6|8           K4x: query blocks per wave, also for <= 32 queries (0: by launch shape)
  int k4x_half;         // TODHIP_K4X_HALF=0|2|3           the process's default for todhip_set_matcher_block_split (-1: adaptive; 1 = 2)
  bool k4x_half_debug;  // TODHIP_K4X_HALF_DEBUG           print every report of the split controller to stderr
  int k4x_fp4_rows;     // TODHIP_K4X_FP4_ROWS=0|1         K4x: launches of 4 or 6 query blocks per wave read the rows from their resident fp4 copy (1)
  int k4x_fp4_rows_mb;  // TODHIP_K4X_FP4_ROWS_MB=n        K4x: the largest fp4 copy a context builds, in MiB (512); beyond it the packed rows are read
  int k4x_pairs;        // TODHIP_K4X_PAIRS=0|1            K4x over the fp4 copy, split 2: two blocks per accumulator, tested at the launch's radius, where measured to win (1); 0: single blocks
};
inline const MatchEnv& match_env() {
  static const MatchEnv env = [] {
    auto num = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
    const char* eng = getenv("TODHIP_K4_ENGINE");
    return MatchEnv{eng ? eng[0] : '\0', num("TODHIP_K4_MODE", -1), num("TODHIP_K4_WAVES_PER_CU", 0), num("TODHIP_K4X_WAVES_PER_CU", 0),
                    num("TODHIP_K4X_SHARE", 16), num("TODHIP_K4X_QT", 0), num("TODHIP_K4X_HALF", -1), getenv("TODHIP_K4X_HALF_DEBUG") != nullptr,
                    num("TODHIP_K4X_FP4_ROWS", 1), num("TODHIP_K4X_FP4_ROWS_MB", 512), num("TODHIP_K4X_PAIRS", 1)};
  }();
  return env;
}

// The fp4 copy of the active rows (ctx.h: db_fp4; layout fp4_rows.h) for a launch that reads it: built here the first time, and again
// when the rows have changed since (tod_db_rows_written). *out stays nullptr where no copy is kept -- switched off, or larger than the
// cap -- and the launch reads the packed rows. The packed rows are readable up to the end of their last 32-row step (kDbSlackBytes).
inline int fp4_rows_ready(todhip_ctx* ctx, uint32_t n_rows, const uint4** out) {
  const MatchEnv& env = match_env();
  const size_t bytes = fp4_rows_bytes(n_rows);
  if (env.k4x_fp4_rows == 0 || bytes > ((size_t)std::max(0, env.k4x_fp4_rows_mb) << 20) || bytes >= (1ull << 32)) return TODHIP_OK;   // (32-bit offsets)
  if (ctx->fp4_gen != ctx->rows_gen) {
    TOD_HIP(ctx->db_fp4.reserve(bytes));
    hipLaunchKernelGGL(expand_rows_fp4_kernel, dim3(fp4_rows_steps(n_rows)), dim3(kBlock), 0, ctx->stream,
                       reinterpret_cast<const uint32_t*>(tod_db_rows(ctx)), fp4_rows_steps(n_rows), ctx->db_fp4.as<uint4>());
    TOD_HIP(hipGetLastError());
    ctx->fp4_gen = ctx->rows_gen;
    ++ctx->counters.fp4_rows_builds;
  }
  *out = ctx->db_fp4.as<uint4>();
  return TODHIP_OK;
}
// Which launches read the copy: every one of 4 or 6 query blocks per wave, in every block form. The copy takes the expansion (a third of
// a split step's vector instructions) out of a loop bound by vector issue and puts four times the bytes through the vector L1 instead;
// measured alone (tools/time_fp4_rows.sh, profiles/match_fp4_rows.json) that pays in each form at 32 000 x 1M (split 2: 1.57 -> 1.43 ms,
// split 3: 1.88 -> 1.82, whole blocks: 2.32 -> 2.28) and from one frame per launch on (1000 x 1M, 8 query waves per tile: 0.102 -> 0.098;
// 4000 queries tie at 0.26), so there is no floor on the launch size. Eight blocks per wave keep the packed rows (no room for two
// steps' fragments), two blocks and the <= 32-query form are bound by HBM, where four times the bytes would cost four times the time.

template <int K, int QT>
int launch_topk_mfma_qt(todhip_ctx* ctx, const uint32_t* d_q, uint32_t nq, uint32_t radius, uint64_t* d_lists, uint32_t* n_lists) {
  constexpr bool PF2 = QT < 8;                                        // register budget: see hamming_topk_mfma
  const MatchEnv& env = match_env();
  const uint32_t cut = radius >= 256u ? kNoLimit : radius + 1u;       // distances are <= 256: no cut beyond that
  const uint32_t n_rows = (uint32_t)tod_db_n_rows(ctx);
  const uint32_t n_qw = (nq + 32u * QT - 1u) / (32u * QT), n_qw64 = (nq + 63u) / 64u;
  const uint32_t nq_pad = n_qw64 * 64u;
  // Rounds of waves: the chip holds 8 of these waves per CU (2 per SIMD, by registers). A launch whose wave count is just
  // under a whole number of rounds has no straggling last round (measured, tools/k4x_sweep.py, 16 000 x 1M: 16 waves per
  // CU = 2 rounds 1.13 ms, 14 = 1.6 rounds 1.37 ms, 8 = all resident 1.36 ms, 32 .. 128 1.11 ms); four rounds while a tile
  // then still has >= 48 steps (a tile starts with empty lists), two otherwise. Tiles: mfma_tile_rows, of >= 256 rows.
  uint32_t wpc = 32;
  if ((uint64_t)n_rows * n_qw < (uint64_t)ctx->n_cu * wpc * 1536u) wpc = 16;
  // A tile starts with empty lists and the radius as its threshold, and every row inside the threshold costs a walk of its block
  // until the list's k-th entry tightens it. On independent bits almost no row is; on self-similar texture (rendered views of
  // rectangle patterns: a median of 1300 rows of 1M within 35 bits of a query, tools/count_close_rows.py) tiles of a few hundred
  // rows spend their life in that walk. One frame's launch therefore gets at most 8 waves per CU (tiles of >= ~4000 rows)
  // and 4 query blocks per wave (launch_topk_mfma): 0.32 -> 0.19 ms on such a frame, 0.096 -> 0.095 ms on independent bits
  // (tools/k4x_chained_frame.sh, tools/k4x_synth_frame.sh).
  if ((uint64_t)n_rows * n_qw < (uint64_t)ctx->n_cu * 16u * 4096u) wpc = 8;
  if (env.k4x_wpc > 0) wpc = (uint32_t)env.k4x_wpc;
  Tiling t;
  if (!finish_tiling(n_rows, mfma_tile_rows(n_rows, (uint32_t)ctx->n_cu * wpc / n_qw, 256u, true), n_qw, &t)) return TODHIP_EINVAL;
  uint8_t* const d_stored = prepare_lists<K>(ctx, t.n_tiles, nq_pad, n_qw64);
  if (!d_stored) return TODHIP_EHIP;
  KernelTimer timer{ctx};
  if (int rc = timer.begin()) return rc;
  // radius < 128: every threshold is >= 0 and the block test may compare raw bits (see mfma_block_test). cut <= 64 / <= 96: the
  // thresholds minus 128 / 64 are >= 0 as well and a block may be split after 2 / 3 of its 4 MFMAs (mfma_block_test_part); which
  // split a launch takes is K4xSplit's business (match_split.h).
  const uint32_t min_split = QT < 4 ? 4u : (cut <= 64u ? 2u : (cut <= 96u ? 3u : 4u));   // the lowest split the thresholds allow
  if (ctx->k4x.may_split(min_split, env.k4x_half)) {
    if (!ctx->k4x_stats_host.p) {
      TOD_HIP(ctx->k4x_stats_host.reserve(64));
      std::memset(ctx->k4x_stats_host.p, 0, 64);
      TOD_HIP(ctx->k4x_stats_dev.reserve(64));
      TOD_HIP(hipMemsetAsync(ctx->k4x_stats_dev.p, 0, 64, ctx->stream));
    }
    ctx->k4x.take_report(ctx->k4x_stats_host.as<uint32_t>(), ctx->counters, min_split, env.k4x_half, env.k4x_half_debug);
  }
  const uint32_t split = ctx->k4x.next(min_split, env.k4x_half);       // 4 = whole blocks
  // the kernels' MODE; 4 is hamming_topk_fp4rows' split 2 in single blocks (hamming_topk_mfma knows one split-2 form, MODE 2)
  // The paired step where it was measured to win (profiles/match_pairs.json, the pass alone, adaptive form, parent and child
  // alternating): six blocks per wave at every size (4 .. 32 frames: -6 .. -9 %), four blocks per wave for one frame's launch
  // (0.106 -> 0.094 ms); at two frames (2000 queries, four blocks, tiles twice as long) it lost 4 % (0.131 -> 0.137), so launches of
  // four blocks beyond 1024 queries keep the single-block step.
  const bool pairs = env.k4x_pairs != 0 && (QT == 6 || nq <= 1024u);
  const int mode = split == 2 ? (pairs ? 2 : 4) : split == 3 ? 3 : cut <= 128u ? 1 : 0;
  ctx->counters.last_block_split = split;
  uint32_t* const d_stats = split < 4 ? ctx->k4x_stats_dev.as<uint32_t>() : nullptr;
  const uint4* rows_fp4 = nullptr;                                     // the fp4 copy, where this launch reads it
  if ((QT == 4 || QT == 6) && t.rows_per_tile % 32u == 0u)          // (a tile starts on a step of the copy: mfma_tile_rows gives whole steps)
    if (int rc = fp4_rows_ready(ctx, n_rows, &rows_fp4)) return rc;
  ctx->counters.last_fp4_rows = rows_fp4 ? 1u : 0u;
  // the two passes differ in the rows they read and in nothing behind them
  auto launch = [&](auto kern, auto rows) {
    hipLaunchKernelGGL(kern, dim3(t.blocks_per_xcd * 8u), dim3(kBlock), 0, ctx->stream, rows, d_q, n_rows, nq, nq_pad, t.rows_per_tile,
                       t.n_tiles, n_qw, n_qw64, t.blocks_per_xcd, t.tiles_per_xcd, cut, (uint32_t)std::max(2, env.k4x_share),
                       ctx->m_part.as<uint32_t>(), ctx->m_bound.as<uint32_t>(), d_stored, d_stats ? d_stats + 2u * (split - 2u) : nullptr);
  };
  auto launch_mode = [&](auto M) {
    constexpr int MODE = decltype(M)::value;
    if constexpr (QT == 4 || QT == 6)                                  // (eight blocks per wave leave no room for two steps' fragments)
      if (rows_fp4) return launch(hamming_topk_fp4rows<K, QT, MODE>, rows_fp4);
    launch(hamming_topk_mfma<K, QT, MODE == 4 ? 2 : MODE, PF2>, reinterpret_cast<const uint32_t*>(tod_db_rows(ctx)));
  };
  switch (mode) {
    case 0: launch_mode(std::integral_constant<int, 0>{}); break;
    case 1: launch_mode(std::integral_constant<int, 1>{}); break;
    case 2: launch_mode(std::integral_constant<int, 2>{}); break;
    case 4: launch_mode(std::integral_constant<int, 4>{}); break;
    default: launch_mode(std::integral_constant<int, 3>{}); break;
  }
  if (int rc = timer.end()) return rc;
  if (d_stats) ++ctx->k4x.seq_sent;
  if (nq <= 64u && !d_stats && t.n_tiles >= 256u) return launch_merge_wave<K>(ctx, nq, nq_pad, t, d_stored, n_qw64, d_lists, n_lists);
  return launch_merge<K>(ctx, nq, nq_pad, t, d_stored, n_qw64, d_stats, d_lists, n_lists);
}

template <int K>
int launch_topk_mfma_q32(todhip_ctx* ctx, const uint32_t* d_q, uint32_t nq, uint32_t radius, uint64_t* d_lists, uint32_t* n_lists) {
  const uint32_t cut = radius >= 256u ? kNoLimit : radius + 1u;
  const uint32_t n_rows = (uint32_t)tod_db_n_rows(ctx), n_qw64 = 1u, nq_pad = 64u;
  // one wave per tile; about 32 waves per CU in all (each holds four 1 KB loads in flight), tiles of >= 2048 rows
  Tiling t;
  if (!finish_tiling(n_rows, mfma_tile_rows(n_rows, (uint32_t)ctx->n_cu * 32u, 2048u, false), 1u, &t)) return TODHIP_EINVAL;
  uint8_t* const d_stored = prepare_lists<K>(ctx, t.n_tiles, nq_pad, n_qw64);
  if (!d_stored) return TODHIP_EHIP;
  KernelTimer timer{ctx};
  if (int rc = timer.begin()) return rc;
  auto kern = cut <= 128u ? hamming_topk_mfma_q32<K, true> : hamming_topk_mfma_q32<K, false>;
  ctx->counters.last_fp4_rows = 0;                                    // one query block per wave: the packed rows, bound by HBM
  hipLaunchKernelGGL(kern, dim3((t.n_tiles + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlock), 0, ctx->stream,
                     reinterpret_cast<const uint32_t*>(tod_db_rows(ctx)), d_q, n_rows, nq, nq_pad, t.rows_per_tile, t.n_tiles, n_qw64, cut,
                     (uint32_t)std::max(4, match_env().k4x_share), ctx->m_part.as<uint32_t>(), ctx->m_bound.as<uint32_t>(), d_stored);
  if (int rc = timer.end()) return rc;
  return launch_merge_wave<K>(ctx, nq, nq_pad, t, d_stored, n_qw64, d_lists, n_lists);
}

template <int K>
int launch_topk_mfma(todhip_ctx* ctx, const uint32_t* d_q, uint32_t nq, uint32_t radius, uint64_t* d_lists, uint32_t* n_lists) {
  const int env_qt = match_env().k4x_qt;
  if (nq <= 32u && !(env_qt > 0))
    return launch_topk_mfma_q32<K>(ctx, d_q, nq, radius, d_lists, n_lists);
  // Query blocks of 32 per wave (QT): the registers hold 8 beside the k-entry lists for k <= 2, 6 for k <= 5 (the reference's k,
  // DescriptorMatcher.cpp:211), 4 beyond. Six is the default even where eight fit: with eight a wave takes 256 registers, two waves
  // fill a SIMD's file, and every kernel of the other stages (ORB, verifier) then waits for a matcher workgroup to retire before
  // one of its own can start -- a quarter of a DB pass, 25 dependent launches per ORB batch. With six (213-221 registers, allocated
  // in eights: 64-80 of a SIMD's 512 stay free) those kernels run beside the matcher's waves: alone the pass is 2 % slower (2.36 vs 2.32 ms whole blocks), in the
  // pipeline ORB's stage falls from 1.9 to 1.2 ms, the verifier's from 2.05 to 1.5, and the matcher's own launch is no slower
  // (tools/ab_k4x_residency.sh: headline 16.2k -> 16.6k frames/s, chained 8.7k -> 9.9k). Among the candidates the one that pads nq
  // the least wins when that saves more than 3 % (a wave computes all its blocks; 1000 queries are 4 x 256 but 6 x 192).
  // TODHIP_K4X_QT forces one (experiments).
  // With at most 64 queries a wave holds two blocks (QT = 2): 8 MFMAs per 1 KB of rows -- the pass is then bound by HBM,
  // not by the matrix pipe (BASELINE.json's "achieved HBM GB/s on BF-matcher" regime; tools/k4_small_q.py).
  constexpr int kMaxQT = K <= 2 ? 8 : (K <= 5 ? 6 : 4);
  auto padded = [&](uint32_t qt) { return (uint64_t)((nq + 32u * qt - 1u) / (32u * qt) * (32u * qt)); };
  int qt = kMaxQT >= 6 ? 6 : 4;
  if (kMaxQT >= 8 && padded(8) * 103u < padded(6) * 100u) qt = 8;
  if (qt > 4 && padded(4) * 103u < padded((uint32_t)qt) * 100u) qt = 4;
  if (padded(2) * 103u < padded((uint32_t)qt) * 100u) qt = 2;
  if (nq <= 2048u && qt > 4) qt = 4;                                  // a frame or two: longer tiles, see launch_topk_mfma_qt
  if ((env_qt == 2 || env_qt == 4 || env_qt == 6 || env_qt == 8) && env_qt <= kMaxQT) qt = env_qt;
  if (qt == 8) return launch_topk_mfma_qt<K, (kMaxQT >= 8 ? 8 : 4)>(ctx, d_q, nq, radius, d_lists, n_lists);
  if (qt == 6) return launch_topk_mfma_qt<K, (kMaxQT >= 6 ? 6 : 4)>(ctx, d_q, nq, radius, d_lists, n_lists);
  if (qt == 2) return launch_topk_mfma_qt<K, 2>(ctx, d_q, nq, radius, d_lists, n_lists);
  return launch_topk_mfma_qt<K, 4>(ctx, d_q, nq, radius, d_lists, n_lists);
}

template <int K>
int launch_topk(todhip_ctx* ctx, const uint32_t* d_q, uint32_t nq, uint32_t radius, uint64_t* d_lists, uint32_t* n_lists) {
  if (k4_engine(ctx, nq) == 1) return launch_topk_mfma<K>(ctx, d_q, nq, radius, d_lists, n_lists);
  const MatchEnv& env = match_env();
  const uint32_t cut = radius >= 256u ? 0xFFFFFFFFu : radius + 1u;   // distances are <= 256: no cut beyond that
  const uint32_t n_rows = (uint32_t)tod_db_n_rows(ctx);
  const uint32_t n_qw = (nq + 63u) / 64u;
  const uint32_t nq_pad = n_qw * 64u;
  // Tiling (measured, tools/time_k4.py): about three times more waves than fit the chip at once and tiles of at most
  // ~2048 rows (16 000 queries x 1M rows: 3.27 ms with 4096-row tiles, 3.20 ms with 2048; 10M rows: 35.6 -> 34.3 ms).
  // An exactly-resident grid of long-running waves (the first design) lost 15-20 %: the hardware does not spread
  // blocks evenly over the CUs, and the query waves of a large tile drift apart in it (scalar-cache and L2 misses);
  // short blocks rebalance by themselves and keep a tile's readers together.
  uint32_t n_tiles;
  if (env.k4_wpc > 0) {
    n_tiles = (uint32_t)ctx->n_cu * (uint32_t)env.k4_wpc / n_qw;
  } else {
    n_tiles = std::max(3u * (uint32_t)ctx->n_cu * (uint32_t)kWavesPerCU / n_qw, (n_rows + 2047u) / 2048u);
    n_tiles = std::min(n_tiles, 8192u);
  }
  if (n_tiles < 1) n_tiles = 1;
  if (n_tiles >= 8) n_tiles = (n_tiles + 7u) & ~7u;      // whole tiles per XCD (8 XCDs)
  uint32_t rows_per_tile = (n_rows + n_tiles - 1) / n_tiles;
  rows_per_tile = ((rows_per_tile + 2 * kGroupRows - 1) / (2 * kGroupRows)) * (2 * kGroupRows);
  if (rows_per_tile < 64) rows_per_tile = 64;
  Tiling t;
  if (!finish_tiling(n_rows, rows_per_tile, n_qw, &t)) return TODHIP_EINVAL;
  uint8_t* const d_stored = prepare_lists<K>(ctx, t.n_tiles, nq_pad, n_qw);
  if (!d_stored) return TODHIP_EHIP;
  KernelTimer timer{ctx};
  if (int rc = timer.begin()) return rc;
  // every schedule is exact; TODHIP_K4_MODE overrides the choice (diagnostics: tools/k4_on_correlated_descriptors.py)
  const int mode = (env.k4_mode >= 0 && env.k4_mode <= 3 && cut <= 256u) ? env.k4_mode
                                                                         : (cut <= 38u ? 2 : (cut <= 48u ? 1 : (cut <= 80u ? 3 : 0)));
  auto kern = mode == 2 ? hamming_topk_tiles<K, 2>
                        : (mode == 1 ? hamming_topk_tiles<K, 1> : (mode == 3 ? hamming_topk_tiles<K, 3> : hamming_topk_tiles<K, 0>));
  hipLaunchKernelGGL(kern, dim3(t.blocks_per_xcd * 8u), dim3(kBlock), 0, ctx->stream,
                     reinterpret_cast<const uint32_t*>(tod_db_rows(ctx)), d_q, n_rows, nq, nq_pad, t.rows_per_tile, t.n_tiles, n_qw,
                     t.blocks_per_xcd, t.tiles_per_xcd, cut, ctx->m_part.as<uint32_t>(), ctx->m_bound.as<uint32_t>(), d_stored);
  if (int rc = timer.end()) return rc;
  return launch_merge<K>(ctx, nq, nq_pad, t, d_stored, n_qw, nullptr, d_lists, n_lists);
}
