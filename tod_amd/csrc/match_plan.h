// The launch plan every top-k DB pass shares, whatever its engine and row width: the tiling that follows the engine's choice of tile
// size (the arithmetic is match_tiles.h's tile_plan), the workspaces of the partial lists, and the tile merge behind the pass.
// Included by match.hip (in front of match_launch.h) and match_wide.hip inside their anonymous namespaces, after match_keys.h and
// match_merge.h.

// rows_per_tile is the engine's choice, rounded to its granule. False: a tile would not fit the partial key's row bits.
inline bool finish_tiling(uint32_t n_rows, uint32_t rows_per_tile, uint32_t n_qw, Tiling* t) {
  if (rows_per_tile > kLocalMask) return false;
  *t = tile_plan(n_rows, rows_per_tile, n_qw, kWavesPerBlock, kMergeGroups);
  return true;
}

// The partial lists (m_part) and, in one buffer under one memset, the per-query bound words (0xFFFFFFFF = none published) and the
// per-(tile, 64 queries) flag bytes (0xFF = nothing stored). Returns the flags; nullptr: a HIP error, left in the context.
template <int K>
uint8_t* prepare_lists(todhip_ctx* ctx, uint32_t n_tiles, uint32_t nq_pad, uint32_t n_qw64) {
  const size_t bound_bytes = (size_t)nq_pad * sizeof(uint32_t), flag_bytes = (size_t)n_tiles * n_qw64;
  hipError_t e = ctx->m_part.reserve((size_t)n_tiles * K * nq_pad * sizeof(uint32_t));
  if (e == hipSuccess) e = ctx->m_bound.reserve(bound_bytes + flag_bytes);
  if (e == hipSuccess) e = hipMemsetAsync(ctx->m_bound.p, 0xFF, bound_bytes + flag_bytes, ctx->stream);
  if (e != hipSuccess) { ctx->last_hip_error = (int)e; return nullptr; }
  return ctx->m_bound.as<uint8_t>() + bound_bytes;
}

// K4m behind a DB pass. d_stats: the DB pass's split-block counters, which this form carries to pinned memory (K4xSplit::take_report
// reads them there).
template <int K>
int launch_merge(todhip_ctx* ctx, uint32_t nq, uint32_t nq_pad, const Tiling& t, const uint8_t* d_stored, uint32_t n_qw64,
                 const uint32_t* d_stats, uint64_t* d_lists, uint32_t* n_lists) {
  hipLaunchKernelGGL(merge_tiles_kernel<K>, dim3((nq + kBlock - 1) / kBlock, t.groups), dim3(kBlock), 0, ctx->stream,
                     ctx->m_part.as<uint32_t>(), nq, nq_pad, t.n_tiles, t.rows_per_tile, tod_db_first_row(ctx), t.groups, d_stored, n_qw64, d_lists,
                     d_stats, d_stats ? ctx->k4x_stats_host.as<uint32_t>() : (uint32_t*)nullptr, d_stats ? ctx->k4x.seq_sent : 0u);
  TOD_HIP(hipGetLastError());
  *n_lists = t.groups;
  return TODHIP_OK;
}

// The wave form: a handful of queries over thousands of tiles, a wave per (query, group). A function of its own, so that a
// translation unit that never asks for it (match_wide.hip) does not carry merge_tiles_wave_kernel.
template <int K>
int launch_merge_wave(todhip_ctx* ctx, uint32_t nq, uint32_t nq_pad, const Tiling& t, const uint8_t* d_stored, uint32_t n_qw64,
                      uint64_t* d_lists, uint32_t* n_lists) {
  hipLaunchKernelGGL(merge_tiles_wave_kernel<K>, dim3((nq + kWavesPerBlock - 1) / kWavesPerBlock, t.groups), dim3(kBlock), 0, ctx->stream,
                     ctx->m_part.as<uint32_t>(), nq, nq_pad, t.n_tiles, t.rows_per_tile, tod_db_first_row(ctx), t.groups, d_stored, n_qw64, d_lists);
  TOD_HIP(hipGetLastError());
  *n_lists = t.groups;
  return TODHIP_OK;
}
