// mfma_tile_rows (tod_amd/csrc/match_tiles.h) against the three expressions it replaced, restated here as they stood in
// launch_topk_mfma_qt, launch_topk_mfma_q32 and launch_collect: every n_rows in 1..70 000, a spread of query waves, 256 CUs.
// tile_plan against the three expressions it replaced, restated as they stood in finish_tiling (n_tiles, blocks_per_xcd,
// tiles_per_xcd, groups), launch_wide (n_tiles, groups) and launch_collect (n_tiles, blocks): the same sweep (1, 31, 32 and 33 rows are
// part of it), each with the tile size its launcher asks for. 4 waves per block, a merge fan-in of 16.
// Prints the number of comparisons; exits 1 at the first difference.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "match_tiles.h"

static uint32_t old_k4x(uint32_t n_rows, uint32_t n_cu, uint32_t wpc, uint32_t n_qw) {
  uint32_t n_tiles = std::max(1u, n_cu * wpc / n_qw);
  n_tiles = std::min(n_tiles, std::max(1u, n_rows / 256u));
  n_tiles = std::min(n_tiles, 8192u);
  if (n_tiles >= 16) n_tiles &= ~7u;
  return ((n_rows + n_tiles - 1) / n_tiles + 31u) & ~31u;
}
static uint32_t old_q32(uint32_t n_rows, uint32_t n_cu) {
  uint32_t n_tiles = std::max(1u, std::min<uint32_t>(n_cu * 32u, n_rows / 2048u));
  n_tiles = std::min(n_tiles, 8192u);
  return ((n_rows + n_tiles - 1) / n_tiles + 31u) & ~31u;
}
static uint32_t old_collect(uint32_t n_rows, uint32_t n_cu, uint32_t n_qw) {
  uint32_t n_tiles = std::max(1u, n_cu * 16u / n_qw);
  n_tiles = std::min(std::min(n_tiles, std::max(1u, n_rows / 256u)), 8192u);
  return (uint32_t)((((uint64_t)n_rows + n_tiles - 1u) / n_tiles + 31u) & ~31ull);
}


// finish_tiling, as it stood in match_launch.h
struct OldTiling { uint32_t n_tiles, blocks_per_xcd, tiles_per_xcd, groups; };
static OldTiling old_finish_tiling(uint32_t n_rows, uint32_t rows_per_tile, uint32_t n_qw) {
  OldTiling t;
  t.n_tiles = (n_rows + rows_per_tile - 1) / rows_per_tile;
  const uint32_t items = t.n_tiles * n_qw;
  const uint32_t blocks = (items + 4 - 1) / 4;
  t.blocks_per_xcd = (blocks + 7u) / 8u;
  t.tiles_per_xcd = 0;
  if (t.n_tiles >= 8 && t.n_tiles % 8u == 0) {
    t.tiles_per_xcd = t.n_tiles / 8u;
    t.blocks_per_xcd = (t.tiles_per_xcd * n_qw + 4 - 1) / 4;
  }
  t.groups = std::min(t.n_tiles, (uint32_t)16);
  return t;
}
// launch_wide's and launch_collect's tile count; launch_wide's merge fan-in and grid; launch_collect's grid
static uint32_t old_linear_tiles(uint32_t n_rows, uint32_t rows_per_tile) { return (uint32_t)(((uint64_t)n_rows + rows_per_tile - 1u) / rows_per_tile); }
static uint32_t old_wide_groups(uint32_t n_tiles) { return std::min(n_tiles, (uint32_t)16); }
static uint32_t old_wide_blocks(uint32_t n_tiles, uint32_t n_qw) { return (uint32_t)(((uint64_t)n_tiles * n_qw + 4 - 1u) / 4); }
static uint32_t old_collect_blocks(uint32_t n_tiles, uint32_t n_qw) { return (n_tiles * n_qw + 4 - 1u) / 4; }

static bool plan_equals_old(uint32_t n_rows, uint32_t rows_per_tile, uint32_t n_qw, const char* who) {
  const Tiling t = tile_plan(n_rows, rows_per_tile, n_qw, 4u, 16u);
  const OldTiling o = old_finish_tiling(n_rows, rows_per_tile, n_qw);
  const uint32_t lin = old_linear_tiles(n_rows, rows_per_tile);
  const bool ok = t.rows_per_tile == rows_per_tile && t.n_tiles == o.n_tiles && t.blocks_per_xcd == o.blocks_per_xcd &&
                  t.tiles_per_xcd == o.tiles_per_xcd && t.groups == o.groups && t.n_tiles == lin && t.groups == old_wide_groups(lin) &&
                  t.blocks == old_wide_blocks(lin, n_qw) && t.blocks == old_collect_blocks(lin, n_qw);
  if (!ok) printf("plan (%s) n_rows %u rows_per_tile %u n_qw %u: %u tiles, %u blocks, %u per XCD, %u tiles per XCD, %u groups\n", who, n_rows,
                  rows_per_tile, n_qw, t.n_tiles, t.blocks, t.blocks_per_xcd, t.tiles_per_xcd, t.groups);
  return ok;
}

int main() {
  const uint32_t n_cu = 256, n_qws[] = {1, 2, 3, 5, 8, 11, 32, 63, 84, 125, 250, 500, 513, 4096, 4097, 8192, 8193, 100000};
  unsigned long long n = 0;
  for (uint32_t n_rows = 1; n_rows <= 70000; ++n_rows) {
    const uint32_t a = mfma_tile_rows(n_rows, n_cu * 32u, 2048u, false), b = old_q32(n_rows, n_cu);
    if (a != b) { printf("q32 n_rows %u: %u, was %u\n", n_rows, a, b); return 1; }
    if (!plan_equals_old(n_rows, a, 1u, "q32")) return 1;
    n += 2;
    for (uint32_t n_qw : n_qws) {
      for (uint32_t wpc : {8u, 16u, 32u, 1u, 14u, 128u}) {             // the launcher's three choices, and TODHIP_K4X_WAVES_PER_CU's
        const uint32_t c = mfma_tile_rows(n_rows, n_cu * wpc / n_qw, 256u, true), d = old_k4x(n_rows, n_cu, wpc, n_qw);
        if (c != d) { printf("K4x n_rows %u n_qw %u wpc %u: %u, was %u\n", n_rows, n_qw, wpc, c, d); return 1; }
        if (!plan_equals_old(n_rows, c, n_qw, "K4x")) return 1;
        n += 2;
      }
      const uint32_t e = mfma_tile_rows(n_rows, n_cu * 16u / n_qw, 256u, false), f = old_collect(n_rows, n_cu, n_qw);
      if (e != f) { printf("R1 n_rows %u n_qw %u: %u, was %u\n", n_rows, n_qw, e, f); return 1; }
      if (!plan_equals_old(n_rows, e, n_qw, "R1, W1")) return 1;
      n += 2;
    }
  }
  printf("%llu\n", n);
  return 0;
}
