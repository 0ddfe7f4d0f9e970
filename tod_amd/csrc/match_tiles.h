// The DB tiles of the matrix-core searches and the grid that follows from them (host, plain C++; included by ctx.h; tested stand-alone
// by tests/match_tiles_host_test.cpp). Each launcher brings its own, measured wish for the tile count; what follows it is shared.
#pragma once
#include <algorithm>
#include <cstdint>

// Rows per tile when a launcher would like want_tiles tiles: 1 to 8192 tiles of at least min_rows rows (while the DB has that many), a
// multiple of 8 from 16 on if whole_xcds (K4x: whole tiles per XCD), whole 32-row steps. That really gives ceil(n_rows / result) tiles.
inline uint32_t mfma_tile_rows(uint32_t n_rows, uint32_t want_tiles, uint32_t min_rows, bool whole_xcds) {
  uint32_t n_tiles = std::min(std::min(std::max(1u, want_tiles), std::max(1u, n_rows / min_rows)), 8192u);
  if (whole_xcds && n_tiles >= 16u) n_tiles &= ~7u;
  return (uint32_t)((((uint64_t)n_rows + n_tiles - 1u) / n_tiles + 31u) & ~31ull);
}

// What a choice of rows_per_tile gives: the tile count; the grid of blocks of waves_per_block work items (tile, query wave), n_qw
// query waves per tile -- linear (blocks: R1, W1), or per XCD (blocks_per_xcd x 8; whole tiles per XCD when there are 8 k of them: the
// work-item decode of K4 and K4x); and the merge fan-in.
struct Tiling { uint32_t n_tiles, rows_per_tile, blocks, blocks_per_xcd, tiles_per_xcd, groups; };
inline Tiling tile_plan(uint32_t n_rows, uint32_t rows_per_tile, uint32_t n_qw, uint32_t waves_per_block, uint32_t max_groups) {
  Tiling t;
  t.rows_per_tile = rows_per_tile;
  t.n_tiles = (uint32_t)(((uint64_t)n_rows + rows_per_tile - 1u) / rows_per_tile);
  t.blocks = (uint32_t)(((uint64_t)t.n_tiles * n_qw + waves_per_block - 1u) / waves_per_block);
  t.blocks_per_xcd = (t.blocks + 7u) / 8u;
  t.tiles_per_xcd = 0;
  if (t.n_tiles >= 8 && t.n_tiles % 8u == 0) {
    t.tiles_per_xcd = t.n_tiles / 8u;
    t.blocks_per_xcd = (t.tiles_per_xcd * n_qw + waves_per_block - 1) / waves_per_block;
  }
  t.groups = std::min(t.n_tiles, max_groups);
  return t;
}
