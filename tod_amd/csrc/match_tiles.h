// The DB tiles of the matrix-core searches (host, plain C++; included by ctx.h). Each launcher brings its own, measured wish.
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
