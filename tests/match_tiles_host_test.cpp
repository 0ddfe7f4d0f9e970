// mfma_tile_rows (tod_amd/csrc/match_tiles.h) against the three expressions it replaced, restated here as they stood in
// launch_topk_mfma_qt, launch_topk_mfma_q32 and launch_collect: every n_rows in 1..70 000, a spread of query waves, 256 CUs.
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

int main() {
  const uint32_t n_cu = 256, n_qws[] = {1, 2, 3, 5, 8, 11, 32, 63, 84, 125, 250, 500, 513, 4096, 4097, 8192, 8193, 100000};
  unsigned long long n = 0;
  for (uint32_t n_rows = 1; n_rows <= 70000; ++n_rows) {
    const uint32_t a = mfma_tile_rows(n_rows, n_cu * 32u, 2048u, false), b = old_q32(n_rows, n_cu);
    if (a != b) { printf("q32 n_rows %u: %u, was %u\n", n_rows, a, b); return 1; }
    ++n;
    for (uint32_t n_qw : n_qws) {
      for (uint32_t wpc : {8u, 16u, 32u, 1u, 14u, 128u}) {             // the launcher's three choices, and TODHIP_K4X_WAVES_PER_CU's
        const uint32_t c = mfma_tile_rows(n_rows, n_cu * wpc / n_qw, 256u, true), d = old_k4x(n_rows, n_cu, wpc, n_qw);
        if (c != d) { printf("K4x n_rows %u n_qw %u wpc %u: %u, was %u\n", n_rows, n_qw, wpc, c, d); return 1; }
        ++n;
      }
      const uint32_t e = mfma_tile_rows(n_rows, n_cu * 16u / n_qw, 256u, false), f = old_collect(n_rows, n_cu, n_qw);
      if (e != f) { printf("R1 n_rows %u n_qw %u: %u, was %u\n", n_rows, n_qw, e, f); return 1; }
      ++n;
    }
  }
  printf("%llu\n", n);
  return 0;
}
