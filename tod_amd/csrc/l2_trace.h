// Diagnostics (TODHIP_L2_TRACE, tools/l2_wave_times.py): the report of the (start, end) ticks, 100 MHz, that every wave of the float
// matcher's pass 2 left in the partition buffer. Host code; included by l2.hip.
#pragma once
#include <algorithm>
#include <cstdio>
#include <vector>

#include "ctx.h"
#include "l2_plan.h"

// waits for the stream, so only a diagnostics run calls it
static int l2_trace_report(todhip_ctx* ctx, const void* d_trace, uint32_t q_blocks, uint32_t n_chunks) {
  const size_t n_waves = (size_t)q_blocks * n_chunks * kWaves;
  std::vector<uint64_t> tr(2 * n_waves);
  TOD_HIP(hipStreamSynchronize(ctx->stream));
  TOD_HIP(hipMemcpy(tr.data(), d_trace, tr.size() * 8, hipMemcpyDeviceToHost));
  uint64_t t0 = ~0ull, t1 = 0;
  for (size_t i = 0; i < n_waves; ++i) { t0 = std::min(t0, tr[2 * i]); t1 = std::max(t1, tr[2 * i + 1]); }
  std::vector<double> start(n_waves), end(n_waves);
  for (size_t i = 0; i < n_waves; ++i) { start[i] = (tr[2 * i] - t0) * 0.01; end[i] = (tr[2 * i + 1] - t0) * 0.01; }
  std::sort(start.begin(), start.end()); std::sort(end.begin(), end.end());
  auto pct = [&](const std::vector<double>& v, double p) { return v[(size_t)(p * (v.size() - 1))]; };
  for (uint32_t y = 0; y < q_blocks; ++y) {
    double sum = 0; size_t cnt = 0; double byx[8] = {0}; size_t nx[8] = {0}; double byw[4] = {0};
    for (uint32_t x = 0; x + 1 < n_chunks; ++x) for (uint32_t w = 0; w < kWaves; ++w) {
      const double e = (tr[2 * (((size_t)y * n_chunks + x) * kWaves + w) + 1] - t0) * 0.01;
      sum += e; ++cnt; byx[x & 7] += e; ++nx[x & 7]; byw[w] += e;
    }
    fprintf(stderr, "[todhip l2 trace]   query block %u: mean end %.1f us; by chunk %% 8:", y, sum / cnt);
    for (int i = 0; i < 8; ++i) fprintf(stderr, " %.1f", byx[i] / nx[i]);
    fprintf(stderr, "; by wave:");
    for (int i = 0; i < 4; ++i) fprintf(stderr, " %.1f", byw[i] / (cnt / 4));
    fprintf(stderr, "\n");
  }
  fprintf(stderr, "[todhip l2 trace] pass 2: %zu waves, span %.1f us; wave start p50 %.1f p99 %.1f max %.1f us; wave end min %.1f p10 %.1f p50 %.1f p90 %.1f max %.1f us\n",
          n_waves, (t1 - t0) * 0.01, pct(start, 0.5), pct(start, 0.99), start.back(), end.front(), pct(end, 0.1), pct(end, 0.5), pct(end, 0.9), end.back());
  return TODHIP_OK;
}
