// The optional bit order of the resident Hamming DB (todhip_set_db_bit_order, include/todhip.h): which of a descriptor's 256 bit
// positions the stored rows hold first. Plain host C++ without HIP, so that it can be compiled, run and sanitized on the CPU
// (tests/bit_order_host_test.cpp); the statistics it reads and the kernels that apply its result are db_bitorder.hip's.
// No reference lines: the reference has no such step. The greedy walk is the ORB paper's (Rublee et al. 2011, 4.3) with one fixed
// threshold.
//
// Bit i of a descriptor is bit i % 8 (LSB first) of byte i / 8, i.e. bit i % 32 of the little-endian dword i / 32.
#pragma once

#include <algorithm>
#include <cstdint>

// Statistics of S sample rows (1 <= S <= 65536): ones[b] = rows with bit b set, both[a * 256 + b] = rows with bits a and b both set
// (both[b * 256 + b] == ones[b]). All arithmetic is u64: with counts of real rows v <= S^2 / 4 = 2^30 and, by Cauchy-Schwarz,
// c(a, b)^2 <= v[a] v[b], so every term below stays <= 2^62.
//   v[b] = ones[b] (S - ones[b])                               (S^2 x the bit's variance)
//   candidates: v descending, ties by ascending b
//   b is accepted iff v[b] > 0 and, for every a accepted before it, 4 c(a, b)^2 < v[a] v[b] with
//   c(a, b) = |S both[a][b] - ones[a] ones[b]|                 (S^2 x the covariance: |correlation| < 1/2)
// rank[] = the accepted bits followed by the rejected ones, each in candidate order: constant bits and (near) copies of an earlier
// bit go to the back.
inline void tod_bit_order_rank(uint64_t S, const uint32_t* ones, const uint32_t* both, uint8_t rank[256]) {
  uint64_t v[256];
  int cand[256];
  for (int b = 0; b < 256; ++b) { v[b] = (uint64_t)ones[b] * (S - ones[b]); cand[b] = b; }
  std::stable_sort(cand, cand + 256, [&](int a, int b) { return v[a] > v[b]; });   // stable: ties stay in ascending b
  int acc[256], rej[256], n_acc = 0, n_rej = 0;
  for (int i = 0; i < 256; ++i) {
    const int b = cand[i];
    bool ok = v[b] > 0;
    for (int j = 0; j < n_acc && ok; ++j) {
      const int a = acc[j];
      const uint64_t x = S * (uint64_t)both[a * 256 + b], y = (uint64_t)ones[a] * ones[b];
      const uint64_t c = x > y ? x - y : y - x;
      ok = 4u * c * c < v[a] * v[b];
    }
    if (ok) acc[n_acc++] = b; else rej[n_rej++] = b;
  }
  for (int i = 0; i < n_acc; ++i) rank[i] = (uint8_t)acc[i];
  for (int i = 0; i < n_rej; ++i) rank[n_acc + i] = (uint8_t)rej[i];
}

// Where rank r is stored: position 32 E[r / 32] + r % 32. The layout serves the matrix-core engine: a lane of hamming_topk_mfma
// loads dwords 4 h .. 4 h + 3 of its row (h = lane >> 5) and MFMA step s multiplies register s of every lane, so step s covers
// dwords s and s + 4 of a row -- the evaluation order of a split block is dwords 0, 4, 1, 5, 2, 6, 3, 7, and ranks 0-63 are what
// its first instruction sees, 0-127 its first two. The vector-ALU engine tests after words 0-2, 0-3 and 0-5 and so sees ranks 0-31,
// 64-95 and 128-159 first: still exact (Hamming distance does not depend on the order), but not the best order for that engine.
constexpr int kBitOrderDword[8] = {0, 4, 1, 5, 2, 6, 3, 7};

// src_of[p] = the original bit that stored position p holds
inline void tod_bit_order_layout(const uint8_t rank[256], uint8_t src_of[256]) {
  for (int r = 0; r < 256; ++r) src_of[32 * kBitOrderDword[r / 32] + r % 32] = rank[r];
}

inline void tod_bit_order_from_stats(uint64_t S, const uint32_t* ones, const uint32_t* both, uint8_t src_of[256]) {
  uint8_t rank[256];
  tod_bit_order_rank(S, ones, both, rank);
  tod_bit_order_layout(rank, src_of);
}
