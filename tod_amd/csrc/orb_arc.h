// The arc search of the FAST-9/16 score on 16-bit pairs, and the entries of fast_nms_kernel's survivor list (host and device, plain
// C++, no HIP include: included by orb_fast.h, tested stand-alone by tests/orb_nms_host_test.cpp against the per-arc statement of
// the score and against every position of a tile).
//
// The score of a pixel is the largest t for which 9 contiguous ring pixels are all brighter than p + t or all darker than p - t:
// with the differences d[i] = ring[i] - p, max(0, max over the 16 arcs of min d, max over the 16 arcs of min -d). min(-d) is
// -max(d), so both polarities come from the same 16 differences: the brighter one is the largest sliding minimum, the darker one
// minus the smallest sliding maximum. A difference lies in [-255, 255], so 16 bits hold it exactly, and a register holds ring
// elements i and i + 8 in its two halves: the cyclic ring is 8 registers, element k >= 8 is register k - 8 with its halves swapped,
// and a sliding window over the 16 starting points is 8 packed operations.
#pragma once
#include <cstdint>

#include "orb_compass.h"

namespace tod_orb {

#if defined(__HIP_DEVICE_COMPILE__)
typedef short pair16 __attribute__((ext_vector_type(2)));
TOD_ORB_HD pair16 pk_min(pair16 a, pair16 b) { return __builtin_elementwise_min(a, b); }
TOD_ORB_HD pair16 pk_max(pair16 a, pair16 b) { return __builtin_elementwise_max(a, b); }
TOD_ORB_HD pair16 pk_swap(pair16 a) { return __builtin_shufflevector(a, a, 1, 0); }
TOD_ORB_HD int pk_lo(pair16 a) { return a.x; }
TOD_ORB_HD int pk_hi(pair16 a) { return a.y; }
// (lo - p, hi - p) of two pixels lo, hi and the centre pixel p in both halves of pp
TOD_ORB_HD pair16 pk_diff(uint32_t lo, uint32_t hi, uint32_t pp) {
  return __builtin_bit_cast(pair16, lo | (hi << 16)) - __builtin_bit_cast(pair16, pp);
}
#else
struct pair16 { int16_t x, y; };
TOD_ORB_HD pair16 pk_min(pair16 a, pair16 b) { return {a.x < b.x ? a.x : b.x, a.y < b.y ? a.y : b.y}; }
TOD_ORB_HD pair16 pk_max(pair16 a, pair16 b) { return {a.x > b.x ? a.x : b.x, a.y > b.y ? a.y : b.y}; }
TOD_ORB_HD pair16 pk_swap(pair16 a) { return {a.y, a.x}; }
TOD_ORB_HD int pk_lo(pair16 a) { return a.x; }
TOD_ORB_HD int pk_hi(pair16 a) { return a.y; }
TOD_ORB_HD pair16 pk_diff(uint32_t lo, uint32_t hi, uint32_t pp) {
  return {(int16_t)((int)lo - (int)(pp & 0xFFFFu)), (int16_t)((int)hi - (int)(pp >> 16))};
}
#endif

template <bool kMin> TOD_ORB_HD pair16 pk_pick(pair16 a, pair16 b) { return kMin ? pk_min(a, b) : pk_max(a, b); }
// element k (taken mod 16) of a cyclic sequence held as 8 pairs (i, i + 8), as a pair (k, k + 8)
TOD_ORB_HD pair16 ring_at(const pair16 (&v)[8], int k) { return (k & 8) ? pk_swap(v[k & 7]) : v[k & 7]; }

// kMin: the largest, over the 16 arcs of 9 contiguous elements, of the arc's minimum; else the smallest of the arcs' maxima.
// Sliding windows of 2, 4, 8, then 9 elements, as the 32-bit form had them.
template <bool kMin> TOD_ORB_HD int arc9_fold(const pair16 (&d)[8]) {
  pair16 m2[8], m4[8], best = {};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < 8; ++i) m2[i] = pk_pick<kMin>(d[i], ring_at(d, i + 1));
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < 8; ++i) m4[i] = pk_pick<kMin>(m2[i], ring_at(m2, i + 2));
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < 8; ++i) {
    const pair16 m9 = pk_pick<kMin>(pk_pick<kMin>(m4[i], ring_at(m4, i + 4)), ring_at(d, i + 8));
    best = i ? pk_pick<!kMin>(best, m9) : m9;
  }
  const int lo = pk_lo(best), hi = pk_hi(best);
  return kMin ? (lo > hi ? lo : hi) : (lo < hi ? lo : hi);
}

// the FAST-9/16 score from the ring's differences, d[i] = (ring[i] - p, ring[i + 8] - p): 0 unless it is above the threshold
TOD_ORB_HD int fast_score_pairs(const pair16 (&d)[8]) {
  const int bright = arc9_fold<true>(d), dark = -arc9_fold<false>(d);
  const int best = bright > dark ? bright : dark;
  return best > kFastThr ? best : 0;
}

// An entry of fast_nms_kernel's survivor list: the scored position (px, py) of a tile, px in [0, row_w) with row_w <= 128. The
// entries of a group of four neighbours are the first one's + 0 .. 3.
TOD_ORB_HD uint32_t nms_entry(int px, int py) { return ((uint32_t)py << 7) | (uint32_t)px; }
TOD_ORB_HD int nms_entry_px(uint32_t e) { return (int)(e & 127u); }
TOD_ORB_HD int nms_entry_py(uint32_t e) { return (int)(e >> 7); }

}  // namespace tod_orb
