// Lowe's ratio test against another object (todhip_ratio_other_device, include/todhip.h): THE statement of its predicate, of
// the limit a query's search may stop at, and of the rows of an object inside a window of searched rows. match_other.hip evaluates
// these functions on the device and on the host; tests/ratio_other_host_test.cpp includes this header into a host program. Plain C++.
//
// other(q, o) is the least Hamming distance from query q to a searched row that does not belong to object o, kRatioOtherNone when
// there is no such row. A query whose nearest kept match is at distance d1 in object o1 survives iff there is no other object's row,
// or (float)d1 < ratio * (float)other(q, o1): the comparison of the classic test (todhip_set_ratio_test), in binary32, with the
// second neighbour taken from another object.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define TOD_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TOD_HD inline
#endif

namespace tod {

constexpr uint32_t kRatioOtherNone = 0xFFFFFFFFu;             // "no row of another object", and "no limit"

// (float)d1 < ratio * (float)other, one multiplication rounded to binary32 (the library is built without contraction)
TOD_HD bool ratio_other_passes(uint32_t d1, float ratio, uint32_t other) {
  const float rhs = ratio * (float)other;
  return (float)d1 < rhs;
}

// the predicate
TOD_HD bool ratio_other_survives(uint32_t d1, float ratio, uint32_t other) {
  return other == kRatioOtherNone || ratio_other_passes(d1, ratio, other);
}

// The least integer L with ratio_other_passes(d1, ratio, L), 0 < ratio <= 1: every other >= L passes (the right-hand side does not
// fall as `other` grows), every other < L fails, so a search for other(q, o) may stop at L. L >= 1 (d1 >= 0 is not below 0), and
// kRatioOtherNone where L would not fit 32 bits (a ratio near 0): no limit, which is always safe.
TOD_HD uint32_t ratio_other_limit(uint32_t d1, float ratio) {
  const double guess = (double)d1 / (double)ratio;
  if (!(guess < 4.0e9)) return kRatioOtherNone;
  uint32_t L = (uint32_t)guess;                                 // within a few units of the answer: binary32's rounding decides
  while (L > 0u && ratio_other_passes(d1, ratio, L - 1u)) --L;
  while (!ratio_other_passes(d1, ratio, L)) ++L;
  return L;
}

// Rows [lo, hi) of some numbering, seen from a window of n rows that starts at row `first` of that numbering: the window-local rows
// [lo', hi') of the intersection, lo' == hi' when it is empty. An object's rows in a shard (first = shard_first, n = shard_rows) and an
// excluded interval in a DB tile (first = the tile's first searched row, n = its rows) are both this.
struct RowInterval { uint32_t lo, hi; };
TOD_HD RowInterval ratio_other_clamp(uint64_t lo, uint64_t hi, uint64_t first, uint64_t n) {
  const uint64_t end = first + n;
  const uint64_t a = lo < first ? first : lo, b = hi > end ? end : hi;
  if (a >= b) return RowInterval{0u, 0u};
  return RowInterval{(uint32_t)(a - first), (uint32_t)(b - first)};
}

// is window-local row r outside the interval? (one subtraction, one unsigned comparison: the form the DB pass walks a block with)
TOD_HD bool ratio_other_counts(uint32_t r, RowInterval iv) { return r - iv.lo >= iv.hi - iv.lo; }

}  // namespace tod
