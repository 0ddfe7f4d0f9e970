// The filters of the float matcher (todhip_set_l2_ratio_test, todhip_cross_check_l2_device; definitions: include/todhip.h): THE
// statement of the ratio predicate, and of how a squared distance becomes the integer that cross_check.h's predicate compares.
// l2_finalize_kernel and l2_merge_knn_kernel<K> (l2.hip) evaluate l2_ratio_passes on the device, cross_check.hip's float kernel
// compares l2_d2_bits; tests/l2_filters_host_test.cpp includes this header into a host program. Plain C++.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "cross_check.h"   // TOD_HD

namespace tod {

// a value todhip_set_l2_ratio_test takes: 0 (off) or 0 < ratio <= 1. NaN fails every comparison.
TOD_HD bool l2_ratio_valid(float ratio) { return ratio == 0.f || (ratio > 0.f && ratio <= 1.f); }

// Lowe's test on a query's two nearest rows, d2_1 <= d2_2 their exact squared distances: dist = sqrtf(d2) in binary32, and the query
// keeps its matches iff dist1 < ratio * dist2 -- one binary32 product, nothing to fuse it with. Two rows at equal distance fail at
// every ratio <= 1.
TOD_HD bool l2_ratio_passes(float d2_1, float d2_2, float ratio) {
  const float bound = ratio * sqrtf(d2_2);
  return sqrtf(d2_1) < bound;
}

// The same on the first two keys of a query's ascending list, (binary32 bits of d2) << 32 | row, ~0 = no such row: a query with fewer
// than two rows to its name passes.
TOD_HD float l2_key_d2(uint64_t key) {
  const uint32_t bits = (uint32_t)(key >> 32);
  float d2;
  memcpy(&d2, &bits, sizeof d2);
  return d2;
}
TOD_HD bool l2_ratio_keeps(uint64_t key1, uint64_t key2, float ratio) {
  return key1 == ~0ull || key2 == ~0ull || l2_ratio_passes(l2_key_d2(key1), l2_key_d2(key2), ratio);
}

// d(q, g) of the float cross-check: the bits of a d2 >= 0 (never -0: the sum starts at +0 and adds squares), whose order as unsigned
// integers is the order of the values -- cross_check_beats applies to them unchanged.
TOD_HD uint32_t l2_d2_bits(float d2) {
  uint32_t bits;
  memcpy(&bits, &d2, sizeof bits);
  return bits;
}

}  // namespace tod
