// tod_amd/csrc/ratio_other.h in a stand-alone host program (tests/test_ratio_other_cpu.py builds it with -fsanitize=address,undefined):
// the predicate, the limit against brute force, and the clamp of an object's rows to a shard and to a DB tile.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ratio_other.h"

#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

using tod::kRatioOtherNone;
using tod::RowInterval;

static bool same(RowInterval a, uint32_t lo, uint32_t hi) { return a.lo == lo && a.hi == hi; }

// the rows of [lo, hi) that a window shows, one by one
static bool clamp_equals_rows(uint64_t lo, uint64_t hi, uint64_t first, uint64_t n) {
  const RowInterval iv = tod::ratio_other_clamp(lo, hi, first, n);
  if (iv.lo > iv.hi || iv.hi > n) return false;
  for (uint64_t r = 0; r < n; ++r) {
    const bool inside = first + r >= lo && first + r < hi;
    if (tod::ratio_other_counts((uint32_t)r, iv) == inside) return false;
  }
  return true;
}

int main() {
  // ---- the predicate
  CHECK(tod::ratio_other_survives(0, 0.8f, kRatioOtherNone));
  CHECK(tod::ratio_other_survives(512, 0.5f, kRatioOtherNone));
  CHECK(!tod::ratio_other_survives(4, 0.5f, 8));                  // 4 < 4.0 fails
  CHECK(tod::ratio_other_survives(4, 0.5f, 9));
  CHECK(!tod::ratio_other_survives(6, 0.75f, 8));                 // 6 < 6.0 fails
  CHECK(tod::ratio_other_survives(5, 0.75f, 8));
  CHECK(!tod::ratio_other_survives(0, 1.0f, 0));                  // an exact copy in another object
  CHECK(tod::ratio_other_survives(0, 1.0f, 1));
  CHECK(!tod::ratio_other_survives(8, 1.0f, 8) && tod::ratio_other_survives(7, 1.0f, 8));
  CHECK(!tod::ratio_other_survives(4, 0.8f, 5) && tod::ratio_other_survives(3, 0.8f, 5));   // 4 < 4.0 fails in binary32
  std::printf("predicate\n");

  // ---- the limit: the least L that passes, against every (d1, d) up to 512
  const float ratios[] = {0.5f, 0.75f, 0.8f, 1.0f};
  for (float ratio : ratios) {
    for (uint32_t d1 = 0; d1 <= 512; ++d1) {
      const uint32_t L = tod::ratio_other_limit(d1, ratio);
      uint32_t brute = kRatioOtherNone;
      for (uint32_t d = 0; d <= 2048 && brute == kRatioOtherNone; ++d)
        if (tod::ratio_other_passes(d1, ratio, d)) brute = d;
      CHECK(L == brute);
      CHECK(L >= 1 && L >= d1);
      for (uint32_t d = 0; d <= 512; ++d) {
        CHECK(tod::ratio_other_passes(d1, ratio, d) == (d >= L));  // monotone: the search may stop at L
        // what the filter computes, min(other, L), decides as other itself does
        CHECK(tod::ratio_other_survives(d1, ratio, d < L ? d : L) == tod::ratio_other_survives(d1, ratio, d));
      }
      CHECK(tod::ratio_other_survives(d1, ratio, L));              // no other object: min(NONE, L) = L survives as NONE does
    }
    std::printf("limit %g\n", (double)ratio);
  }
  CHECK(tod::ratio_other_limit(4, 0.5f) == 9 && tod::ratio_other_limit(6, 0.75f) == 9 && tod::ratio_other_limit(0, 0.8f) == 1);
  CHECK(tod::ratio_other_limit(35, 0.8f) == 44 && tod::ratio_other_limit(256, 1.0f) == 257);
  // ratios near 0: no 32-bit limit, or a huge one that still is the least
  CHECK(tod::ratio_other_limit(512, 1e-30f) == kRatioOtherNone);
  CHECK(tod::ratio_other_limit(0, 1e-30f) == 1);
  {
    const uint32_t L = tod::ratio_other_limit(300, 1e-6f);
    CHECK(L != kRatioOtherNone && tod::ratio_other_passes(300, 1e-6f, L) && !tod::ratio_other_passes(300, 1e-6f, L - 1));
  }
  std::printf("limit extremes\n");

  // ---- the clamp: an object's rows in a shard
  CHECK(same(tod::ratio_other_clamp(97, 354, 0, 1059), 97, 354));     // unsharded
  CHECK(same(tod::ratio_other_clamp(97, 354, 97, 962), 0, 257));      // the shard begins with the object
  CHECK(same(tod::ratio_other_clamp(97, 354, 64, 290), 33, 290));     // ... ends with it
  CHECK(tod::ratio_other_clamp(97, 354, 354, 705).lo == tod::ratio_other_clamp(97, 354, 354, 705).hi);   // another shard's object
  CHECK(tod::ratio_other_clamp(97, 354, 0, 97).lo == tod::ratio_other_clamp(97, 354, 0, 97).hi);
  CHECK(tod::ratio_other_clamp(0, 0, 0, 1059).lo == tod::ratio_other_clamp(0, 0, 0, 1059).hi);           // an empty object
  CHECK(tod::ratio_other_clamp(354, 354, 300, 100).lo == tod::ratio_other_clamp(354, 354, 300, 100).hi);
  CHECK(tod::ratio_other_clamp(10, 20, 0, 0).lo == tod::ratio_other_clamp(10, 20, 0, 0).hi);             // a shard without rows
  // an object straddling a tile: rows 97 .. 353 over tiles of 288 rows
  CHECK(same(tod::ratio_other_clamp(97, 354, 0, 288), 97, 288));
  CHECK(same(tod::ratio_other_clamp(97, 354, 288, 288), 0, 66));
  CHECK(same(tod::ratio_other_clamp(359, 1059, 864, 195), 0, 195));   // the DB's last, short tile, all of it excluded
  // beyond 32 bits of rows in the full numbering
  CHECK(same(tod::ratio_other_clamp(0xFFFFFF00ull, 0xFFFFFFF0ull, 0xFFFFFF80ull, 0x100), 0, 0x70));
  // every window of a small world, row by row (empty objects, empty windows, objects around both ends)
  for (uint64_t lo = 0; lo <= 12; ++lo)
    for (uint64_t hi = lo; hi <= 12; ++hi)
      for (uint64_t first = 0; first <= 12; ++first)
        for (uint64_t n = 0; first + n <= 13; ++n) CHECK(clamp_equals_rows(lo, hi, first, n));
  // the walk's test on rows a wave meets outside its tile: the unsigned wrap of "the step before the first"
  {
    const RowInterval none = tod::ratio_other_clamp(0, 0, 0, 288), all = tod::ratio_other_clamp(0, 288, 0, 288);
    CHECK(tod::ratio_other_counts(0u, none) && tod::ratio_other_counts(287u, none) && tod::ratio_other_counts(0xFFFFFFE4u, none));
    CHECK(!tod::ratio_other_counts(0u, all) && !tod::ratio_other_counts(287u, all) && tod::ratio_other_counts(288u, all));
  }
  std::printf("clamp\n");
  std::printf("ok\n");
  return 0;
}
