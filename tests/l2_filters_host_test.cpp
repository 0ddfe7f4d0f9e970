// Stand-alone host program over tod_amd/csrc/l2_filters.h and cross_check.h (built with -fsanitize=address,undefined by
// tests/test_l2_filters_cpu.py): the ratio predicate at its edges, the setter's domain, and cross_check.h's predicate used with the
// bits of squared distances. Prints one line per check group and "ok"; any failed check prints what failed and exits 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "cross_check.h"
#include "l2_filters.h"

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

// the defining distance, as include/todhip.h states it (this file is built without fused multiply-add: -ffp-contract=off)
static float d2_seq(const std::vector<float>& q, const std::vector<float>& r) {
  volatile float acc = 0.f;
  for (size_t i = 0; i < q.size(); ++i) {
    volatile float t = q[i] - r[i];
    volatile float p = t * t;
    acc = acc + p;
  }
  return acc;
}

static uint64_t key(float d2, uint32_t row) { return ((uint64_t)tod::l2_d2_bits(d2) << 32) | row; }

int main() {
  // the setter's domain
  CHECK(tod::l2_ratio_valid(0.f) && tod::l2_ratio_valid(1.f) && tod::l2_ratio_valid(0.5f) && tod::l2_ratio_valid(1e-30f));
  CHECK(!tod::l2_ratio_valid(-0.5f) && !tod::l2_ratio_valid(1.0000001f) && !tod::l2_ratio_valid(2.f));
  CHECK(!tod::l2_ratio_valid(std::nanf("")) && !tod::l2_ratio_valid(std::numeric_limits<float>::infinity()));
  std::printf("domain\n");

  // equal distances fail at every ratio, a zero nearest distance passes unless the second is zero too
  for (float r : {0.5f, 0.8f, 1.f}) {
    CHECK(!tod::l2_ratio_passes(25.f, 25.f, r));
    CHECK(!tod::l2_ratio_passes(0.f, 0.f, r));
    CHECK(tod::l2_ratio_passes(0.f, 16.f, r));
  }
  // the exact boundary: distances 3 and 6 at ratio 0.5 fail, 6 replaced by the next binary32 above it passes
  const float next6 = std::nextafterf(6.f, 7.f);
  CHECK(!tod::l2_ratio_passes(9.f, 36.f, 0.5f));
  CHECK(tod::l2_ratio_passes(9.f, next6 * next6, 0.5f));
  CHECK(tod::l2_ratio_passes(9.f, 36.f, 0.8f) && tod::l2_ratio_passes(9.f, 36.f, 1.f));
  // distances 9 and 11: 9 is not below 0.8 * 11
  CHECK(!tod::l2_ratio_passes(81.f, 121.f, 0.8f) && tod::l2_ratio_passes(81.f, 121.f, 1.f));
  // against the definition written out, over a grid of squared distances
  for (uint32_t a = 0; a < 40; ++a)
    for (uint32_t b = a; b < 40; ++b)
      for (float r : {0.25f, 0.5f, 0.8f, 1.f}) {
        const float d1 = std::sqrt((float)a * 1.7f), d2 = std::sqrt((float)b * 1.7f);
        volatile float bound = r * d2;
        CHECK(tod::l2_ratio_passes((float)a * 1.7f, (float)b * 1.7f, r) == (d1 < bound));
      }
  std::printf("predicate\n");

  // keys: fewer than two rows pass; the keys' distance field is the bits of d2
  CHECK(tod::l2_ratio_keeps(key(9.f, 5), ~0ull, 0.5f) && tod::l2_ratio_keeps(~0ull, ~0ull, 0.5f));
  CHECK(!tod::l2_ratio_keeps(key(9.f, 5), key(36.f, 2), 0.5f) && tod::l2_ratio_keeps(key(9.f, 5), key(36.f, 2), 0.8f));
  CHECK(!tod::l2_ratio_keeps(key(25.f, 1), key(25.f, 2), 1.f));
  CHECK(tod::l2_key_d2(key(12.5f, 77)) == 12.5f && tod::l2_key_d2(key(0.f, 0xFFFFFFFFu)) == 0.f);
  std::printf("keys\n");

  // d2 bits: +0 is 0, the order of the bits is the order of the values, and cross_check_beats on them is the (d2, q) order
  CHECK(tod::l2_d2_bits(0.f) == 0u);
  const float vals[] = {0.f, 1e-38f, 1e-20f, 0.5f, 1.f, std::nextafterf(1.f, 2.f), 12.f, 3600.f, 1e30f, std::numeric_limits<float>::infinity()};
  for (size_t i = 0; i + 1 < sizeof vals / sizeof *vals; ++i) CHECK(tod::l2_d2_bits(vals[i]) < tod::l2_d2_bits(vals[i + 1]));
  for (float da : vals)
    for (float db : vals)
      for (uint32_t qa = 0; qa < 3; ++qa)
        for (uint32_t qb = 0; qb < 3; ++qb)
          CHECK(tod::cross_check_beats(tod::l2_d2_bits(da), qa, tod::l2_d2_bits(db), qb) == (da < db || (da == db && qa < qb)));
  std::printf("bits\n");

  // the early-exit trap's three queries: one component a in dimension 0, 127 and 0 again, against the zero row -- equal sums whose
  // partial sums reach a^2 in the first and in the last step; the first takes the row from the second and keeps it against the third
  {
    std::vector<float> row(128, 0.f), q0(128, 0.f), q1(128, 0.f), q2(128, 0.f);
    q0[0] = 7.f; q1[127] = 7.f; q2[0] = 7.f;
    const uint32_t b0 = tod::l2_d2_bits(d2_seq(q0, row)), b1 = tod::l2_d2_bits(d2_seq(q1, row)), b2 = tod::l2_d2_bits(d2_seq(q2, row));
    CHECK(b0 == b1 && b1 == b2 && b0 == tod::l2_d2_bits(49.f));
    CHECK(tod::cross_check_beats(b0, 5, b1, 40) && !tod::cross_check_beats(b2, 69, b0, 5) && !tod::cross_check_beats(b1, 40, b0, 5));
  }
  std::printf("trap\n");

  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
