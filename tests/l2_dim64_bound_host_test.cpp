// The float matcher's filter bound (tod_amd/csrc/l2_bound.h) at 64 dimensions (desc_bytes 256), on the host against extended
// precision: tests/l2_bound_host_test.cpp's checks and families at the narrower width, with the norms summed in
// l2_prepare_narrow_kernel's order. The constants of eps(q) are the 128-wide ones; this program is what says they hold here.
//   score(q, r) = |r|^2 + <bf16(-2 q), bf16(r)>      the bf16 x bf16 products exact, |r|^2 the sum of squares of the f32 row
//   (a) |score + |q|^2 - d2| <= eps(q)               for every pair, d2 both the defining sequential f32 sum over 64 dimensions and exact
//   (b) score(r1) - score(r2) - (d2(r1) - d2(r2)) <= 2 eps(q)   for every two rows of a case
//   (c) the worst-case families reach more than 0.9 of eps: the bound is no slacker here than at 128
// eps(q) = tod::l2_eps(|q|^2, Rmax^2), both norms in f32 in the narrow prepare kernel's order: lane l holds v[l]^2, then the six
// butterfly steps s += shfl_xor(s, 32 ... 1); lane 0's value.
// Worst-case families: every component one f32 ulp beside a bf16 rounding boundary (or on it), signs such that all 2 x 64 first-order
// error terms of <q^, r^> add up. Random cases: signed, integer, sparse, wide-exponent and RootSIFT-like vectors, seeded.
//
//   l2_dim64_bound_host_test                               the checks; prints counts and the largest used fraction of eps; exit 1 on a failure
//   l2_dim64_bound_host_test --plan-widths                 l2_plan (l2_plan.h) at the two widths on l2_plan_host_test.cpp's grid; prints the cases
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "l2_bound.h"
#include "l2_plan.h"

namespace {

constexpr int kD = 64;
static_assert(kD == (int)kDimNarrow, "the narrower descriptor width");
static_assert(l2_dim_of(256) == 64 && l2_dim_of(512) == 128 && l2_dim_of(64) == 0 && l2_dim_of(1024) == 0, "the two float widths");
static_assert(l2_tile_loads(64) == 5 && l2_tile_loads(128) == 9 && l2_ring_slot_bytes(64) == 32 * 64 * 2 + 256 &&
              l2_ring_slot_bytes(128) == kRingSlotBytes, "one tile's loads and ring slot, from the width");
typedef long double real;
struct Vec { float v[kD]; };

float bf16_value(float x) { const uint32_t b = (uint32_t)tod::l2_bf16_rne(x) << 16; return __builtin_bit_cast(float, b); }

// |v|^2 in f32 as l2_prepare_narrow_kernel sums it
float norm2_device_order(const Vec& x) {
  float s[64], t[64];
  for (int l = 0; l < 64; ++l) s[l] = x.v[l] * x.v[l];
  for (int off = 32; off > 0; off >>= 1) {
    for (int l = 0; l < 64; ++l) t[l] = s[l] + s[l ^ off];
    memcpy(s, t, sizeof s);
  }
  return s[0];
}

real norm2_exact(const Vec& x) { real s = 0; for (int i = 0; i < kD; ++i) s += (real)x.v[i] * (real)x.v[i]; return s; }

real score(const Vec& q, const Vec& r) {
  real dot = 0;
  for (int i = 0; i < kD; ++i) dot += (real)bf16_value(-2.0f * q.v[i]) * (real)bf16_value(r.v[i]);
  return norm2_exact(r) + dot;
}

float d2_f32(const Vec& q, const Vec& r) {                  // the definition (include/todhip.h), dim = 64
  float acc = 0.f;
  for (int i = 0; i < kD; ++i) { const float t = q.v[i] - r.v[i]; const float tt = t * t; acc = acc + tt; }
  return acc;
}

real d2_exact(const Vec& q, const Vec& r) {
  real s = 0;
  for (int i = 0; i < kD; ++i) { const real t = (real)q.v[i] - (real)r.v[i]; s += t * t; }
  return s;
}

struct Tally {
  long pairs = 0, row_pairs = 0, bad_a = 0, bad_b = 0;
  double worst_ratio = 0, worst_diff_ratio = 0;             // largest |error| / eps and (differential error) / (2 eps)
};

void check_case(const Vec& q, const std::vector<Vec>& rows, Tally& t, const char* what) {
  float rmax2 = 0.f;
  for (const Vec& r : rows) rmax2 = fmaxf(rmax2, norm2_device_order(r));
  const real eps = (real)tod::l2_eps(norm2_device_order(q), rmax2), q2 = norm2_exact(q);
  std::vector<real> err(rows.size());
  for (size_t i = 0; i < rows.size(); ++i) {
    const real sc = score(q, rows[i]);
    err[i] = sc + q2 - (real)d2_f32(q, rows[i]);
    const real err_exact = sc + q2 - d2_exact(q, rows[i]);
    const real worst = fmaxl(fabsl(err[i]), fabsl(err_exact));
    ++t.pairs;
    if (eps > 0 && (double)(worst / eps) > t.worst_ratio) t.worst_ratio = (double)(worst / eps);
    if (!(worst <= eps)) {
      if (t.bad_a++ < 3) fprintf(stderr, "(a) fails, %s row %zu: error %.6Lg (exact d2: %.6Lg), eps %.6Lg\n", what, i, err[i], err_exact, eps);
    }
  }
  for (size_t i = 0; i < rows.size(); ++i)
    for (size_t j = 0; j < rows.size(); ++j) {
      if (i == j) continue;
      const real diff = err[i] - err[j];
      ++t.row_pairs;
      if (eps > 0 && (double)(diff / (2 * eps)) > t.worst_diff_ratio) t.worst_diff_ratio = (double)(diff / (2 * eps));
      if (!(diff <= 2 * eps)) {
        if (t.bad_b++ < 3) fprintf(stderr, "(b) fails, %s rows %zu, %zu: differential error %.6Lg, 2 eps %.6Lg\n", what, i, j, diff, 2 * eps);
      }
    }
}

// the f32 one ulp below (dir < 0) / above (dir > 0) / exactly on (dir == 0) the boundary between the bf16 values of mantissa m and
// m + 1 (m = 0..126) at 2^e
float beside_boundary(int m, int e, int dir) {
  const float mid = ldexpf(1.0f + (2 * m + 1) / 256.0f, e);
  return dir < 0 ? nextafterf(mid, 0.f) : dir > 0 ? nextafterf(mid, INFINITY) : mid;
}

// l2_bound_host_test.cpp's family at 64 dimensions: `down` components that round down, then components that round up, the last `free`
// dimensions 0; low row: every error term positive; high = -low; an adjusted row; a row of half the norm
void worst_case(int m, int e, int down, int free, int scale_r, bool exact, Tally& t) {
  Vec q{}, low{}, high{};
  const int used = kD - free;
  for (int i = 0; i < used; ++i) {
    const bool dn = i < down;
    float c;
    if (exact) c = beside_boundary(dn ? (m & ~1) : (m | 1), e, 0);
    else c = beside_boundary(m, e, dn ? -1 : 1);
    q.v[i] = c;
    low.v[i] = ldexpf(dn ? -c : c, scale_r);
    high.v[i] = -low.v[i];
  }
  std::vector<Vec> rows{low, high};
  if (free) { Vec adj = low; adj.v[kD - 1] = ldexpf(1.0f, e + scale_r); rows.push_back(adj); }
  Vec half = high;
  for (int i = 0; i < kD; ++i) half.v[i] *= 0.5f;
  rows.push_back(half);
  check_case(q, rows, t, "worst-case family");
}

struct Rng {                                                // xorshift64*
  uint64_t s;
  uint64_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 0x2545F4914F6CDD1Dull; }
  float unit() { return (float)(next() >> 40) * (1.0f / 16777216.0f); }
  float signed_unit() { return 2.0f * unit() - 1.0f; }
};

void random_vec(Rng& g, int kind, Vec& x) {
  for (int i = 0; i < kD; ++i) {
    switch (kind) {
      case 0: x.v[i] = g.signed_unit(); break;                                          // signed (SURF, KAZE)
      case 1: x.v[i] = floorf(g.unit() * 256.0f); break;                                // integers
      case 2: x.v[i] = g.unit() < 0.8f ? 0.0f : g.signed_unit(); break;                 // sparse, with zeros
      case 3: x.v[i] = ldexpf(g.signed_unit(), (int)(g.next() % 40u) - 20); break;      // exponents spread over 2^-20 .. 2^20
      default: x.v[i] = g.unit(); break;                                                // non-negative
    }
  }
  if (kind == 4) {
    const float n = sqrtf(norm2_device_order(x));
    for (int i = 0; i < kD; ++i) x.v[i] = sqrtf(x.v[i]) / sqrtf(n * 8.0f);
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--plan-widths")) {
    // on tests/l2_plan_host_test.cpp's grid: l2_plan without the trailing argument is l2_plan at 128 in every field, and l2_plan at 64
    // differs from it in q_bf16_bytes alone, which is halved. Prints the number of cases.
    const uint32_t tile_sample = 256u * 32u;
    const uint32_t rows[] = {1, 2, 31, 32, 33, 255u * 32u, tile_sample, tile_sample + 1u, 8u * tile_sample - 1u, 8u * tile_sample, 65504, 65505,
                             65535, 65536, 65537, 70000, 500000, 1u << 24};
    const uint32_t nqs[] = {1, 511, 512, 513, 1000, 16000};
    const uint32_t cus[] = {1, 64, 256, 304};
    L2Knobs knob_sets[6];
    knob_sets[1].chunk_rounds = 3; knob_sets[2].sample_tiles = 512; knob_sets[3].seed_chunks = 7; knob_sets[4].seed_chunks = 1000000;
    knob_sets[5].no_candidates = true;
    auto same_but_q = [](const L2Plan& a, const L2Plan& b) {
      return a.nq_pad == b.nq_pad && a.q_blocks == b.q_blocks && a.n_tiles == b.n_tiles && a.n_chunks == b.n_chunks &&
             a.tiles_per_chunk == b.tiles_per_chunk && a.n_parts == b.n_parts && a.seed_pass == b.seed_pass && a.fast == b.fast &&
             a.sample_tiles == b.sample_tiles && a.sample_stride == b.sample_stride && a.s_chunks == b.s_chunks && a.s_tpc == b.s_tpc &&
             a.s_used == b.s_used && a.kt0 == b.kt0 && a.kt1 == b.kt1 && a.k_eff == b.k_eff && a.margin == b.margin &&
             a.keys_bytes == b.keys_bytes && a.cand_cnt_bytes == b.cand_cnt_bytes && a.flags_bytes == b.flags_bytes &&
             a.q_eps_bytes == b.q_eps_bytes && a.q_norm_bytes == b.q_norm_bytes && a.thr_bytes == b.thr_bytes && a.seed_bytes == b.seed_bytes &&
             a.scan_marks_bytes == b.scan_marks_bytes && a.cand_bytes == b.cand_bytes && a.slots_bytes == b.slots_bytes &&
             a.slot_cnt_bytes == b.slot_cnt_bytes && a.part_bytes == b.part_bytes;
    };
    unsigned long cases = 0;
    for (uint32_t n : rows) for (uint32_t nq : nqs) for (uint32_t k = 1; k <= 8; ++k) for (uint32_t n_cu : cus) for (const L2Knobs& kn : knob_sets) {
      const L2Plan dflt = l2_plan(n, nq, k, n_cu, kn), wide = l2_plan(n, nq, k, n_cu, kn, kDim), narrow = l2_plan(n, nq, k, n_cu, kn, kDimNarrow);
      const bool ok = same_but_q(dflt, wide) && dflt.q_bf16_bytes == wide.q_bf16_bytes && same_but_q(wide, narrow) &&
                      narrow.q_bf16_bytes * 2 == wide.q_bf16_bytes && narrow.q_bf16_bytes == (size_t)narrow.nq_pad * kDimNarrow * 2;
      if (!ok) { fprintf(stderr, "n_rows %u nq %u k %u n_cu %u: the plans of the two widths differ beyond q_bf16_bytes\n", n, nq, k, n_cu); return 1; }
      ++cases;
    }
    printf("%lu\n", cases);
    return 0;
  }
  if (argc > 1) { fprintf(stderr, "unknown argument %s\n", argv[1]); return 2; }

  Tally worst, rnd;
  const int mantissas[] = {0, 1, 2, 31, 64, 126};
  const int exponents[] = {-40, -20, -1, 0, 3, 20, 40};
  const int downs[] = {0, 31, 32, 62, 64};
  for (int m : mantissas)
    for (int e : exponents)
      for (int down : downs)
        for (int free : {0, 2})
          for (int scale_r : {-6, 0, 5})
            for (bool exact : {false, true}) worst_case(m, e, down > kD - free ? kD - free : down, free, scale_r, exact, worst);

  Rng g{0x9E3779B97F4A7C15ull};
  for (int c = 0; c < 600; ++c) {                           // 600 cases x 8 rows = 4800 pairs
    Vec q;
    std::vector<Vec> rows(8);
    random_vec(g, c % 5, q);
    for (Vec& r : rows) random_vec(g, (c / 5) % 5, r);
    if (c % 3 == 0) for (int i = 0; i < kD; ++i) rows[0].v[i] = q.v[i] + 0.01f * g.signed_unit() * q.v[i];   // a near neighbour
    if (c % 7 == 0) for (int i = 0; i < kD; ++i) rows[1].v[i] *= 1000.0f;                                   // an Rmax row far out
    check_case(q, rows, rnd, "random case");
  }

  printf("worst-case families: %ld pairs, %ld ordered row pairs, (a) fails %ld, (b) fails %ld, largest |error| / eps %.4f, "
         "largest differential error / 2 eps %.4f\n", worst.pairs, worst.row_pairs, worst.bad_a, worst.bad_b, worst.worst_ratio,
         worst.worst_diff_ratio);
  printf("random cases: %ld pairs, %ld ordered row pairs, (a) fails %ld, (b) fails %ld, largest |error| / eps %.4f, "
         "largest differential error / 2 eps %.4f\n", rnd.pairs, rnd.row_pairs, rnd.bad_a, rnd.bad_b, rnd.worst_ratio, rnd.worst_diff_ratio);
  const bool tight = worst.worst_ratio > 0.9;               // (c)
  if (!tight) fprintf(stderr, "(c) fails: the worst-case families reach only %.4f of eps\n", worst.worst_ratio);
  return tight && worst.bad_a + worst.bad_b + rnd.bad_a + rnd.bad_b == 0 ? 0 : 1;
}
