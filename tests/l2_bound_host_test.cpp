// The float matcher's filter bound (tod_amd/csrc/l2_bound.h) on the host, against extended precision. For a query q and the rows r of
// a DB (a "case"; Rmax = the largest row norm of the case):
//   score(q, r) = |r|^2 + <bf16(-2 q), bf16(r)>      as the matrix cores form it, but in extended precision: |r|^2 the sum of squares
//                                                    of the f32 row, the bf16 x bf16 products exact. (The f32 accumulation on the
//                                                    GPU is the only difference; tests/test_l2_numerics_gpu.py runs the same inputs.)
//   (a) |score + |q|^2 - d2| <= eps(q)               for every pair, d2 both the defining sequential f32 sum and the exact value
//   (b) score(r1) - score(r2) - (d2(r1) - d2(r2)) <= 2 eps(q)   for every two rows of a case: what the threshold A_k + 2 eps needs
//   (c) on the worst-case families the largest |error| / eps is above 0.9: the bound is not slack by an unnoticed factor
// eps(q) = tod::l2_eps(|q|^2, Rmax^2) with the two norms summed in f32 in the prepare kernel's order (a lane's two dimensions, then
// the six butterfly steps). Extended precision = long double (at least binary64: its own rounding is 2^-44 of eps or less).
//
// Worst-case families: every component sits one f32 ulp beside a bf16 rounding boundary (or exactly on it: ties to even), and the
// signs are such that all 2 x 128 first-order error terms of <q^, r^> add up. `low` rows score too low, `high` rows too high.
// Random cases: signed, non-negative, unit-norm, sparse and wide-exponent vectors from a seeded generator.
//
//   l2_bound_host_test                     run the checks; prints the counts and the largest |error| / eps; exit 1 when one fails
//   l2_bound_host_test --old-constant      the same with eps as it stood before the correction, 2^-7 (1 + 2^-6) |q| Rmax + ...:
//                                          (a) and (b) fail on the worst-case families (tests/test_l2_bound_cpu.py holds that)
//   l2_bound_host_test --eps N2 RMAX2 ...  prints l2_eps(N2, RMAX2) for each pair of f32 arguments, one %a per line
//   l2_bound_host_test --plan N_ROWS NQ K N_CU   prints what l2_plan (l2_plan.h) decides about the seed pass's sample, name and value
//                                          per line: tests/test_l2_numerics_cpu.py places its rows by it
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "l2_bound.h"
#include "l2_plan.h"

namespace {

constexpr int kD = 128;
static_assert(kD == (int)kDim, "the descriptor width");
typedef long double real;
struct Vec { float v[kD]; };

bool g_old_constant = false;

float bf16_value(float x) { const uint32_t b = (uint32_t)tod::l2_bf16_rne(x) << 16; return __builtin_bit_cast(float, b); }

// |v|^2 in f32 as l2_prepare_kernel sums it: lane l holds v[2l]^2 + v[2l+1]^2, then s += shfl_xor(s, 32 ... 1); lane 0's value
float norm2_device_order(const Vec& x) {
  float s[64], t[64];
  for (int l = 0; l < 64; ++l) { const float a = x.v[2 * l], b = x.v[2 * l + 1]; const float aa = a * a, bb = b * b; s[l] = aa + bb; }
  for (int off = 32; off > 0; off >>= 1) {
    for (int l = 0; l < 64; ++l) t[l] = s[l] + s[l ^ off];
    memcpy(s, t, sizeof s);
  }
  return s[0];
}

float eps_of(float q_norm2, float rmax2) {
  if (!g_old_constant) return tod::l2_eps(q_norm2, rmax2);
  const float nq = sqrtf(q_norm2), rmax = sqrtf(rmax2);     // the formula as it stood
  return 0.0079345703125f * nq * rmax + 6.103515625e-05f * (nq + rmax) * (nq + rmax);
}

real norm2_exact(const Vec& x) { real s = 0; for (int i = 0; i < kD; ++i) s += (real)x.v[i] * (real)x.v[i]; return s; }

real score(const Vec& q, const Vec& r) {
  real dot = 0;
  for (int i = 0; i < kD; ++i) dot += (real)bf16_value(-2.0f * q.v[i]) * (real)bf16_value(r.v[i]);
  return norm2_exact(r) + dot;
}

float d2_f32(const Vec& q, const Vec& r) {                  // the definition (include/todhip.h)
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

// checks (a) and (b) for one case
void check_case(const Vec& q, const std::vector<Vec>& rows, Tally& t, const char* what) {
  float rmax2 = 0.f;
  for (const Vec& r : rows) rmax2 = fmaxf(rmax2, norm2_device_order(r));
  const real eps = (real)eps_of(norm2_device_order(q), rmax2), q2 = norm2_exact(q);
  std::vector<real> err(rows.size());                       // against the f32 d2, which the k-NN order is made of
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
      const real diff = err[i] - err[j];                    // = score(ri) - score(rj) - (d2(ri) - d2(rj))
      ++t.row_pairs;
      if (eps > 0 && (double)(diff / (2 * eps)) > t.worst_diff_ratio) t.worst_diff_ratio = (double)(diff / (2 * eps));
      if (!(diff <= 2 * eps)) {
        if (t.bad_b++ < 3) fprintf(stderr, "(b) fails, %s rows %zu, %zu: differential error %.6Lg, 2 eps %.6Lg\n", what, i, j, diff, 2 * eps);
      }
    }
}

// ---------------------------------------------------------------------------------------------- the worst-case families
// the f32 one ulp below (dir < 0) / above (dir > 0) / exactly on (dir == 0) the boundary between the bf16 values of mantissa m and
// m + 1 (m = 0..126) at 2^e: below rounds down, above rounds up, on the boundary the even mantissa wins
float beside_boundary(int m, int e, int dir) {
  const float mid = ldexpf(1.0f + (2 * m + 1) / 256.0f, e);
  return dir < 0 ? nextafterf(mid, 0.f) : dir > 0 ? nextafterf(mid, INFINITY) : mid;
}

// q: `down` components that round down, then components that round up, the last `free` dimensions 0 (the adjusters of the GPU cases).
// low row: -q where q rounds down, +q where it rounds up, so every error term of <q^, r^> is positive and the score is too low;
// high row = -low. scale_r: a power of two on the rows. exact: components ON the boundary (m even rounds down, m odd up).
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
  if (free) { Vec adj = low; adj.v[kD - 1] = ldexpf(1.0f, e + scale_r); rows.push_back(adj); }   // bf16-exact, norm a little larger
  Vec half = high;                                          // a row of a smaller norm: Rmax, not |r|, is in eps
  for (int i = 0; i < kD; ++i) half.v[i] *= 0.5f;
  rows.push_back(half);
  check_case(q, rows, t, "worst-case family");
}

// ---------------------------------------------------------------------------------------------- random cases
struct Rng {                                                // xorshift64*: the same stream everywhere
  uint64_t s;
  uint64_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 0x2545F4914F6CDD1Dull; }
  float unit() { return (float)(next() >> 40) * (1.0f / 16777216.0f); }                 // [0, 1)
  float signed_unit() { return 2.0f * unit() - 1.0f; }
};

void random_vec(Rng& g, int kind, Vec& x) {
  for (int i = 0; i < kD; ++i) {
    switch (kind) {
      case 0: x.v[i] = g.signed_unit(); break;                                          // signed
      case 1: x.v[i] = floorf(g.unit() * 256.0f); break;                                // SIFT-like integers
      case 2: x.v[i] = g.unit() < 0.8f ? 0.0f : g.signed_unit(); break;                 // sparse, with zeros
      case 3: x.v[i] = ldexpf(g.signed_unit(), (int)(g.next() % 40u) - 20); break;      // exponents spread over 2^-20 .. 2^20
      default: x.v[i] = g.unit(); break;                                                // non-negative
    }
  }
  if (kind == 4) {                                          // RootSIFT-like: roots of non-negative values, a norm near 1
    const float n = sqrtf(norm2_device_order(x));
    for (int i = 0; i < kD; ++i) x.v[i] = sqrtf(x.v[i]) / sqrtf(n * 8.0f);
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--eps")) {
    if (argc < 4 || (argc - 2) % 2) { fprintf(stderr, "--eps takes pairs of numbers\n"); return 2; }
    for (int i = 2; i + 1 < argc; i += 2) printf("%a\n", (double)tod::l2_eps(strtof(argv[i], nullptr), strtof(argv[i + 1], nullptr)));
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "--plan")) {
    if (argc != 6) { fprintf(stderr, "--plan takes N_ROWS NQ K N_CU\n"); return 2; }
    const L2Plan P = l2_plan((uint32_t)atol(argv[2]), (uint32_t)atol(argv[3]), (uint32_t)atol(argv[4]), (uint32_t)atol(argv[5]), L2Knobs{});
    printf("tile_rows %u\nn_tiles %u\none_gemm %d\nsample_tiles %u\nsample_stride %u\ns_tpc %u\ns_used %u\nmargin %g\ncand_cap %u\nlist_cap %u\n",
           kTileRows, P.n_tiles, (int)P.one_gemm(), P.sample_tiles, P.sample_stride, P.s_tpc, P.s_used, (double)P.margin, kCandCap, kListCap);
    return 0;
  }
  g_old_constant = argc > 1 && !strcmp(argv[1], "--old-constant");
  if (argc > 1 && !g_old_constant) { fprintf(stderr, "unknown argument %s\n", argv[1]); return 2; }

  // the rounding itself: the issue's two values, ties to even, signs, zeros
  const float lo = 1.0f + 0x1p-8f - 0x1p-22f, hi = 1.0f + 0x1p-8f + 0x1p-22f;
  bool rne_ok = tod::l2_bf16_rne(lo) == 0x3F80u && tod::l2_bf16_rne(hi) == 0x3F81u && tod::l2_bf16_rne(1.0f + 0x1p-8f) == 0x3F80u &&
                tod::l2_bf16_rne(1.0f + 0x3p-8f) == 0x3F82u && tod::l2_bf16_rne(-hi) == 0xBF81u && tod::l2_bf16_rne(0.0f) == 0u &&
                tod::l2_bf16_rne(-0.0f) == 0x8000u && tod::l2_bf16_rne(-2.0f * lo) == 0xC000u;
  if (!rne_ok) fprintf(stderr, "l2_bf16_rne: a known value is wrong\n");

  Tally worst, rnd;
  const int mantissas[] = {0, 1, 2, 31, 64, 126};
  const int exponents[] = {-40, -20, -1, 0, 3, 20, 40};
  const int downs[] = {0, 63, 64, 126, 128};
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
  return rne_ok && tight && worst.bad_a + worst.bad_b + rnd.bad_a + rnd.bad_b == 0 ? 0 : 1;
}
