// OrbPlan (tod_amd/csrc/orb_plan.h) against the expressions it replaced, restated here as they stood in orb.hip: features_per_level,
// level_table and check_args, the five capacities and the control block of orb_device, the address tod_orb_stages computed by hand,
// and the grid extent at every launch site. Field by field over a sweep of image sizes around the 62-pixel limit of a level and the
// tile sizes, level counts 0..17, scale factors up to one that drives levels to 0 x 0 pixels, feature counts, capacities and batch
// sizes up to the 65535 (level, frame) pairs of a grid dimension. Then the documented rules, directly:
//   a level too small for a keypoint (h <= 2 kEdge or w <= 2 kEdge) wants nothing, every other level wants its share -- so
//   want[l] == 0 iff the level is too small, wherever the share is positive (a share can round to 0: 1 feature over 3 levels);
//   the shares sum to n_features when the last level's is positive, and so do the wants when no level is too small;
//   invalid arguments are TODHIP_EINVAL even with cap == 0, which alone is TODHIP_ECAPACITY.
// Also check_pattern and the pattern domain's reason (pattern_domain below).
// Prints "<plans compared> <calls refused>"; exits 1 at the first difference.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "orb_plan.h"

using namespace tod_orb;

// ---- as they stood in orb.hip
static void old_features_per_level(uint32_t n_features, uint32_t n_levels, float scale_factor, uint32_t* out) {
  const float factor = 1.0f / scale_factor;
  float n_desired = (float)n_features * (1.f - factor) / (1.f - powf(factor, (float)n_levels));
  int sum = 0;
  for (uint32_t l = 0; l + 1 < n_levels; ++l) {
    out[l] = (uint32_t)rintf(n_desired);
    sum += (int)out[l];
    n_desired *= factor;
  }
  const int rest = (int)n_features - sum;
  out[n_levels - 1] = rest > 0 ? (uint32_t)rest : 0u;
}
static int old_check_args(uint32_t F, uint32_t H, uint32_t W, uint32_t n_features, uint32_t n_levels, float scale_factor, uint32_t cap) {
  if (n_levels == 0 || n_levels > 16u || !(scale_factor > 1.f) || H < 8 || W < 8 || n_features == 0 || F == 0 ||
      F > 65535u || (size_t)n_levels * F > 65535u)
    return TODHIP_EINVAL;
  return cap == 0 ? TODHIP_ECAPACITY : TODHIP_OK;
}
struct OldTab { uint32_t n_levels, F, h[16], w[16], want[16]; float scale[16]; };
static uint32_t old_level_table(uint32_t H, uint32_t W, uint32_t F, uint32_t n_features, uint32_t n_levels, float scale_factor, OldTab* T) {
  uint32_t per_level[16], want_max = 0;
  old_features_per_level(n_features, n_levels, scale_factor, per_level);
  std::memset(T, 0, sizeof(*T));
  T->n_levels = n_levels; T->F = F;
  for (uint32_t lvl = 0; lvl < n_levels; ++lvl) {
    float scale = 1.f;
    for (uint32_t i = 0; i < lvl; ++i) scale = scale * scale_factor;
    const uint32_t w = (uint32_t)rintf((float)W / scale), h = (uint32_t)rintf((float)H / scale);
    T->h[lvl] = h; T->w[lvl] = w; T->scale[lvl] = scale;
    T->want[lvl] = (h <= 2u * 31 || w <= 2u * 31) ? 0u : per_level[lvl];
    want_max = std::max(want_max, T->want[lvl]);
  }
  return want_max;
}

#define CHECK(cond)                                                                                                              \
  do {                                                                                                                           \
    if (!(cond)) {                                                                                                               \
      printf("F %u H %u W %u n_features %u n_levels %u scale_factor %g cap %u: %s\n", F, H, W, nf, nl, (double)sf, cap, #cond); \
      return false;                                                                                                              \
    }                                                                                                                            \
  } while (0)

static unsigned long long n_plans = 0, n_refused = 0;

static bool one(uint32_t F, uint32_t H, uint32_t W, uint32_t nf, uint32_t nl, float sf, uint32_t cap) {
  OrbPlan P;
  std::memset(&P, 0xEE, sizeof(P));
  const int rc = orb_plan(F, H, W, nf, nl, sf, cap, &P), old_rc = old_check_args(F, H, W, nf, nl, sf, cap);
  CHECK(rc == old_rc && rc == check_args(F, H, W, nf, nl, sf, cap));
  const bool invalid = nl == 0 || nl > 16 || !(sf > 1.f) || H < 8 || W < 8 || nf == 0 || F == 0 || (unsigned long long)nl * F > 65535ull;
  CHECK(rc == (invalid ? TODHIP_EINVAL : cap == 0 ? TODHIP_ECAPACITY : TODHIP_OK));       // EINVAL before ECAPACITY
  if (rc != TODHIP_OK) { ++n_refused; return true; }
  ++n_plans;
  // ---- orb_device's sizes, as they stood
  const size_t px = (size_t)H * W;
  const uint32_t cand_cap = (uint32_t)(px / 4 + 64);
  const uint32_t sel1_cap = 2u * nf + 16u, sel2_cap = nf + 16u;
  const size_t V = (size_t)nl * F;
  OldTab T;
  const uint32_t want_max = old_level_table(H, W, F, nf, nl, sf, &T);
  CHECK(P.F == F && P.H == H && P.W == W && P.n_levels == nl && P.cap == cap);
  CHECK(P.px == px && P.V == V && P.cand_cap == cand_cap && P.sel1_cap == sel1_cap && P.sel2_cap == sel2_cap && P.want_max == want_max);
  // the control block: small.reserve((V + F + 1) * kCtlWords * 4); d_cnt = d_small + V * kCtlWords; d_totals = d_cnt + F * kCtlWords;
  // the kernels got d_cnt + 8, tod_orb_stages (F == 1) small + n_levels * kCtlWords + 8
  CHECK(P.ctl_words * sizeof(uint32_t) == (V + F + 1) * 512 * sizeof(uint32_t));
  CHECK(P.cnt_off == V * 512 && P.totals_off == V * 512 + (size_t)F * 512 && P.level_counts_off == V * 512 + 8);
  if (F == 1) CHECK(P.level_counts_off == (size_t)nl * 512 + 8);
  // the totals row is one row like the others: it holds the totals of up to kCtlWords frames (a larger batch writes behind the block
  // as sized here and at the parent -- into the slack DevBuf::reserve adds; this test pins the sizes as they are, not that)
  CHECK(P.totals_off + std::min(F, kCtlWords) <= P.ctl_words);
  // ---- the level table
  CHECK(P.tab.n_levels == nl && P.tab.F == F);
  uint32_t share[16], sum_share = 0, sum_want = 0;
  features_per_level(nf, nl, sf, share);
  bool any_small = false;
  for (uint32_t l = 0; l < 16; ++l) {
    CHECK(P.tab.img[l] == nullptr);
    if (l >= nl) { CHECK(P.tab.h[l] == 0 && P.tab.w[l] == 0 && P.tab.want[l] == 0 && P.tab.scale[l] == 0.f && P.resize_x[l] == 0); continue; }
    CHECK(P.tab.h[l] == T.h[l] && P.tab.w[l] == T.w[l] && P.tab.want[l] == T.want[l]);
    CHECK(std::memcmp(&P.tab.scale[l], &T.scale[l], sizeof(float)) == 0);
    const bool small = P.tab.h[l] <= 2u * kEdge || P.tab.w[l] <= 2u * kEdge;
    CHECK(P.tab.want[l] == (small ? 0u : share[l]));
    if (share[l] > 0) CHECK((P.tab.want[l] == 0) == small);
    any_small = any_small || small;
    sum_share += share[l]; sum_want += P.tab.want[l];
    // the resize launch: if (lvl > 0 && h * w > 0u) ... dim3((h * w + 255u) / 256u, F)
    const uint32_t h = T.h[l], w = T.w[l];
    CHECK(P.resize_x[l] == ((l > 0 && h * w > 0u) ? (h * w + 255u) / 256u : 0u));
  }
  CHECK(P.tab.h[0] == H && P.tab.w[0] == W && P.tab.scale[0] == 1.f);
  if (share[nl - 1] > 0) CHECK(sum_share == nf);
  if (share[nl - 1] > 0 && !any_small) CHECK(sum_want == nf);
  // ---- the grids, as they stood at the launch sites (tiles: 64 x 16 for fast_nms_kernel, 128 x 64 for blur_kernel)
  const uint32_t Vg = (uint32_t)V, px_blocks = (uint32_t)((px + 255) / 256);
  auto is = [](const OrbGrid& g, uint32_t x, uint32_t y, uint32_t z) { return g.x == x && g.y == y && g.z == z; };
  CHECK(is(P.copy_rows, px_blocks, F, 1));
  CHECK(is(P.fast_nms, (W + 64 - 1) / 64, (H + 16 - 1) / 16, Vg));
  CHECK(is(P.fast_threshold, Vg, 1, 1));
  CHECK(is(P.split, (cand_cap + 255u) / 256u, Vg, 1) && is(P.rank_ties, (cand_cap + 255u) / 256u, Vg, 1));
  CHECK(is(P.harris, (2u * want_max + 255u) / 256u, Vg, 1) && is(P.rank_harris, (2u * want_max + 255u) / 256u, Vg, 1));
  CHECK(is(P.blur, (W + 128 - 1) / 128, (H + 64 - 1) / 64, Vg));
  CHECK(is(P.describe, (want_max + 3u) / 4u, Vg, 1));
  CHECK(is(P.copy_out, (8u * cap + 255u) / 256u, F, 1));
  CHECK(Vg <= 65535u && F <= 65535u);                       // what rides in a grid's y or z
  return true;
}

// check_pattern: one point moved through all of int8 x int8 at the table's first, a middle and its last position is refused exactly
// when x^2 + y^2 > 900; and what the domain is for -- a point inside it, steered by any direction (cos, sin) = (m10, m01) / |m| in
// the float expressions of steer_of and steered_test, rounds to coordinates of magnitude <= 30 < kEdge, so the test reads a pixel of
// the keypoint's own level.
static bool pattern_domain() {
  int8_t pat[1024];
  default_pattern(pat);
  if (check_pattern(nullptr) != TODHIP_OK || check_pattern(pat) != TODHIP_OK) return false;
  for (int slot : {0, 2, 510, 1020, 1022})                       // byte offsets of points: the first test, a middle one, the last
    for (int x = -128; x <= 127; ++x)
      for (int y = -128; y <= 127; ++y) {
        default_pattern(pat);
        pat[slot] = (int8_t)x; pat[slot + 1] = (int8_t)y;
        const int want = x * x + y * y <= 900 ? TODHIP_OK : TODHIP_EINVAL;
        if (check_pattern(pat) != want) { printf("check_pattern: (%d, %d) at byte %d\n", x, y, slot); return false; }
      }
  static_assert(kPatternDomainRadius2 == 900 && kPatternRadius2 <= kPatternDomainRadius2 && 2 * 15 * 15 <= kPatternDomainRadius2, "domains");
  for (int x = -30; x <= 30; ++x)
    for (int y = -30; y <= 30; ++y) {
      if (x * x + y * y <= 29 * 29 || x * x + y * y > 900) continue;   // the outer ring
      for (int m10 = -2000; m10 <= 2000; m10 += 7)
        for (int m01 = -2000; m01 <= 2000; m01 += 11) {
          const float fm10 = (float)m10 * 613.f, fm01 = (float)m01 * 577.f;
          const float nrm = sqrtf(fm10 * fm10 + fm01 * fm01);
          const float ca = nrm > 0.f ? fm10 / nrm : 1.f, sa = nrm > 0.f ? fm01 / nrm : 0.f;
          const int rx = (int)rintf((float)x * ca - (float)y * sa), ry = (int)rintf((float)x * sa + (float)y * ca);
          if (std::abs(rx) > 30 || std::abs(ry) > 30) { printf("steered (%d, %d) by (%d, %d): (%d, %d)\n", x, y, m10, m01, rx, ry); return false; }
        }
    }
  return true;
}

int main() {
  if (!pattern_domain()) return 1;
  static_assert(kEdge == 31 && kMaxLevels == 16 && kCtlWords == 512 && kNmsTileW == 64 && kNmsTileH == 16 && kBlurTileW == 128 &&
                kBlurTileH == 64 && kLevelCountWord == 8, "the restated expressions above spell these out");
  const uint32_t sizes[] = {7, 8, 9, 62, 63, 64, 65, 96, 240, 480, 640, 1080, 1920};
  const uint32_t levels[] = {0, 1, 2, 3, 8, 16, 17}, features[] = {0, 1, 7, 500, 2000}, frames[] = {0, 1, 32, 65535, 65536};
  const float factors[] = {1.0f, 1.01f, 1.2f, 2.0f, 4.0f, 64.0f};
  for (uint32_t H : sizes)
    for (uint32_t W : sizes)
      for (uint32_t nl : levels)
        for (float sf : factors)
          for (uint32_t nf : features)
            for (uint32_t F : frames)
              for (uint32_t cap : {0u, 1u, nf})
                if (!one(F, H, W, nf, nl, sf, cap)) return 1;
  // n_levels * F on both sides of the limit
  const uint32_t pairs[][2] = {{1, 65535}, {3, 21845}, {15, 4369}, {5, 13107}, {16, 4095}, {16, 4096}, {2, 32768}, {4, 16384}, {8, 8192}, {3, 21846}};
  for (const auto& p : pairs)
    for (uint32_t cap : {0u, 1u, 500u})
      if (!one(p[1], 480, 640, 500, p[0], 1.2f, cap)) return 1;
  printf("%llu %llu\n", n_plans, n_refused);
  return 0;
}
