// The three table- and word-based forms of stage A's arithmetic against the per-pixel statements they replaced (host, no GPU):
//   resize_taps (tod_amd/csrc/orb_plan.h) against the expressions resize_kernel evaluated for every pixel, for every destination
//     index of the pyramid steps of 640 x 480 and 1920 x 1080, of tiny and odd sizes, and of dst == src - 1 for src in 8..80; indices
//     inside [0, src), weights inside [0, 2048] and summing to 2048; and the plan's tap table: its regions are disjoint, the column
//     taps are padded to whole groups of four with the last column's;
//   compass4 (orb_compass.h) against fast_compass position by position: exhaustively around the two thresholds (the centre p in
//     0..255, every ring value in {p - 22 .. p - 19, p + 19 .. p + 22, 0, 255} clipped to 0..255), on 10^6 seeded random windows,
//     always with four different positions so that a mix-up of lanes shows; and through window4 on a random staged tile, indexed
//     as pass 1 of fast_nms_kernel indexes it;
//   row_moments (orb_moments.h) against the byte loop of patch_moments on random, all-255 and all-0 patches of 31 x 31 pixels, every
//     row's half-width from disc_umax.
// Prints "<taps compared> <compass positions compared> <patch rows compared>"; exits 1 at the first difference.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "orb_compass.h"
#include "orb_moments.h"
#include "orb_plan.h"

using namespace tod_orb;

#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); return false; } } while (0)

static uint32_t rng_state = 0x9E3779B9u;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- the resize
static long n_taps = 0;
static bool check_taps(uint32_t sn, uint32_t dn) {
  std::vector<ResizeTap> taps(dn);
  resize_taps(sn, dn, taps.data());
  for (uint32_t x = 0; x < dn; ++x, ++n_taps) {
    // as they stood in resize_kernel
    const float sx = (float)sn / (float)dn;
    const float fx = ((float)x + 0.5f) * sx - 0.5f;
    const int x0 = (int)floorf(fx);
    const int wx = (int)rintf((fx - (float)x0) * 2048.f);
    const int xa = clampi(x0, 0, (int)sn - 1), xb = clampi(x0 + 1, 0, (int)sn - 1);
    const ResizeTap& t = taps[x];
    if (!(t.a == (uint32_t)xa && t.b == (uint32_t)xb && t.wb == (uint32_t)wx && t.wa == (uint32_t)(2048 - wx) && t.a < sn && t.b < sn &&
          t.wb <= 2048u && t.wa <= 2048u)) {
      std::printf("resize_taps(%u, %u)[%u]: %u %u %u %u, expected %d %d %d %d\n", sn, dn, x, t.a, t.b, t.wa, t.wb, xa, xb, 2048 - wx, wx);
      return false;
    }
  }
  return true;
}
static bool check_tap_table(uint32_t H, uint32_t W, uint32_t n_levels, float sf) {
  OrbPlan P;
  CHECK(orb_plan(2, H, W, 500, n_levels, sf, 500, &P) == TODHIP_OK);
  const ResizeTap none = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  std::vector<ResizeTap> taps(P.n_taps, none), one;
  fill_resize_taps(P, taps.data());
  uint32_t end = 0;                                        // the regions follow each other: columns, then rows, level by level
  for (uint32_t l = 0; l < (uint32_t)kMaxLevels; ++l) {
    if (P.resize_x[l] == 0u) { CHECK(P.resize[l].x == 0u && P.resize[l].y == 0u && P.resize[l].z == 0u); continue; }
    const uint32_t h = P.tab.h[l], w = P.tab.w[l], wpad = (w + 3u) / 4u * 4u;
    CHECK(l > 0 && P.tap_x[l] == end && P.tap_x[l] % 4u == 0u && P.tap_y[l] == P.tap_x[l] + wpad && P.tap_y[l] + h <= P.n_taps);
    end = P.tap_y[l] + (h + 3u) / 4u * 4u;
    CHECK(P.resize[l].x * 4u * kResizeGroups >= w && (P.resize[l].x - 1u) * 4u * kResizeGroups < w);
    CHECK(P.resize[l].y * kResizeRows >= h && (P.resize[l].y - 1u) * kResizeRows < h && P.resize[l].z == 2u);
    one.resize(w); resize_taps(P.tab.w[l - 1], w, one.data());
    for (uint32_t x = 0; x < wpad; ++x) CHECK(std::memcmp(&taps[P.tap_x[l] + x], &one[x < w ? x : w - 1u], sizeof(ResizeTap)) == 0);
    one.resize(h); resize_taps(P.tab.h[l - 1], h, one.data());
    for (uint32_t y = 0; y < h; ++y) CHECK(std::memcmp(&taps[P.tap_y[l] + y], &one[y], sizeof(ResizeTap)) == 0);
  }
  CHECK(end == P.n_taps);
  return true;
}

// ---- the compass test
static long n_compass = 0;
// four positions, each with its own centre and ring pixels v[i] = {p, ring 0, ring 4, ring 8, ring 12}
static bool check_compass(const uint8_t (&v)[4][5]) {
  uint32_t word[5] = {0, 0, 0, 0, 0};
  for (int i = 0; i < 4; ++i)
    for (int k = 0; k < 5; ++k) word[k] |= (uint32_t)v[i][k] << (8 * i);
  const uint32_t m = compass4(word[0], word[1], word[2], word[3], word[4]);
  for (int i = 0; i < 4; ++i, ++n_compass) {
    uint8_t img[7 * 7];
    std::memset(img, v[i][0], sizeof(img));
    img[6 * 7 + 3] = v[i][1]; img[3 * 7 + 6] = v[i][2]; img[0 * 7 + 3] = v[i][3]; img[3 * 7 + 0] = v[i][4];   // c[3 W], c[3], c[-3 W], c[-3]
    const bool ref = fast_compass(img + 3 * 7 + 3, 7);
    if (((m >> i) & 1u) != (ref ? 1u : 0u) || (m >> 4) != 0u) {
      std::printf("compass4: position %d, p %d ring %d %d %d %d: mask %x, fast_compass %d\n", i, v[i][0], v[i][1], v[i][2], v[i][3], v[i][4], m, (int)ref);
      return false;
    }
  }
  return true;
}
static bool check_compass_thresholds() {
  for (int p = 0; p < 256; ++p) {
    // position i has the centre p + 37 i and walks the 10^4 ring combinations from its own starting point
    for (int c = 0; c < 10000; ++c) {
      uint8_t v[4][5];
      for (int i = 0; i < 4; ++i) {
        const int pi = (p + 37 * i) & 255;
        const int ring[10] = {pi - 22, pi - 21, pi - 20, pi - 19, pi + 19, pi + 20, pi + 21, pi + 22, 0, 255};
        int ci = (c + 2357 * i) % 10000;
        v[i][0] = (uint8_t)pi;
        for (int k = 1; k < 5; ++k, ci /= 10) v[i][k] = (uint8_t)clampi(ring[ci % 10], 0, 255);
      }
      if (!check_compass(v)) return false;
    }
  }
  return true;
}
static bool check_compass_random() {
  for (int n = 0; n < 1000000; ++n) {
    uint8_t v[4][5];
    for (int i = 0; i < 4; ++i) {
      const uint32_t a = rnd(), b = rnd();
      v[i][0] = (uint8_t)a; v[i][1] = (uint8_t)(a >> 8); v[i][2] = (uint8_t)(a >> 16); v[i][3] = (uint8_t)(a >> 24); v[i][4] = (uint8_t)b;
      if (n & 1)                                           // half of the windows near the centre value, where the thresholds are
        for (int k = 1; k < 5; ++k) v[i][k] = (uint8_t)clampi((int)v[i][0] + (int)(v[i][k] % 61u) - 30, 0, 255);
    }
    if (!check_compass(v)) return false;
  }
  return true;
}
// a staged tile as fast_nms_kernel's s_img: rows of kImgDw words; scored position (px, py) has its centre at byte px + 3 of row py + 3
static bool check_compass_windows() {
  constexpr int kImgDw = 18, kImgW = 4 * kImgDw, kImgH = 24, kScoreW = 66, kScoreH = 18, kGroups = 17;
  for (int rep = 0; rep < 200; ++rep) {
    uint32_t s_img[kImgH * kImgDw];
    for (uint32_t& wd : s_img) {
      wd = rnd();
      if (rep & 1) wd = (wd & 0x1F1F1F1Fu) + 0x70707070u;  // low contrast: both outcomes are common
    }
    uint8_t px_of[kImgH * kImgW];
    std::memcpy(px_of, s_img, sizeof(px_of));              // (little-endian, as the device)
    for (int py = 0; py < kScoreH; ++py)
      for (int g = 0; g < kGroups; ++g) {
        const uint32_t* c = s_img + (py + 3) * kImgDw + g;
        const uint32_t *up = c - 3 * kImgDw, *dn = c + 3 * kImgDw;
        // (a row's last group reads the next row's first word for the two positions past the row's end)
        const uint32_t m = compass4(window4(c[0], c[1], 3), window4(dn[0], dn[1], 3), window4(c[1], c[2], 2), window4(up[0], up[1], 3), c[0]);
        for (int i = 0; i < 4 && 4 * g + i < kScoreW; ++i, ++n_compass) {
          const bool ref = fast_compass(px_of + (py + 3) * kImgW + 4 * g + i + 3, kImgW);
          if (((m >> i) & 1u) != (ref ? 1u : 0u)) { std::printf("windows: row %d group %d position %d: mask %x, fast_compass %d\n", py, g, i, m, (int)ref); return false; }
        }
      }
  }
  return true;
}

// ---- the moments
static long n_rows = 0;
static bool check_moments(int kind) {
  int umax[kHalfPatch + 2];
  disc_umax(umax);
  constexpr int W = 40;                                    // a patch inside a wider image: pixels outside the disc are there and differ
  uint8_t img[31 * W + 8];
  for (uint8_t& b : img) b = kind == 0 ? (uint8_t)rnd() : (kind == 1 ? 255 : 0);
  const int x = 17, y = 15;
  int m10 = 0, m01 = 0, r10 = 0, r01 = 0;
  for (int l = 0; l < 31; ++l, ++n_rows) {
    const int v = l - kHalfPatch;
    const int d = v == 0 ? kHalfPatch : umax[v < 0 ? -v : v];
    int rs = 0, row10 = 0;                                 // as they stood in patch_moments
    for (int u = -d; u <= d; ++u) {
      const int px = img[(size_t)(y + v) * W + x + u];
      row10 += u * px;
      rs += px;
    }
    int rs4, row10_4;
    row_moments(img + (size_t)(y + v) * W + x - kHalfPatch, d, rs4, row10_4);
    if (rs4 != rs || row10_4 != row10) { std::printf("row_moments: kind %d row %d d %d: %d %d, expected %d %d\n", kind, v, d, rs4, row10_4, rs, row10); return false; }
    r10 += row10; r01 += v * rs; m10 += row10_4; m01 += v * rs4;
  }
  CHECK(m10 == r10 && m01 == r01);
  return true;
}

int main() {
  const uint32_t pairs[][2] = {{640, 533}, {533, 444}, {480, 400}, {400, 333}, {1920, 1600}, {1080, 900}, {8, 7}, {9, 8}, {63, 53}};
  for (const auto& p : pairs)
    if (!check_taps(p[0], p[1])) return 1;
  for (uint32_t src = 8; src <= 80; ++src)
    if (!check_taps(src, src - 1)) return 1;
  if (!check_tap_table(480, 640, 3, 1.2f) || !check_tap_table(1080, 1920, 8, 1.2f) || !check_tap_table(70, 75, 3, 1.2f) ||
      !check_tap_table(9, 8, 16, 2.0f) || !check_tap_table(480, 640, 1, 1.2f))
    return 1;
  if (!check_compass_thresholds() || !check_compass_random() || !check_compass_windows()) return 1;
  for (int rep = 0; rep < 2000; ++rep)
    if (!check_moments(0)) return 1;
  if (!check_moments(1) || !check_moments(2)) return 1;
  std::printf("%ld %ld %ld\n", n_taps, n_compass, n_rows);
  return 0;
}
