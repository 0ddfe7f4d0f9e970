// Stage A's launch plan (host, plain C++, no HIP include; included by orb_stages.h; tested stand-alone by tests/orb_plan_host_test.cpp):
// the constants and records the kernels and the host share, the pyramid's geometry, and OrbPlan -- every buffer capacity, the layout of
// the control block, the grid extent of every launch and the resize's tap tables, from the call's seven numbers. The floats of
// features_per_level and level_table decide pyramid sizes, those of resize_taps the pixels of every resized level, and the CPU
// restatement must reproduce both bit for bit: their expressions do not change.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/todhip.h"

namespace tod_orb {

constexpr int kEdge = 31;
constexpr int kHalfPatch = 15;
constexpr int kMaxLevels = 16;
constexpr int kPatternRadius2 = 13 * 13;   // every pattern point: x^2 + y^2 <= 169, so a rotated, rounded point stays inside the patch
// The `pattern` argument's domain (include/todhip.h at todhip_orb): x^2 + y^2 <= 900. A keypoint is kEdge = 31 pixels inside its level,
// a rotation keeps a point's distance from the centre and rintf of a coordinate of magnitude <= 30 (+ a few float roundings) is <= 30,
// so every steered test reads a pixel of the keypoint's own level; the 31 x 31 square of cv::ORB patterns (|x|, |y| <= 15) is inside.
constexpr int kPatternDomainRadius2 = 30 * 30;

struct Cand { int x, y, score; float harris; };

// Control words (device): what the selection kernels hand to each other without a host round trip. One row of kCtlWords per
// (level, frame) with the W_* words below, then one row per frame where word [kLevelCountWord + l] = keypoints of level l, then a
// row of per-frame totals (OrbPlan: cnt_off, level_counts_off, totals_off).
constexpr uint32_t kCtlWords = 512;
enum { W_NCAND = 0, W_NSEL1 = 1, W_THR = 2, W_NEED_EQ = 3, W_NEQ = 4, W_NGT = 5, W_WANT = 6, W_HIST = 32 };
constexpr uint32_t kLevelCountWord = 8;

// geometry of the pyramid levels; want[l] == 0: the level yields nothing (too small, or no features asked of it)
struct LevelTab {
  uint32_t n_levels, F;
  const uint8_t* img[kMaxLevels];                          // level l of frame 0 (frame stride: the level-0 pixel count)
  uint32_t h[kMaxLevels], w[kMaxLevels], want[kMaxLevels];
  float scale[kMaxLevels];
};

// the pixel tiles of the two tiled kernels (orb_fast.h, orb_pyramid.h): a block of fast_nms_kernel, a block of blur_kernel
constexpr int kNmsTileW = 64, kNmsTileH = 16;
constexpr int kBlurTileW = 128, kBlurTileH = 64;

// same generator as the CPU restatement: seeded xorshift, points inside radius 13
inline void default_pattern(int8_t* pat) {
  uint32_t s = 0x9E3779B9u;
  for (int i = 0; i < 256 * 2; ++i) {
    int x, y;
    do {
      s ^= s << 13; s ^= s >> 17; s ^= s << 5;
      x = (int)(s % 27u) - 13;
      s ^= s << 13; s ^= s >> 17; s ^= s << 5;
      y = (int)(s % 27u) - 13;
    } while (x * x + y * y > 13 * 13);
    pat[2 * i] = (int8_t)x;
    pat[2 * i + 1] = (int8_t)y;
  }
}

inline void disc_umax(int* umax) {
  const int hp = kHalfPatch;
  const int vmax = (int)std::floor(hp * std::sqrt(2.0) / 2 + 1), vmin = (int)std::ceil(hp * std::sqrt(2.0) / 2);
  for (int v = 0; v <= vmax; ++v) umax[v] = (int)std::rint(std::sqrt((double)hp * hp - (double)v * v));
  for (int v = hp, v0 = 0; v >= vmin; --v) {
    while (umax[v0] == umax[v0 + 1]) ++v0;
    umax[v] = v0;
    ++v0;
  }
}

inline void features_per_level(uint32_t n_features, uint32_t n_levels, float scale_factor, uint32_t* out) {
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

// a caller's pattern (256 x 4 int8, or null for the built-in one) inside its domain: checked wherever a pattern enters the library,
// before anything is launched or stored
inline int check_pattern(const int8_t* pattern) {
  if (!pattern) return TODHIP_OK;
  for (int i = 0; i < 256 * 2; ++i) {
    const int x = pattern[2 * i], y = pattern[2 * i + 1];
    if (x * x + y * y > kPatternDomainRadius2) return TODHIP_EINVAL;
  }
  return TODHIP_OK;
}

// what every form refuses before it touches the device or the caller's memory; (level, frame) pairs ride in a grid dimension
inline int check_args(uint32_t F, uint32_t H, uint32_t W, uint32_t n_features, uint32_t n_levels, float scale_factor, uint32_t cap) {
  if (n_levels == 0 || n_levels > (uint32_t)kMaxLevels || !(scale_factor > 1.f) || H < 8 || W < 8 || n_features == 0 || F == 0 ||
      F > 65535u || (size_t)n_levels * F > 65535u)
    return TODHIP_EINVAL;
  return cap == 0 ? TODHIP_ECAPACITY : TODHIP_OK;
}

// the pyramid of one geometry: sizes, scales and how many keypoints each level is asked for. A level too small for a keypoint
// (down to 0 x 0 pixels, where the scale has outgrown the image) stays in the table with want == 0. Returns the largest want.
inline uint32_t level_table(uint32_t H, uint32_t W, uint32_t F, uint32_t n_features, uint32_t n_levels, float scale_factor, LevelTab* T) {
  uint32_t per_level[kMaxLevels], want_max = 0;
  features_per_level(n_features, n_levels, scale_factor, per_level);
  std::memset(T, 0, sizeof(*T));
  T->n_levels = n_levels; T->F = F;
  for (uint32_t lvl = 0; lvl < n_levels; ++lvl) {
    float scale = 1.f;
    for (uint32_t i = 0; i < lvl; ++i) scale = scale * scale_factor;
    const uint32_t w = (uint32_t)rintf((float)W / scale), h = (uint32_t)rintf((float)H / scale);
    T->h[lvl] = h; T->w[lvl] = w; T->scale[lvl] = scale;
    T->want[lvl] = (h <= 2u * kEdge || w <= 2u * kEdge) ? 0u : per_level[lvl];     // too small: the level count stays 0
    want_max = std::max(want_max, T->want[lvl]);
  }
  return want_max;
}

// One axis of the bilinear resize, per destination index: the two source indices, clamped into the source, and their 11-bit weights
// (wa + wb = 2048), laid out as the kernel uses them: one 16-byte load and no arithmetic. The sample position is
// (i + 0.5) * (src_n / dst_n) - 0.5 in floats; these expressions are the CPU restatement's, term for term, and must not be contracted
// or reassociated. They depend on the geometry alone, so resize_kernel reads them from tables that are filled once per geometry
// instead of dividing and rounding for every pixel.
struct ResizeTap { uint32_t a, b, wa, wb; };
inline void resize_taps(uint32_t src_n, uint32_t dst_n, ResizeTap* taps) {
  const float s = (float)src_n / (float)dst_n;
  for (uint32_t i = 0; i < dst_n; ++i) {
    const float f = ((float)i + 0.5f) * s - 0.5f;
    const int i0 = (int)floorf(f);
    const int w = (int)rintf((f - (float)i0) * 2048.f);
    taps[i].a = (uint32_t)std::min(std::max(i0, 0), (int)src_n - 1); taps[i].b = (uint32_t)std::min(std::max(i0 + 1, 0), (int)src_n - 1);
    taps[i].wa = (uint32_t)(2048 - w); taps[i].wb = (uint32_t)w;
  }
}

// the pixel tile of a block of resize_kernel: a lane writes four neighbouring pixels of a row
constexpr uint32_t kResizeGroups = 16, kResizeRows = 16;

// One call's sizes and grids. (level l, frame f) is virtual frame l F + f: it owns slice l F + f of every per-level buffer and row
// l F + f of the control block, and rides in the last grid dimension of every launch.
struct OrbGrid { uint32_t x, y, z; };
struct OrbPlan {
  uint32_t F, H, W, n_levels, cap;                         // as asked
  size_t px, V;                                            // pixels of a level-0 frame = the frame stride of every image buffer; virtual frames
  uint32_t cand_cap, sel1_cap, sel2_cap;                   // records per virtual frame: candidates (and ties), the 2n best by score, the n best
  size_t ctl_words, cnt_off, level_counts_off, totals_off; // the control block and, in words, its per-frame rows, their level counts, the totals
  uint32_t want_max;                                       // 0: no level can hold a keypoint, nothing is launched
  LevelTab tab;                                            // img[] stays null here: the workspace's owner fills it in
  OrbGrid copy_rows, fast_nms, fast_threshold, split, rank_ties, harris, rank_harris, blur, describe, copy_out;
  uint32_t resize_x[kMaxLevels];                           // level l's pixels in blocks of 256; 0: no resize launch (level 0, or no pixels)
  OrbGrid resize[kMaxLevels];                              // level l's resize launch where resize_x[l] != 0: tiles across, tiles down, frames
  uint32_t tap_x[kMaxLevels], tap_y[kMaxLevels], n_taps;   // of such a level: where its column and row taps start in the tap table; its size
};

// the tap table of a plan: the column taps of every resized level, padded to whole groups of four with copies of the last column's
// (a lane's four taps are always there and always name pixels of the source), and its row taps
inline void fill_resize_taps(const OrbPlan& P, ResizeTap* taps) {
  for (uint32_t lvl = 1; lvl < P.n_levels; ++lvl) {
    if (P.resize_x[lvl] == 0u) continue;
    const uint32_t w = P.tab.w[lvl];
    resize_taps(P.tab.w[lvl - 1], w, taps + P.tap_x[lvl]);
    for (uint32_t i = w; i < (w + 3u) / 4u * 4u; ++i) taps[P.tap_x[lvl] + i] = taps[P.tap_x[lvl] + w - 1u];
    resize_taps(P.tab.h[lvl - 1], P.tab.h[lvl], taps + P.tap_y[lvl]);
  }
}

// check_args' status; *P is filled when that is TODHIP_OK
inline int orb_plan(uint32_t F, uint32_t H, uint32_t W, uint32_t n_features, uint32_t n_levels, float scale_factor, uint32_t cap,
                    OrbPlan* P) {
  if (const int bad = check_args(F, H, W, n_features, n_levels, scale_factor, cap)) return bad;
  P->F = F; P->H = H; P->W = W; P->n_levels = n_levels; P->cap = cap;
  P->px = (size_t)H * W; P->V = (size_t)n_levels * F;
  P->cand_cap = (uint32_t)(P->px / 4 + 64); P->sel1_cap = 2u * n_features + 16u; P->sel2_cap = n_features + 16u;
  P->ctl_words = (P->V + F + 1) * kCtlWords;
  P->cnt_off = P->V * kCtlWords; P->level_counts_off = P->cnt_off + kLevelCountWord; P->totals_off = P->cnt_off + (size_t)F * kCtlWords;
  P->want_max = level_table(H, W, F, n_features, n_levels, scale_factor, &P->tab);
  const uint32_t Vg = (uint32_t)P->V;
  P->copy_rows = {(uint32_t)((P->px + 255) / 256), F, 1u};
  P->n_taps = 0;
  for (uint32_t lvl = 0; lvl < (uint32_t)kMaxLevels; ++lvl) {
    const uint32_t hw = lvl < n_levels ? P->tab.h[lvl] * P->tab.w[lvl] : 0u;
    P->resize_x[lvl] = (lvl > 0 && hw > 0u) ? (hw + 255u) / 256u : 0u;
    P->resize[lvl] = {0u, 0u, 0u}; P->tap_x[lvl] = P->tap_y[lvl] = 0u;
    if (P->resize_x[lvl] == 0u) continue;
    const uint32_t h = P->tab.h[lvl], w = P->tab.w[lvl], groups = (w + 3u) / 4u;
    P->resize[lvl] = {(groups + kResizeGroups - 1u) / kResizeGroups, (h + kResizeRows - 1u) / kResizeRows, F};
    P->tap_x[lvl] = P->n_taps; P->tap_y[lvl] = P->n_taps + 4u * groups;      // both start on a group of four
    P->n_taps = P->tap_y[lvl] + (h + 3u) / 4u * 4u;
  }
  P->fast_nms = {(W + kNmsTileW - 1) / kNmsTileW, (H + kNmsTileH - 1) / kNmsTileH, Vg};
  P->fast_threshold = {Vg, 1u, 1u};
  P->split = P->rank_ties = {(P->cand_cap + 255u) / 256u, Vg, 1u};
  P->harris = P->rank_harris = {(2u * P->want_max + 255u) / 256u, Vg, 1u};
  P->blur = {(W + kBlurTileW - 1) / kBlurTileW, (H + kBlurTileH - 1) / kBlurTileH, Vg};
  P->describe = {(P->want_max + 3u) / 4u, Vg, 1u};
  P->copy_out = {(8u * cap + 255u) / 256u, F, 1u};
  return TODHIP_OK;
}

}  // namespace tod_orb
