// rescale_depth (Trainer.cpp:62-81; the detection side does the same in ecto_opencv's RescaledRegisteredDepth, detector.py:26,62):
// THE statement of its arithmetic -- the geometry of the resize (host) and the value of one pixel of the rescaled image (host and
// device). rescale_depth_kernel (train.hip) writes rescaled_depth_at for every pixel; the verifier's cluster kernel (verify_prep.h)
// evaluates it at the keypoint pixels only, so that no H x W image exists between a sensor-sized depth image and the poses. Both
// must give the same bytes: plain C++ float and double expressions, no fused multiply-add (the library is built with
// -ffp-contract=off), nothing from a math library but floor.
// Plain C++ as well: tests/depth_rescale_host_test.cpp includes this header into a host program.
//
// cv::rescaleDepth to float metres, then -- when the depth image is not of the image size -- a resize into the top
// int(dH * factor) rows of an H x W image, the rest NaN. The reference's call
// cv::resize(depth, subregion, subregion.size(), CV_INTER_NN) (:78) hands CV_INTER_NN (== 0) to the `fx` parameter,
// so what it EXECUTES is cv::resize's default, bilinear interpolation; `nearest` selects what its comment (:77)
// intends. Both follow cv::resize's float path (third-party arithmetic, recalled; parity unpinned):
//   nearest : source = floor(x * (1 / (dst / src))) clamped to the last column / row, in double
//   bilinear: f = (float)((x + 0.5) * (src / dst) - 0.5), s = floor(f), f -= s; s < 0 -> s = 0, f = 0; s + 1 >= src
//             width -> the single tap S[src - 1] * 1; rows: the two row indices are clamped, the weights are kept;
//             out = (S00 * (1 - fx) + S01 * fx) * (1 - fy) + (S10 * (1 - fx) + S11 * fx) * fy in float, no fma
//             (a NaN tap poisons the pixel even under a zero weight, as in the reference).
//   exact 2x shrink: cv::resize turns INTER_LINEAR into its INTER_AREA fast path: (S00 + S01 + S10 + S11) * 0.25f.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define TOD_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TOD_HD inline
#endif

namespace tod {

// what rescale_geometry decides once per image pair; mode: kEqual conversion only (:68-71), kNearest, kBilinear, kShrink2
struct RescaleGeom {
  enum { kEqual = 0, kNearest = 1, kBilinear = 2, kShrink2 = 3 };
  uint32_t dH, dW, sub_rows;                                         // the source's size; rows >= sub_rows of the result are NaN
  int mode;
  double sx, sy;                                                     // source pixels per result pixel
};

// host part of rescale_depth: the geometry of the resize. Returns false when cv::Mat::rowRange / cv::resize would throw.
inline bool rescale_geometry(uint32_t dH, uint32_t dW, uint32_t H, uint32_t W, int nearest, RescaleGeom* g) {
  g->dH = dH; g->dW = dW;
  if (dH == H && dW == W) { g->sub_rows = H; g->mode = RescaleGeom::kEqual; g->sx = 1.0; g->sy = 1.0; return true; }
  const float factor = (float)W / (float)dW;                     // :73
  const int rows = (int)((float)dH * factor);                    // rowRange(0, dsize.height * factor), :76
  if (rows <= 0 || (uint32_t)rows > H) return false;
  g->sub_rows = (uint32_t)rows;
  const double inv_x = (double)W / (double)dW, inv_y = (double)rows / (double)dH;   // cv::resize: inv_scale = dst / src
  g->mode = nearest ? RescaleGeom::kNearest : ((dW == 2u * W && dH == 2u * (uint32_t)rows) ? RescaleGeom::kShrink2 : RescaleGeom::kBilinear);
  g->sx = 1.0 / inv_x; g->sy = 1.0 / inv_y;                      // ifx (nearest) == scale_x (bilinear) == 1 / inv_scale
  return true;
}

TOD_HD float depth_metres(const void* src, int is_u16, size_t i) {
  if (!is_u16) return reinterpret_cast<const float*>(src)[i];
  const uint16_t d = reinterpret_cast<const uint16_t*>(src)[i];
  return d ? (float)d * 0.001f : __builtin_nanf("");                 // cv::rescaleDepth
}

TOD_HD int rescale_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// pixel (x, y) of the rescaled image; x < W and y < H of the geometry's result size are the caller's to hold
TOD_HD float rescaled_depth_at(const void* src, int is_u16, const RescaleGeom& g, uint32_t x, uint32_t y) {
  const uint32_t dH = g.dH, dW = g.dW;
  float z = __builtin_nanf("");
  if (y < g.sub_rows) {
    if (g.mode == RescaleGeom::kEqual) {                             // sizes equal: conversion only (:68-71)
      z = depth_metres(src, is_u16, (size_t)y * dW + x);
    } else if (g.mode == RescaleGeom::kNearest) {
      const uint32_t fx = (uint32_t)floor((double)x * g.sx), fy = (uint32_t)floor((double)y * g.sy);
      const uint32_t sx = fx < dW - 1u ? fx : dW - 1u, sy = fy < dH - 1u ? fy : dH - 1u;
      z = depth_metres(src, is_u16, (size_t)sy * dW + sx);
    } else if (g.mode == RescaleGeom::kShrink2) {                    // exact 2x shrink
      const size_t o = (size_t)(2u * y) * dW + 2u * x;
      z = (depth_metres(src, is_u16, o) + depth_metres(src, is_u16, o + 1) + depth_metres(src, is_u16, o + dW) +
           depth_metres(src, is_u16, o + dW + 1)) * 0.25f;
    } else {                                                         // bilinear
      float fx = (float)(((double)x + 0.5) * g.sx - 0.5), fy = (float)(((double)y + 0.5) * g.sy - 0.5);
      int sx = (int)floorf(fx), sy = (int)floorf(fy);
      fx -= (float)sx; fy -= (float)sy;
      if (sx < 0) { sx = 0; fx = 0.f; }
      const bool one_tap = sx + 1 >= (int)dW;
      if (one_tap) sx = (int)dW - 1;
      const int sy0 = rescale_clampi(sy, 0, (int)dH - 1), sy1 = rescale_clampi(sy + 1, 0, (int)dH - 1);
      float h0, h1;
      if (one_tap) {
        h0 = depth_metres(src, is_u16, (size_t)sy0 * dW + sx) * 1.f;
        h1 = depth_metres(src, is_u16, (size_t)sy1 * dW + sx) * 1.f;
      } else {
        const float a0 = 1.f - fx, a1 = fx;
        h0 = depth_metres(src, is_u16, (size_t)sy0 * dW + sx) * a0 + depth_metres(src, is_u16, (size_t)sy0 * dW + sx + 1) * a1;
        h1 = depth_metres(src, is_u16, (size_t)sy1 * dW + sx) * a0 + depth_metres(src, is_u16, (size_t)sy1 * dW + sx + 1) * a1;
      }
      z = h0 * (1.f - fy) + h1 * fy;
    }
  }
  return z;
}

}  // namespace tod
