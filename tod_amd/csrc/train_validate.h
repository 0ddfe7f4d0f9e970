// validateKeyPoints + depthTo3dSparse + cameraToWorld (training.cpp:57-195) for ONE keypoint: THE statement of what a training view
// does with a keypoint, shared by validate_kernel (train.hip: one view, an eroded image in memory) and validate_batch_kernel (a batch
// of device-resident views: no eroded image, no rescaled depth image). Both must give the same bytes: plain C++ integer, float and
// double expressions, no fused multiply-add (the library is built with -ffp-contract=off), nothing from a math library but rintf.
// Plain C++ as well: tests/train_validate_host_test.cpp includes this header into a host program.
//
// The eroded mask (training.cpp:69-71: cv::erode by the 3 x 3 element, 4 iterations, border value +inf) is the minimum over the 9 x 9
// window restricted to the image: eroded pixel (x, y) is open iff no mask pixel of [x - 4, x + 4] x [y - 4, y + 4], clipped to the
// image, is zero. A keypoint asks about its rounded pixel and, if that is closed, about the at most 25 pixels of the +-2 window
// around it (clipped to the image), so about a 13 x 13 neighbourhood of the mask at most: eroded_window reads that neighbourhood once
// and answers all 25 questions from a word of bits; eroded_at is the same statement for one pixel, written as the definition.
// roundWithinBounds clamps to [0, width] in the reference (:53-55), which can index one column past the image; here the clamp is to
// width - 1 / height - 1.
#pragma once
#include <cfloat>

#include "depth_rescale.h"

namespace tod {

struct TrainCam { float fx, fy, cx, cy, R[9], T[3]; };              // K's four numbers, R row-major, T

TOD_HD int train_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the definition: eroded pixel (x, y) of a packed H x W mask, 0 <= x < W, 0 <= y < H
TOD_HD bool eroded_at(const uint8_t* mask, int H, int W, int x, int y) {
  const int x0 = train_clampi(x - 4, 0, W - 1), x1 = train_clampi(x + 4, 0, W - 1);
  const int y0 = train_clampi(y - 4, 0, H - 1), y1 = train_clampi(y + 4, 0, H - 1);
  for (int yy = y0; yy <= y1; ++yy)
    for (int xx = x0; xx <= x1; ++xx)
      if (!mask[(size_t)yy * W + xx]) return false;
  return true;
}

// The 25 eroded pixels around (x, y) at once: bit 5 (dy + 2) + (dx + 2) is set iff (x + dx, y + dy) lies in the image and is open.
// Row r of the 13 x 13 neighbourhood becomes 13 bits (a pixel outside the image counts as not zero: the window is clipped), nine
// consecutive set bits starting at bit i say that row r does not close column x - 2 + i, and an eroded pixel is open when its nine
// rows all say so. The loops have constant bounds: unrolled, nothing is indexed at run time.
TOD_HD uint32_t eroded_window(const uint8_t* mask, int H, int W, int x, int y) {
  uint32_t open = 0x1FFFFFFu;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int r = 0; r < 13; ++r) {
    const int yy = y - 6 + r;
    uint32_t h = 0x1Fu;                                              // a row outside the image closes nothing
    if (yy >= 0 && yy < H) {
      uint32_t b = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (int c = 0; c < 13; ++c) {
        const int xx = x - 6 + c;
        if (xx < 0 || xx >= W || mask[(size_t)yy * W + xx]) b |= 1u << c;
      }
      const uint32_t t2 = b & (b >> 1), t4 = t2 & (t2 >> 2), t8 = t4 & (t4 >> 4);   // 2, 4, 8 consecutive set bits from bit i on
      h = t8 & (b >> 8) & 0x1Fu;
    }
    // row r lies in the nine rows of the eroded pixels of window rows j with j <= r <= j + 8
    uint32_t m = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 5; ++j) m |= ((r >= j && r <= j + 8) ? h : 0x1Fu) << (5 * j);
    open &= m;
  }
  uint32_t inside = 0;                                               // the window's pixels that exist
  for (int j = 0; j < 5; ++j)
    for (int i = 0; i < 5; ++i)
      if (x - 2 + i >= 0 && x - 2 + i < W && y - 2 + j >= 0 && y - 2 + j < H) inside |= 1u << (5 * j + i);
  return open & inside;
}
TOD_HD bool eroded_window_at(uint32_t win, int x, int y, int xx, int yy) { return (win >> (5 * (yy - y + 2) + (xx - x + 2))) & 1u; }

// the keypoint's pixel: rounded to nearest, ties to even (rintf in the default rounding mode), clamped to the image
TOD_HD void rounded_pixel(float px, float py, int H, int W, int* x, int* y) {
  *x = train_clampi((int)rintf(px), 0, W - 1);
  *y = train_clampi((int)rintf(py), 0, H - 1);
}

// The rescue of a keypoint whose pixel (*x, *y) is closed: the open eroded pixel of the +-2 window, clipped to the image, nearest
// the keypoint in float32 squared distance; among equals the lowest column, then the lowest row (columns outside, rows inside, a
// strict comparison). er(column, row) -> open? is asked about pixels of the image only. Returns false, the pixel unchanged, when
// the window holds no open pixel.
template <typename Er>
TOD_HD bool rescue_pixel(Er er, float px, float py, int H, int W, int* x, int* y) {
  const int x0 = *x, y0 = *y;
  float best = FLT_MAX;
  int bx = x0, by = y0;
  bool good = false;
  for (int ii = train_clampi(x0 - 2, 0, W - 1); ii <= train_clampi(x0 + 2, 0, W - 1); ++ii)
    for (int jj = train_clampi(y0 - 2, 0, H - 1); jj <= train_clampi(y0 + 2, 0, H - 1); ++jj)
      if (er(ii, jj)) {
        const float d = ((float)ii - px) * ((float)ii - px) + ((float)jj - py) * ((float)jj - py);
        if (d < best) { best = d; bx = ii; by = jj; good = true; }
      }
  *x = bx; *y = by;
  return good;
}

// the depth at the chosen pixel of an H x W view, in metres: geom is rescale_geometry(dH, dW -> H, W); sizes equal: the unit
// conversion only (cv::rescaleDepth), otherwise the pixel of the rescaled image without that image
TOD_HD float train_depth_at(const void* depth, int is_u16, const RescaleGeom& geom, int x, int y) {
  if (geom.mode == RescaleGeom::kEqual) return depth_metres(depth, is_u16, (size_t)y * geom.dW + x);
  return rescaled_depth_at(depth, is_u16, geom, (uint32_t)x, (uint32_t)y);
}

// cv::isValidDepth(float): everything but NaN, FLT_MAX, -FLT_MAX and FLT_MIN
TOD_HD bool valid_depth(float z) { return !(!(z == z) || z == FLT_MAX || z == -FLT_MAX || z == FLT_MIN); }

// depthTo3dSparse at the integer pixel, then cameraToWorld: (p - T) * R, double accumulation like cv::gemm on CV_32F
TOD_HD void back_project(const TrainCam& cam, int x, int y, float z, float* out3) {
  const float p[3] = {((float)x - cam.cx) * z / cam.fx, ((float)y - cam.cy) * z / cam.fy, z};
  const float q[3] = {p[0] - cam.T[0], p[1] - cam.T[1], p[2] - cam.T[2]};
  for (int c = 0; c < 3; ++c) {
    double s = 0;
    for (int k = 0; k < 3; ++k) s += (double)q[k] * (double)cam.R[3 * k + c];
    out3[c] = (float)s;
  }
}

}  // namespace tod
