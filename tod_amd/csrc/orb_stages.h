// What stage A's translation units share (orb.hip: detection and description; orb_learn.hip: the rBRIEF pattern learner): the level
// table, the selection's record, the moment and steering arithmetic of describe_kernel, and the door through which the learner runs
// the detection stages of todhip_orb_masked and reads where they left their results. Device functions here are the ONLY statement
// of that arithmetic: a bit of the learner's response matrix and a bit of a descriptor come from the same expressions.
#pragma once

#include "ctx.h"

namespace tod_orb {

constexpr int kEdge = 31;
constexpr int kHalfPatch = 15;
constexpr int kMaxLevels = 16;
constexpr int kPatternRadius2 = 13 * 13;   // every pattern point: x^2 + y^2 <= 169, so a rotated, rounded point stays inside the patch

struct Cand { int x, y, score; float harris; };

// control words of one level and one frame (device): what the selection kernels hand to each other without a
// host round trip; [8 + l] = keypoints of level l
constexpr uint32_t kCtlWords = 512;

// geometry of the pyramid levels; want[l] == 0: the level yields nothing (too small, or no features asked of it)
struct LevelTab {
  uint32_t n_levels, F;
  const uint8_t* img[kMaxLevels];                          // level l of frame 0 (frame stride: the level-0 pixel count)
  uint32_t h[kMaxLevels], w[kMaxLevels], want[kMaxLevels];
  float scale[kMaxLevels];
};

// integer moments over the radius-15 disc around (x, y): lane l < 31 owns row l - 15, every lane of the wave gets the sums
__device__ __forceinline__ void patch_moments(const uint8_t* __restrict__ img, int W, int x, int y, const int (&umax)[kHalfPatch + 2],
                                              uint32_t l, int& m10, int& m01) {
  m10 = 0; m01 = 0;
  if (l < 31u) {
    const int v = (int)l - kHalfPatch;
    const int d = v == 0 ? kHalfPatch : umax[v < 0 ? -v : v];
    int rs = 0;
    for (int u = -d; u <= d; ++u) {
      const int px = img[(size_t)(y + v) * W + x + u];
      m10 += u * px;
      rs += px;
    }
    m01 = v * rs;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { m10 += __shfl_xor(m10, off); m01 += __shfl_xor(m01, off); }
}

// the patch's orientation as (cos, sin), no angle quantisation
__device__ __forceinline__ void steer_of(float fm10, float fm01, float& ca, float& sa) {
  const float nrm = sqrtf(fm10 * fm10 + fm01 * fm01);
  ca = nrm > 0.f ? fm10 / nrm : 1.f; sa = nrm > 0.f ? fm01 / nrm : 0.f;
}

// one test (x0, y0, x1, y1) steered by (ca, sa) on the blurred level image around (x, y)
__device__ __forceinline__ bool steered_test(const uint8_t* __restrict__ blur, int W, int x, int y, float ca, float sa, const int8_t* pp) {
  const int x0 = (int)rintf((float)pp[0] * ca - (float)pp[1] * sa), y0 = (int)rintf((float)pp[0] * sa + (float)pp[1] * ca);
  const int x1 = (int)rintf((float)pp[2] * ca - (float)pp[3] * sa), y1 = (int)rintf((float)pp[2] * sa + (float)pp[3] * ca);
  const int t0 = blur[(size_t)(y + y0) * W + (x + x0)], t1 = blur[(size_t)(y + y1) * W + (x + x1)];
  return t0 < t1;
}

// Where one frame's detection stages left their results in the context's ORB workspace (valid until the context's next ORB call):
// keypoint i of level l is sel[l * sel_fs + i], i < level_counts[l], on image T.img[l] / blur + l * fs; its place in the output
// order is the earlier levels' counts + i, and n = min(their sum, n_features) of them are the call's keypoints.
struct Stages {
  LevelTab T;
  const uint8_t* blur; const Cand* sel; const uint32_t* level_counts;
  size_t fs; uint32_t sel_fs, want_max, n;
  int umax[kHalfPatch + 2];
};

}  // namespace tod_orb

// orb.hip: the stages of todhip_orb_masked (capacity n_features, built-in pattern) on a device-resident frame; d_mask (may be null)
// has row pitch W. Synchronizes the stream.
int tod_orb_stages(todhip_ctx* ctx, const uint8_t* d_gray, const uint8_t* d_mask, uint32_t H, uint32_t W, uint32_t stride,
                   uint32_t n_features, uint32_t n_levels, float scale_factor, tod_orb::Stages* out);
