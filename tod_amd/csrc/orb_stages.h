// What stage A's translation units share (orb.hip: detection and description; orb_learn.hip: the rBRIEF pattern learner): the launch
// plan with the level table and the selection's record (orb_plan.h), the wave-aggregated append, the moment and steering arithmetic of
// describe_kernel, and the doors through which the learner stages a host view and runs the detection stages of todhip_orb_masked and
// reads where they left their results. Device functions here are the ONLY statement of that arithmetic: a bit of the learner's
// response matrix and a bit of a descriptor come from the same expressions.
#pragma once

#include "ctx.h"
#include "orb_moments.h"
#include "orb_plan.h"

namespace tod_orb {

// Append to a list whose order is free: one atomic per wave on *counter (LDS or global memory), every flagged lane gets its slot.
// Called by all lanes of the wave together.
__device__ __forceinline__ uint32_t wave_append(uint32_t* counter, bool flag) {
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long bal = __builtin_amdgcn_ballot_w64(flag);
  if (bal == 0ull) return 0u;
  const uint32_t first = (uint32_t)__ffsll((long long)bal) - 1u;
  uint32_t base = 0;
  if (lane == first) base = atomicAdd(counter, (uint32_t)__popcll(bal));
  base = (uint32_t)__builtin_amdgcn_readlane((int)base, (int)first);
  return base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
}

// The inclusive prefix sum of v over the wave's 64 lanes (lane 63 holds the wave's sum), on the DPP path: shifts by 1, 2, 4 and 8
// inside a row of 16 lanes, then lane 15 of every row into the next row and lane 31 into the upper half. A lane whose source lies
// outside its row, or whose row is not in the row mask, adds the 0 given as the old value. Called by all lanes of the wave together.
__device__ __forceinline__ uint32_t wave_prefix_sum(uint32_t v) {
#define TOD_ORB_DPP_ADD(ctrl, rows) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, rows, 0xF, false)
  TOD_ORB_DPP_ADD(0x111, 0xF); TOD_ORB_DPP_ADD(0x112, 0xF); TOD_ORB_DPP_ADD(0x114, 0xF); TOD_ORB_DPP_ADD(0x118, 0xF);   // row_shr:1, 2, 4, 8
  TOD_ORB_DPP_ADD(0x142, 0xA); TOD_ORB_DPP_ADD(0x143, 0xC);                                                             // row_bcast:15, row_bcast:31
#undef TOD_ORB_DPP_ADD
  return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)wave_prefix_sum(v), 63); }

// integer moments over the radius-15 disc around (x, y): lane l < 31 owns row l - 15, every lane of the wave gets the sums
__device__ __forceinline__ void patch_moments(const uint8_t* __restrict__ img, int W, int x, int y, const int (&umax)[kHalfPatch + 2],
                                              uint32_t l, int& m10, int& m01) {
  m10 = 0; m01 = 0;
  if (l < 31u) {
    const int v = (int)l - kHalfPatch;
    const int d = v == 0 ? kHalfPatch : umax[v < 0 ? -v : v];
    int rs;
    // the row from u = -15 as eight unaligned words (orb_moments.h): a keypoint is kEdge pixels inside its level, the 32 bytes in its row
    row_moments(img + (size_t)(y + v) * W + x - kHalfPatch, d, rs, m10);
    m01 = v * rs;
  }
  m10 = (int)wave_sum((uint32_t)m10); m01 = (int)wave_sum((uint32_t)m01);      // (two's complement: the sums are exact in any order)
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
  // (32-bit offsets into the frame's slice, as every pixel index of a level is)
  const int t0 = blur[(uint32_t)(y + y0) * (uint32_t)W + (uint32_t)(x + x0)], t1 = blur[(uint32_t)(y + y1) * (uint32_t)W + (uint32_t)(x + x1)];
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

// orb.hip: a host image and its mask (may be null), both with row stride `stride`, into the context's ORB workspace at row pitch W
// (of wider rows only the W pixels are read: the buffers may end with the last row's pixels); *d_mask is null without a mask. The
// copies are on the context's stream.
int tod_orb_stage_host_view(todhip_ctx* ctx, const uint8_t* gray, const uint8_t* mask, uint32_t H, uint32_t W, uint32_t stride,
                            const uint8_t** d_gray, const uint8_t** d_mask);
// orb.hip: the stages of todhip_orb_masked (capacity n_features, built-in pattern) on a device-resident frame; d_mask (may be null)
// has row pitch W. Synchronizes the stream.
int tod_orb_stages(todhip_ctx* ctx, const uint8_t* d_gray, const uint8_t* d_mask, uint32_t H, uint32_t W, uint32_t stride,
                   uint32_t n_features, uint32_t n_levels, float scale_factor, tod_orb::Stages* out);
