// The end of stage A: orientation and the 256 steered tests of every selected keypoint, written in output order into the workspace,
// and the hand-over of the first `cap` of them to the caller. Included by orb.hip inside its anonymous namespace, after orb_stages.h
// (patch_moments, steer_of, steered_test: the arithmetic the pattern learner shares).

struct DescribeArgs {
  const uint8_t* blur;                          // the blurred level images (virtual-frame slices); image, pitch and scale: the level table
  const Cand* sel;                              // the levels' selections (virtual-frame slices)
  const uint32_t* level_counts;                 // per frame: word l = keypoints of level l; output base = sum of the earlier levels' counts
  uint32_t cap;
  const int8_t* pattern; int umax[kHalfPatch + 2];
  float* kp_xy; float* kp_aux; uint8_t* desc;
  size_t fs; uint32_t sel_fs;                   // frame strides: images; selection (outputs: cap rows, controls: kCtlWords)
};

// one wave per keypoint: integer moments over the radius-15 disc (lane = row), then 4 tests per lane. The arguments are only read:
// umax is indexed by the lane's row, and an argument block that is also written moves to scratch as a whole.
__global__ __launch_bounds__(256) void describe_kernel(LevelTab T, const DescribeArgs A) {
  const uint32_t v = blockIdx.y, lvl = v / T.F, f = v - lvl * T.F;
  if (T.want[lvl] == 0u) return;
  const uint8_t* __restrict__ img = T.img[lvl] + f * A.fs;
  const uint8_t* __restrict__ blur = A.blur + v * A.fs;
  const Cand* __restrict__ sel = A.sel + (size_t)v * A.sel_fs;
  const uint32_t* __restrict__ level_counts = A.level_counts + f * kCtlWords;
  float* kp_xy = A.kp_xy + (size_t)f * A.cap * 2; float* kp_aux = A.kp_aux + (size_t)f * A.cap * 4;
  uint8_t* desc = A.desc + (size_t)f * A.cap * 32;
  const float scale = T.scale[lvl];
  const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6), l = threadIdx.x & 63u;
  if (i >= level_counts[lvl]) return;
  uint32_t base = 0;
  for (uint32_t j = 0; j < lvl; ++j) base += level_counts[j];
  const uint32_t o = base + i;
  if (o >= A.cap) return;
  const Cand c = sel[i];
  const int x = c.x, y = c.y, W = (int)T.w[lvl];
  int m10, m01;
  patch_moments(img, W, x, y, A.umax, l, m10, m01);
  const float fm10 = (float)m10, fm01 = (float)m01;
  float ca, sa;
  steer_of(fm10, fm01, ca, sa);
  uint32_t nib = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) nib |= (uint32_t)steered_test(blur, W, x, y, ca, sa, A.pattern + 4 * (4 * (int)l + b)) << b;
  const uint32_t hi = __shfl_down(nib, 1);
  if ((l & 1u) == 0u) desc[(size_t)o * 32 + (l >> 1)] = (uint8_t)(nib | (hi << 4));
  if (l == 0) {
    float ang = atan2f(fm01, fm10) * 57.29577951308232f;
    if (ang < 0.f) ang += 360.f;
    kp_xy[2 * o] = (float)x * scale; kp_xy[2 * o + 1] = (float)y * scale;
    kp_aux[4 * o] = 31.f * scale; kp_aux[4 * o + 1] = ang; kp_aux[4 * o + 2] = c.harris; kp_aux[4 * o + 3] = (float)lvl;
  }
}

// the graph writes keypoints into workspace buffers; this kernel hands the first min(total, cap) of them to the caller
__global__ __launch_bounds__(256) void copy_out_kernel(const uint32_t* __restrict__ level_counts, uint32_t n_levels, uint32_t cap,
                                                       const float* __restrict__ s_xy, const float* __restrict__ s_aux,
                                                       const uint32_t* __restrict__ s_desc, float* __restrict__ d_xy,
                                                       float* __restrict__ d_aux, uint32_t* __restrict__ d_desc,
                                                       uint32_t* __restrict__ totals) {
  const uint32_t f = blockIdx.y;
  level_counts += f * kCtlWords;
  s_xy += (size_t)f * cap * 2; s_aux += (size_t)f * cap * 4; s_desc += (size_t)f * cap * 8;
  d_xy += (size_t)f * cap * 2; d_aux += (size_t)f * cap * 4; d_desc += (size_t)f * cap * 8;
  uint32_t total = 0;
  for (uint32_t l = 0; l < n_levels; ++l) total += level_counts[l];
  const uint32_t n = min(total, cap);
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;      // one dword each: 2 + 4 + 8 dwords per keypoint
  if (i == 0) totals[f] = total;
  if (i < 2u * n) d_xy[i] = s_xy[i];
  if (i < 4u * n) d_aux[i] = s_aux[i];
  if (i < 8u * n) d_desc[i] = s_desc[i];
}
