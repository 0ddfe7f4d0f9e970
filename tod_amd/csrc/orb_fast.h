// FAST-9/16 on every level in one launch: the score, its border rule, the compass pre-test, and fast_nms_kernel, which scores a tile
// in LDS, suppresses non-maxima, applies the level-0 mask and appends the candidates with their score histogram.
// Included by orb.hip inside its anonymous namespace, after orb_stages.h (wave_append, the tile size) and orb_pyramid.h (load_px4).

constexpr int kFastThr = 20;

// FAST-9/16 score: max over the 16 arcs of 9 contiguous circle pixels, both polarities, of the minimum difference.
// Sliding minima over the (cyclic) circle: windows of 2, 4, 8, then 9.
__device__ __forceinline__ int arc9_max(const int (&d)[16]) {
  int m2[16], m4[16], best = -(1 << 30);
#pragma unroll
  for (int i = 0; i < 16; ++i) m2[i] = min(d[i], d[(i + 1) & 15]);
#pragma unroll
  for (int i = 0; i < 16; ++i) m4[i] = min(m2[i], m2[(i + 2) & 15]);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int m8 = min(m4[i], m4[(i + 4) & 15]);
    best = max(best, min(m8, d[(i + 8) & 15]));
  }
  return best;
}

// the border rule of the score: positions whose ring or whose non-maximum neighbourhood cannot hold a keypoint score 0 and read nothing
__device__ __forceinline__ bool fast_in_border(uint32_t h, uint32_t w, int x, int y) {
  return x < kEdge - 1 || x >= (int)w - kEdge + 1 || y < kEdge - 1 || y >= (int)h - kEdge + 1;
}

// the score of the pixel at c in an image of row pitch W (a position outside fast_in_border)
__device__ __forceinline__ int fast_score_at(const uint8_t* c, int W) {
  const int p = c[0];
  int d[16], nd[16];
  d[0] = c[3 * W] - p;       d[1] = c[3 * W + 1] - p;   d[2] = c[2 * W + 2] - p;   d[3] = c[W + 3] - p;
  d[4] = c[3] - p;           d[5] = c[-W + 3] - p;      d[6] = c[-2 * W + 2] - p;  d[7] = c[-3 * W + 1] - p;
  d[8] = c[-3 * W] - p;      d[9] = c[-3 * W - 1] - p;  d[10] = c[-2 * W - 2] - p; d[11] = c[-W - 3] - p;
  d[12] = c[-3] - p;         d[13] = c[W - 3] - p;      d[14] = c[2 * W - 2] - p;  d[15] = c[3 * W - 1] - p;
#pragma unroll
  for (int i = 0; i < 16; ++i) nd[i] = -d[i];
  const int best = max(0, max(arc9_max(d), arc9_max(nd)));
  return best > kFastThr ? best : 0;
}

// What a 9-arc above the threshold needs: any 9 contiguous ring pixels hold two cyclically adjacent ones of the compass points
// (ring positions 0, 4, 8, 12), so two adjacent compass points are both brighter than p + kFastThr or both darker than
// p - kFastThr wherever fast_score_at is not 0. Same pixels, same comparisons (d > kFastThr, -d > kFastThr) as the score's.
__device__ __forceinline__ bool fast_compass(const uint8_t* c, int W) {
  const int p = c[0];
  const int d0 = c[3 * W] - p, d4 = c[3] - p, d8 = c[-3 * W] - p, d12 = c[-3] - p;
  const bool b0 = d0 > kFastThr, b4 = d4 > kFastThr, b8 = d8 > kFastThr, b12 = d12 > kFastThr;
  const bool k0 = -d0 > kFastThr, k4 = -d4 > kFastThr, k8 = -d8 > kFastThr, k12 = -d12 > kFastThr;
  return (b0 && b4) || (b4 && b8) || (b8 && b12) || (b12 && b0) || (k0 && k4) || (k4 && k8) || (k8 && k12) || (k12 && k0);
}

// FAST score + 3x3 strict non-maximum suppression + compaction in one pass: a block scores a 64 x 16 pixel tile and
// its 1-pixel halo into LDS (the score image never goes to memory), then suppresses and appends. The candidate order
// is fixed later by the ranking kernels, so appends are aggregated per wave (wave_append).
//
// The score is found in two passes over an LDS copy of the tile's pixels (tile + 1 pixel for the suppression + 3 for the ring,
// loaded once as dwords; every ring read is an LDS read). Pass 1 visits all (64 + 2) x (16 + 2) positions, applies the border
// rule and the compass test (fast_compass: necessary for a non-zero score, five pixels instead of seventeen and no arc search)
// and appends the survivors to an LDS list (wave_append, one LDS atomic per wave). Pass 2 runs the exact score over that
// list with dense lanes. On textured images 4 % of the positions score and 6-7 % survive pass 1, but they are spread so that
// most 64-pixel row segments hold one: an early exit that needs a whole wave to fail the test would almost never be taken, so
// the survivors are compacted instead. On noise every position survives; the list holds them all.
constexpr int kNmsScoreW = kNmsTileW + 2, kNmsScoreN = (kNmsTileH + 2) * kNmsScoreW;     // scored positions: the tile and 1 pixel around
constexpr int kNmsImgDw = (kNmsTileW + 8) / 4, kNmsImgW = 4 * kNmsImgDw, kNmsImgH = kNmsTileH + 8;   // staged pixels: 4 around
__global__ __launch_bounds__(256) void fast_nms_kernel(LevelTab T, Cand* cand, uint32_t cap, uint32_t* counter, uint32_t* hist,
                                                       const uint8_t* __restrict__ mask, uint32_t H0, uint32_t W0, size_t fs) {
  const uint32_t v = blockIdx.z, lvl = v / T.F, f = v - lvl * T.F;
  const uint32_t h = T.h[lvl], w = T.w[lvl];
  if (T.want[lvl] == 0u || blockIdx.x * (uint32_t)kNmsTileW >= w || blockIdx.y * (uint32_t)kNmsTileH >= h) return;   // block-uniform
  const uint8_t* __restrict__ img = T.img[lvl] + f * fs;
  cand += (size_t)v * cap; counter += v * kCtlWords; hist += v * kCtlWords;
  if (mask) mask += f * fs;
  __shared__ int s_score[kNmsScoreN];
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_img[kNmsImgH * kNmsImgDw];          // pixel (x0 - 4 + i, y0 - 4 + r) is byte r * kNmsImgW + i
  __shared__ uint16_t s_list[kNmsScoreN];                   // pass 1's survivors (positions of s_score), in any order
  __shared__ uint32_t s_n;
  const int x0 = (int)blockIdx.x * kNmsTileW, y0 = (int)blockIdx.y * kNmsTileH;
  const uint32_t lane = threadIdx.x & 63u;
  s_hist[threadIdx.x] = 0u;
  if (threadIdx.x == 0) s_n = 0u;
  // the ring of a position outside the border rule reaches pixels [kEdge - 4, w - kEdge + 4) x [kEdge - 4, h - kEdge + 4): only pixel
  // groups that hold one of them are loaded, and such a group lies inside its row (kEdge - 4 >= 3), so inside the frame's slice
  for (int t = (int)threadIdx.x; t < kNmsImgH * kNmsImgDw; t += 256) {
    const int r = t / kNmsImgDw, x = x0 - 4 + 4 * (t - r * kNmsImgDw), y = y0 - 4 + r;
    uint32_t px = 0u;
    if (x + 3 >= kEdge - 4 && x < (int)w - kEdge + 4 && y >= kEdge - 4 && y < (int)h - kEdge + 4) px = load_px4(img + (size_t)y * w + x);
    s_img[t] = px;
  }
  __syncthreads();
  const uint8_t* s_px = reinterpret_cast<const uint8_t*>(s_img);
#pragma unroll
  for (int p0 = 0; p0 < kNmsScoreN; p0 += 256) {             // pass 1
    const int p = p0 + (int)threadIdx.x, py = p / kNmsScoreW, px = p - py * kNmsScoreW;
    const bool valid = p < kNmsScoreN;
    bool go = valid && !fast_in_border(h, w, x0 - 1 + px, y0 - 1 + py);
    if (go) go = fast_compass(s_px + (py + 3) * kNmsImgW + px + 3, kNmsImgW);
    if (valid) s_score[p] = 0;
    const uint32_t slot = wave_append(&s_n, go);
    if (go) s_list[slot] = (uint16_t)p;
  }
  __syncthreads();
  const uint32_t n_list = s_n;                               // <= kNmsScoreN: every position is appended at most once
  for (uint32_t i = threadIdx.x; i < n_list; i += 256u) {    // pass 2
    const int p = s_list[i], py = p / kNmsScoreW, px = p - py * kNmsScoreW;
    s_score[p] = fast_score_at(s_px + (py + 3) * kNmsImgW + px + 3, kNmsImgW);
  }
  __syncthreads();
  const int tx = (int)lane;
#pragma unroll
  for (int j = 0; j < kNmsTileH / 4; ++j) {
    const int ty = (int)(threadIdx.x >> 6) + 4 * j;
    const uint32_t x = (uint32_t)(x0 + tx), y = (uint32_t)(y0 + ty);
    const int* c = &s_score[(ty + 1) * kNmsScoreW + tx + 1];
    const int s = c[0];
    bool keep = s != 0 && !(x < (uint32_t)kEdge || x >= w - kEdge || y < (uint32_t)kEdge || y >= h - kEdge);
    if (keep) {
      constexpr int R = kNmsScoreW;
      keep = c[-R - 1] < s && c[-R] < s && c[-R + 1] < s && c[-1] < s && c[1] < s && c[R - 1] < s && c[R] < s && c[R + 1] < s;
    }
    if (keep && mask) {   // level-0 mask sampled at the nearest pixel (the training cell passes obs.mask to the detector, Trainer.cpp:144-150)
      uint32_t my = (uint32_t)floorf(((float)y + 0.5f) * (float)H0 / (float)h), mx = (uint32_t)floorf(((float)x + 0.5f) * (float)W0 / (float)w);
      my = min(my, H0 - 1u); mx = min(mx, W0 - 1u);
      keep = mask[(size_t)my * W0 + mx] != 0;
    }
    const uint32_t i = wave_append(counter, keep);           // the counter runs on past cap: fast_threshold_kernel clamps it
    if (keep && i < cap) {
      Cand cd; cd.x = (int)x; cd.y = (int)y; cd.score = s; cd.harris = 0.f; cand[i] = cd;
      atomicAdd(&s_hist[s & 255], 1u);
    }
  }
  __syncthreads();
  if (s_hist[threadIdx.x]) atomicAdd(&hist[threadIdx.x], s_hist[threadIdx.x]);
}
