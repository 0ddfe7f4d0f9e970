// FAST-9/16 on every level in one launch: the score, its border rule, the compass pre-test, and fast_nms_kernel, which scores a tile
// in LDS, suppresses non-maxima, applies the level-0 mask and appends the candidates with their score histogram.
// Included by orb.hip inside its anonymous namespace, after orb_stages.h (wave_append, the tile size), orb_compass.h (kFastThr,
// compass4: the pre-test on four positions), orb_arc.h (the arc search, the survivor list's entries) and orb_pyramid.h (load_px4).

// The border rule of the score: positions whose ring or whose non-maximum neighbourhood cannot hold a keypoint score 0 and read
// nothing: x < kEdge - 1, x >= w - kEdge + 1, y < kEdge - 1 or y >= h - kEdge + 1 (pass 1 of fast_nms_kernel applies it).

// the FAST-9/16 score (orb_arc.h) of the pixel at c in an image of row pitch W (a position inside the border rule's rectangle): ring
// pixels i and i + 8 lie opposite each other
__device__ __forceinline__ int fast_score_at(const uint8_t* c, int W) {
  const uint32_t pp = (uint32_t)c[0] * 0x00010001u;
  pair16 d[8];
  d[0] = pk_diff(c[3 * W], c[-3 * W], pp);          d[1] = pk_diff(c[3 * W + 1], c[-3 * W - 1], pp);
  d[2] = pk_diff(c[2 * W + 2], c[-2 * W - 2], pp);  d[3] = pk_diff(c[W + 3], c[-W - 3], pp);
  d[4] = pk_diff(c[3], c[-3], pp);                  d[5] = pk_diff(c[-W + 3], c[W - 3], pp);
  d[6] = pk_diff(c[-2 * W + 2], c[2 * W - 2], pp);  d[7] = pk_diff(c[-3 * W + 1], c[3 * W - 1], pp);
  return fast_score_pairs(d);
}

// Append to a list whose order is free, up to four entries per lane (bit i of m: the lane appends p + i): one popcount per lane, one
// prefix sum of the popcounts across the wave (wave_prefix_sum: six DPP additions, where four ballots with their lane counts took
// sixteen instructions) and one atomic on *counter. Called by all lanes of the wave together.
__device__ __forceinline__ void wave_append4(uint32_t* counter, uint16_t* list, uint32_t m, uint32_t p) {
  const uint32_t c = (uint32_t)__popc(m), v = wave_prefix_sum(c);
  const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
  if (total == 0u) return;                                   // wave-uniform
  uint32_t base = 0u;
  if ((threadIdx.x & 63u) == 0u) base = atomicAdd(counter, total);
  uint16_t* dst = list + ((uint32_t)__builtin_amdgcn_readlane((int)base, 0) + v - c);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if ((m >> i) & 1u) *dst++ = (uint16_t)(p + (uint32_t)i);
}

// FAST score + 3x3 strict non-maximum suppression + compaction in one pass: a block scores a 64 x 16 pixel tile and
// its 1-pixel halo into LDS (the score image never goes to memory), then suppresses and appends. The candidate order
// is fixed later by the ranking kernels, so appends are aggregated per wave (wave_append).
//
// The score is found in two passes over an LDS copy of the tile's pixels (tile + 1 pixel for the suppression + 3 for the ring,
// loaded once as dwords; every ring read is an LDS read). Pass 1 visits all (64 + 2) x (16 + 2) positions, four neighbours of a
// row per lane: it applies the border rule and the compass test (compass4: necessary for a non-zero score, five pixels instead of
// seventeen and no arc search; the five windows of a group are seven aligned LDS words) and appends the survivors to an LDS list
// (wave_append4, one LDS atomic per wave). Pass 2 runs the exact score over that list with dense lanes. On textured images 4 %
// of the positions score and 6-7 % survive pass 1, but they are spread so that most 64-pixel row segments hold one: an early exit that needs a whole wave to fail the test would almost never be taken, so
// the survivors are compacted instead. On noise every position survives; the list holds them all. The suppression and the append
// walk the same list: only a position on it can score, so the other 93 % of the tile are never visited again.
constexpr int kNmsScoreW = kNmsTileW + 2, kNmsScoreN = (kNmsTileH + 2) * kNmsScoreW;     // scored positions: the tile and 1 pixel around
constexpr int kNmsImgDw = (kNmsTileW + 8) / 4, kNmsImgW = 4 * kNmsImgDw, kNmsImgH = kNmsTileH + 8;   // staged pixels: 4 around
constexpr int kNmsGroups = (kNmsScoreW + 3) / 4, kNmsGroupN = (kNmsTileH + 2) * kNmsGroups;           // pass 1's groups of four positions
static_assert(kNmsScoreW % 4 == 2 && kNmsGroups + 1 == kNmsImgDw, "pass 1: a row's last group is two positions, its windows end with the staged row");
__global__ __launch_bounds__(256) void fast_nms_kernel(LevelTab T, Cand* cand, uint32_t cap, uint32_t* counter, uint32_t* hist,
                                                       const uint8_t* __restrict__ mask, uint32_t H0, uint32_t W0, size_t fs) {
  const uint32_t v = blockIdx.z, lvl = v / T.F, f = v - lvl * T.F;
  const uint32_t h = T.h[lvl], w = T.w[lvl];
  if (T.want[lvl] == 0u || blockIdx.x * (uint32_t)kNmsTileW >= w || blockIdx.y * (uint32_t)kNmsTileH >= h) return;   // block-uniform
  const uint8_t* __restrict__ img = T.img[lvl] + f * fs;
  cand += (size_t)v * cap; counter += v * kCtlWords; hist += v * kCtlWords;
  if (mask) mask += f * fs;
  __shared__ __align__(8) int s_score[kNmsScoreN];           // (pass 1 clears it two positions a store; a row starts on an even one)
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_img[kNmsImgH * kNmsImgDw];          // pixel (x0 - 4 + i, y0 - 4 + r) is byte r * kNmsImgW + i
  __shared__ uint16_t s_list[kNmsScoreN];                   // pass 1's survivors (nms_entry of their positions), in any order
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
  for (int t0 = 0; t0 < kNmsGroupN; t0 += 256) {             // pass 1: positions 4 g .. 4 g + 3 of scored row py
    if (t0 + (int)(threadIdx.x & ~63u) >= kNmsGroupN) break; // wave-uniform: no lane of this wave has a group left
    const int t = t0 + (int)threadIdx.x, py = t / kNmsGroups, g = t - py * kNmsGroups, px = 4 * g;
    uint32_t m = 0u;                                         // bit i: position px + i goes on to pass 2
    if (t < kNmsGroupN) {
      int2* z = reinterpret_cast<int2*>(&s_score[py * kNmsScoreW + px]);
      z[0] = make_int2(0, 0);
      if (g + 1 < kNmsGroups) z[1] = make_int2(0, 0);        // the last group of a row is its last two positions
      // the group's positions that the border rule lets through and that lie inside the row are lo .. hi - 1
      const int xs = x0 - 1 + px, y = y0 - 1 + py;
      const int lo = max(kEdge - 1 - xs, 0), hi = min(min((int)w - kEdge + 1 - xs, kNmsScoreW - px), 4);
      if (hi > lo && y >= kEdge - 1 && y < (int)h - kEdge + 1) m = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
      if (m) {
        // the centre pixels are bytes 4 g + 3 .. 4 g + 6 of staged row py + 3. For a row's last group c[2] is the first word of the
        // next staged row (py + 4 < kNmsImgH): it feeds the two positions past the row's end, which are not in m
        const uint32_t* c = s_img + (py + 3) * kNmsImgDw + g;
        const uint32_t *up = c - 3 * kNmsImgDw, *dn = c + 3 * kNmsImgDw;
        m &= compass4(window4(c[0], c[1], 3), window4(dn[0], dn[1], 3), window4(c[1], c[2], 2), window4(up[0], up[1], 3), c[0]);
      }
    }
    wave_append4(&s_n, s_list, m, nms_entry(px, py));
  }
  __syncthreads();
  const uint32_t n_list = s_n;                               // <= kNmsScoreN: every position is appended at most once
  for (uint32_t i = threadIdx.x; i < n_list; i += 256u) {    // pass 2
    const uint32_t e = s_list[i];
    const int py = nms_entry_py(e), px = nms_entry_px(e);
    s_score[py * kNmsScoreW + px] = fast_score_at(s_px + (py + 3) * kNmsImgW + px + 3, kNmsImgW);
  }
  __syncthreads();
  // Suppression walks the list too, with dense lanes: a position that is not on it scores 0 and is no candidate. An entry in the
  // one-pixel halo belongs to the neighbouring tile; one inside the tile has all eight neighbours in s_score.
  for (uint32_t i0 = threadIdx.x & ~63u; i0 < n_list; i0 += 256u) {   // wave-uniform: wave_append is called by the whole wave
    const uint32_t i = i0 + lane;
    uint32_t x = 0u, y = 0u;
    int s = 0;
    bool keep = false;
    if (i < n_list) {
      const uint32_t e = s_list[i];
      const int py = nms_entry_py(e), px = nms_entry_px(e);
      const int* c = &s_score[py * kNmsScoreW + px];
      s = c[0];
      x = (uint32_t)(x0 + px - 1); y = (uint32_t)(y0 + py - 1);
      keep = s != 0 && px >= 1 && px <= kNmsTileW && py >= 1 && py <= kNmsTileH &&
             !(x < (uint32_t)kEdge || x >= w - kEdge || y < (uint32_t)kEdge || y >= h - kEdge);
      if (keep) {
        constexpr int R = kNmsScoreW;
        keep = c[-R - 1] < s && c[-R] < s && c[-R + 1] < s && c[-1] < s && c[1] < s && c[R - 1] < s && c[R] < s && c[R + 1] < s;
      }
      if (keep && mask) {   // level-0 mask sampled at the nearest pixel (the training cell passes obs.mask to the detector, Trainer.cpp:144-150)
        uint32_t my = (uint32_t)floorf(((float)y + 0.5f) * (float)H0 / (float)h), mx = (uint32_t)floorf(((float)x + 0.5f) * (float)W0 / (float)w);
        my = min(my, H0 - 1u); mx = min(mx, W0 - 1u);
        keep = mask[(size_t)my * W0 + mx] != 0;
      }
    }
    const uint32_t slot = wave_append(counter, keep);        // the counter runs on past cap: fast_threshold_kernel clamps it
    if (keep && slot < cap) {
      Cand cd; cd.x = (int)x; cd.y = (int)y; cd.score = s; cd.harris = 0.f; cand[slot] = cd;
      atomicAdd(&s_hist[s & 255], 1u);
    }
  }
  __syncthreads();
  if (s_hist[threadIdx.x]) atomicAdd(&hist[threadIdx.x], s_hist[threadIdx.x]);
}
