// The selection between FAST and the descriptors, per (level, frame), through the control words of orb_plan.h: the score threshold
// from the histogram, the split into sure candidates and ties, the ranking kernel in its two uses (RankArgs), and the Harris response.
// Included by orb.hip inside its anonymous namespace, after orb_stages.h (Cand, LevelTab, W_*, wave_append).

__device__ __forceinline__ unsigned long long key_of(const Cand& c, bool by_harris) {
  uint32_t hi;
  if (by_harris) {
    const uint32_t b = __float_as_uint(c.harris);
    const uint32_t asc = (b & 0x80000000u) ? ~b : (b | 0x80000000u);   // order-preserving map of float to uint
    hi = ~asc;                                                          // descending
  } else {
    hi = 0xFFFFFFFFu - (uint32_t)c.score;
  }
  return ((unsigned long long)hi << 32) | ((unsigned long long)(uint32_t)c.y << 16) | (uint32_t)c.x;
}

// "keep the 2n best by FAST score" only defines a SET (the Harris ranking re-orders it), so a 256-bin histogram
// gives the score threshold T: everything above T is kept, and of the candidates at exactly T the first
// keep - count(> T) in (y, x) order.
__global__ __launch_bounds__(64) void fast_threshold_kernel(LevelTab T, uint32_t* ctl, uint32_t cand_cap) {
  const uint32_t want = T.want[blockIdx.x / T.F], keep = 2u * want;
  if (want == 0u) return;
  ctl += blockIdx.x * kCtlWords;
  const uint32_t l = threadIdx.x;                          // one wave per frame: lane l owns score bins 4 l .. 4 l + 3
  const uint32_t n = min(ctl[W_NCAND], cand_cap);
  uint32_t b[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) b[i] = ctl[W_HIST + 4u * l + i];
  const uint32_t mine = b[0] + b[1] + b[2] + b[3];
  uint32_t suf = mine;                                     // candidates in this lane's bins and all higher ones
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_down(suf, d); if (l + d < 64u) suf += t; }
  uint32_t above = suf - mine, thr = 0, need = 0;
  bool hit = false;
  if (n > keep) {
#pragma unroll
    for (int i = 3; i >= 0; --i) {                         // the highest score at which the count reaches `keep`
      if (!hit && above + b[i] >= keep) { hit = true; thr = 4u * l + (uint32_t)i; need = keep - above; }
      above += b[i];
    }
  }
  const unsigned long long bal = __builtin_amdgcn_ballot_w64(hit);
  const uint32_t winner = bal ? 63u - (uint32_t)__clzll((long long)bal) : 0u;
  if (l == winner) {
    ctl[W_NCAND] = n;
    ctl[W_THR] = thr; ctl[W_NEED_EQ] = (n > keep) ? need : 0u;
    ctl[W_NSEL1] = min(n, keep);
    ctl[W_NGT] = 0u; ctl[W_NEQ] = 0u;
    ctl[W_WANT] = want;                                    // what the Harris ranking keeps (RankArgs::rank_harris)
  }
}

__global__ __launch_bounds__(256) void split_kernel(LevelTab T, const Cand* __restrict__ cand, uint32_t* ctl, Cand* sel1,
                                                    Cand* eq, uint32_t cand_cap, uint32_t sel1_cap) {
  const uint32_t keep = 2u * T.want[blockIdx.y / T.F];
  if (keep == 0u) return;
  cand += (size_t)blockIdx.y * cand_cap; eq += (size_t)blockIdx.y * cand_cap; sel1 += (size_t)blockIdx.y * sel1_cap;
  ctl += blockIdx.y * kCtlWords;
  const uint32_t n = ctl[W_NCAND];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (blockIdx.x * 256u >= n) return;                       // block-uniform
  Cand c = {};
  bool gt = false, eqv = false;
  if (i < n) {
    c = cand[i];
    gt = n <= keep || (uint32_t)c.score > ctl[W_THR];
    eqv = !gt && (uint32_t)c.score == ctl[W_THR];
  }
  // one atomic per wave and list (the order inside both lists is free)
  const uint32_t i_gt = wave_append(&ctl[W_NGT], gt), i_eq = wave_append(&ctl[W_NEQ], eqv);
  if (gt) sel1[i_gt] = c;
  if (eqv) eq[i_eq] = c;
}

// keep the `keep` best of in[0..n) at out[off + rank]: rank by counting against LDS-staged key tiles (keys are unique: they contain
// the position). Every pointer is that of virtual frame 0; the kernel moves on by blockIdx.y. Passed by value and only read.
struct RankArgs {
  const Cand* in; Cand* out; uint32_t in_fs, out_fs;       // records and their strides per virtual frame
  const uint32_t* n_ptr; const uint32_t* keep_ptr;         // control words: how many there are, how many to keep
  const uint32_t* off_ptr;                                 // control word: where in `out` rank 0 goes; null: at 0
  uint32_t* n_out; uint32_t n_out_F;                       // null, or min(n, keep) to row (frame) of n_out, word (level), of n_out_F frames
  int by_harris;                                           // the key: Harris response, or FAST score; ties by (y, x)

  // The ties at the FAST threshold: the first W_NEED_EQ of eq's W_NEQ records in (y, x) order go behind the W_NGT sure ones in sel1.
  // Reads W_NEQ, W_NEED_EQ, W_NGT; writes no control word.
  static RankArgs rank_ties(const Cand* eq, uint32_t cand_cap, Cand* sel1, uint32_t sel1_cap, const uint32_t* ctl) {
    return {eq, sel1, cand_cap, sel1_cap, ctl + W_NEQ, ctl + W_NEED_EQ, ctl + W_NGT, nullptr, 0u, 0};
  }
  // The Harris ranking: the W_WANT best of sel1's W_NSEL1 records go to sel2 in rank order. Reads W_NSEL1, W_WANT; writes the count
  // to the frame's level_counts row (of F frames), word = level.
  static RankArgs rank_harris(const Cand* sel1, uint32_t sel1_cap, Cand* sel2, uint32_t sel2_cap, const uint32_t* ctl,
                              uint32_t* level_counts, uint32_t F) {
    return {sel1, sel2, sel1_cap, sel2_cap, ctl + W_NSEL1, ctl + W_WANT, nullptr, level_counts, F, 1};
  }
};

constexpr uint32_t kRankTile = 2048;
__global__ __launch_bounds__(256) void rank_tiled_kernel(const RankArgs A) {
  __shared__ unsigned long long keys[kRankTile];
  const Cand* __restrict__ in = A.in + (size_t)blockIdx.y * A.in_fs;         // frame: buffers by their strides,
  Cand* out = A.out + (size_t)blockIdx.y * A.out_fs;
  const uint32_t n = A.n_ptr[blockIdx.y * kCtlWords];                        // control words by kCtlWords
  const uint32_t keep = A.keep_ptr[blockIdx.y * kCtlWords];
  const uint32_t off = A.off_ptr ? A.off_ptr[blockIdx.y * kCtlWords] : 0u;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  // blockIdx.y = level * n_out_F + frame
  if (A.n_out && i == 0) A.n_out[(blockIdx.y % A.n_out_F) * kCtlWords + blockIdx.y / A.n_out_F] = min(n, keep);
  if (blockIdx.x * 256u >= n) return;                       // block-uniform
  Cand me;
  unsigned long long mine = ~0ull;
  if (i < n) { me = in[i]; mine = key_of(me, A.by_harris != 0); }
  uint32_t rank = 0;
  for (uint32_t t0 = 0; t0 < n; t0 += kRankTile) {
    const uint32_t tn = min(kRankTile, n - t0);
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < tn; j += 256u) keys[j] = key_of(in[t0 + j], A.by_harris != 0);
    __syncthreads();
    for (uint32_t j = 0; j < tn; ++j) rank += keys[j] < mine;
  }
  if (i < n && rank < keep) out[off + rank] = me;
}

__global__ __launch_bounds__(256) void harris_kernel(LevelTab T, Cand* cand, const uint32_t* __restrict__ n_ptr, size_t fs,
                                                     uint32_t cand_fs) {
  const uint32_t lvl = blockIdx.y / T.F, f = blockIdx.y - lvl * T.F, w = T.w[lvl];
  if (T.want[lvl] == 0u) return;
  const uint8_t* __restrict__ img = T.img[lvl] + f * fs;
  cand += (size_t)blockIdx.y * cand_fs; n_ptr += blockIdx.y * kCtlWords;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= *n_ptr) return;
  const int x = cand[i].x, y = cand[i].y, W = (int)w;
  int a = 0, b = 0, c = 0;
  for (int dy = -3; dy <= 3; ++dy)
    for (int dx = -3; dx <= 3; ++dx) {
      const uint8_t* p = img + (size_t)(y + dy) * w + (x + dx);
      const int ix = ((int)p[1] - (int)p[-1]) * 2 + ((int)p[-W + 1] - (int)p[-W - 1]) + ((int)p[W + 1] - (int)p[W - 1]);
      const int iy = ((int)p[W] - (int)p[-W]) * 2 + ((int)p[W - 1] - (int)p[-W - 1]) + ((int)p[W + 1] - (int)p[-W + 1]);
      a += ix * ix; b += iy * iy; c += ix * iy;
    }
  const float scale = 1.f / (4.f * 7 * 255.f);
  const float s4 = (scale * scale) * (scale * scale);
  const float fa = (float)a, fb = (float)b, fc = (float)c;
  cand[i].harris = (fa * fb - fc * fc - 0.04f * ((fa + fb) * (fa + fb))) * s4;
}
