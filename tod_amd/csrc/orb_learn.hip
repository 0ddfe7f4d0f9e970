// todhip_pattern_learn_* (include/todhip.h, training): learn an rBRIEF test pattern from the keypoints of training views -- the greedy
// selection of Rublee et al. 4.3 on this library's own steered patches. Three device steps:
//   add_view  the detection stages of todhip_orb_masked (orb.hip, through orb_stages.h), then per keypoint its (cos, sin) and per
//             (candidate, keypoint) one bit of the response matrix R, with describe_kernel's own arithmetic;
//   finish    ones[c] by popcount; the candidate order is sorted on the host from those M numbers; rounds 1-4 walk it in blocks of 64
//             candidates: one launch computes the block's AND-popcounts against every accepted row and inside the block, a single wave
//             then resolves the block in exact 64-bit integers. The host reads the state once per round.
// R is candidate-major, a row is row_words 64-bit pieces (piece g = keypoints 64 g .. 64 g + 63), so the device's u64 and the
// header's u32 words are the same bytes.
#include <algorithm>
#include <new>
#include <numeric>
#include <vector>

#include "ctx.h"
#include "orb_stages.h"

using namespace tod_orb;

namespace {

constexpr uint32_t kMinCandidates = 256, kMaxCandidates = 65536, kMaxKeypoints = 32768, kPattern = 256;
constexpr uint32_t kBlock = 64;                            // candidates per step of the greedy walk
constexpr uint32_t kBothCols = kPattern + kBlock;          // a block row's partners: the accepted rows, then the block's own
// selection state (device words): [0] accepted so far, [1 + r] candidate accepted r-th, [257 + r] its round
constexpr uint32_t kStateWords = 1 + 2 * kPattern;

struct LearnKp { int x, y; float ca, sa; uint32_t w, lvl; };

struct SteerArgs {
  const Cand* sel; const uint32_t* level_counts; int umax[kHalfPatch + 2];
  uint32_t sel_fs, room; LearnKp* out;                     // out: the learner's keypoint n0; room: how many still fit (<= n_features)
};

// one wave per keypoint, as describe_kernel: moments, orientation, and the keypoint's record at its place in the output order
__global__ __launch_bounds__(256) void steer_kernel(LevelTab T, SteerArgs A) {
  const uint32_t lvl = blockIdx.y;                         // one frame: virtual frame == level
  if (T.want[lvl] == 0u) return;
  const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6), l = threadIdx.x & 63u;
  if (i >= A.level_counts[lvl]) return;
  uint32_t base = 0;
  for (uint32_t j = 0; j < lvl; ++j) base += A.level_counts[j];
  const uint32_t o = base + i;
  if (o >= A.room) return;
  const Cand c = A.sel[(size_t)lvl * A.sel_fs + i];
  int m10, m01;
  patch_moments(T.img[lvl], (int)T.w[lvl], c.x, c.y, A.umax, l, m10, m01);
  float ca, sa;
  steer_of((float)m10, (float)m01, ca, sa);
  if (l == 0) { LearnKp k; k.x = c.x; k.y = c.y; k.ca = ca; k.sa = sa; k.w = T.w[lvl]; k.lvl = lvl; A.out[o] = k; }
}

// lane = keypoint, the wave walks candidates (wave-uniform coordinates): the ballot of one test is one 64-bit piece of that
// candidate's row, written by lane 0 -- no transposition, no atomics. Keypoints [n0, n1) are this view's; piece n0 / 64 may already
// hold the previous view's bits (earlier launch on the stream) and is completed, every other piece is written whole.
constexpr uint32_t kRespCands = 256;                       // candidates per workgroup, 64 per wave
__global__ __launch_bounds__(256) void response_kernel(const LearnKp* __restrict__ kp, const uint8_t* __restrict__ blur, size_t fs,
                                                       const int8_t* __restrict__ cand, uint32_t M, uint32_t n0, uint32_t n1,
                                                       unsigned long long* rows, uint32_t row_words) {
  const uint32_t l = threadIdx.x & 63u;
  const uint32_t g0 = n0 >> 6, g = g0 + blockIdx.x;
  const uint32_t n = g * 64u + l;
  const bool live = n >= n0 && n < n1;
  LearnKp k = {};
  if (live) k = kp[n];
  const uint8_t* __restrict__ img = blur + (size_t)k.lvl * fs;
  const bool merge = g == g0 && (n0 & 63u) != 0u;
  const uint32_t c0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.y * kRespCands + (threadIdx.x >> 6) * 64u));
  const uint32_t c1 = min(c0 + 64u, M);
  for (uint32_t c = c0; c < c1; ++c) {
    const bool bit = live && steered_test(img, (int)k.w, k.x, k.y, k.ca, k.sa, cand + 4u * c);
    unsigned long long piece = __builtin_amdgcn_ballot_w64(bit);
    if (l == 0) {
      unsigned long long* p = rows + (size_t)c * row_words + g;
      if (merge) piece |= *p;
      *p = piece;
    }
  }
}

// one wave per row
__global__ __launch_bounds__(256) void ones_kernel(const unsigned long long* __restrict__ rows, uint32_t row_words, uint32_t words,
                                                   uint32_t M, uint32_t* __restrict__ ones) {
  const uint32_t c = blockIdx.x * 4u + (threadIdx.x >> 6), l = threadIdx.x & 63u;
  if (c >= M) return;
  const unsigned long long* r = rows + (size_t)c * row_words;
  uint32_t s = 0;
  for (uint32_t w = l; w < words; w += 64u) s += (uint32_t)__popcll(r[w]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (l == 0) ones[c] = s;
}

struct Walk {
  const unsigned long long* rows; uint32_t row_words, words;
  const uint32_t* order; uint32_t n_pos;                   // the candidates with v > 0, in candidate order
  const uint32_t* ones; uint32_t N;
  uint32_t* state; uint8_t* taken; uint32_t* both;         // both: kBlock x kBothCols
};

// workgroup j: both[] of the block's candidate j against the rows accepted before this block (columns 0 .. accepted - 1) and against
// the block's candidates before it (columns 256 + j'); a wave per partner row, lanes over the row's pieces
__global__ __launch_bounds__(256) void both_block_kernel(Walk A, uint32_t blk) {
  const uint32_t j = blockIdx.x, pos = blk * kBlock + j;
  const uint32_t nacc = A.state[0];
  if (pos >= A.n_pos || nacc >= kPattern) return;
  const uint32_t c = A.order[pos];
  if (A.taken[c]) return;
  const unsigned long long* mine = A.rows + (size_t)c * A.row_words;
  const uint32_t l = threadIdx.x & 63u;
  for (uint32_t p = threadIdx.x >> 6; p < nacc + j; p += 4u) {
    const uint32_t other = p < nacc ? A.state[1u + p] : A.order[blk * kBlock + (p - nacc)];
    const unsigned long long* r = A.rows + (size_t)other * A.row_words;
    uint32_t s = 0;
    for (uint32_t w = l; w < A.words; w += 64u) s += (uint32_t)__popcll(mine[w] & r[w]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (l == 0) A.both[j * kBothCols + (p < nacc ? p : kPattern + (p - nacc))] = s;
  }
}

// one wave: the block's candidates in order, each against everything accepted so far (lanes over the accepted), exact integers:
// accepted iff (g^2 << shift) < v[a] v[c] for every a, g = |N both - ones[a] ones[c]| (N <= 2^15: g <= 2^28, every term < 2^63)
__global__ __launch_bounds__(64) void resolve_block_kernel(Walk A, uint32_t blk, uint32_t shift, uint32_t round) {
  __shared__ uint32_t s_ones[kPattern], s_col[kPattern];   // of accepted slot a: its popcount, its column in this block's both[]
  const uint32_t l = threadIdx.x;
  uint32_t nacc = A.state[0];
  for (uint32_t a = l; a < nacc; a += 64u) { s_ones[a] = A.ones[A.state[1u + a]]; s_col[a] = a; }
  __syncthreads();
  const unsigned long long N = A.N;
  for (uint32_t j = 0; j < kBlock; ++j) {
    const uint32_t pos = blk * kBlock + j;
    if (pos >= A.n_pos || nacc >= kPattern) break;
    const uint32_t c = A.order[pos];
    if (A.taken[c]) continue;
    const unsigned long long oc = A.ones[c], vc = oc * (N - oc);
    bool bad = vc == 0ull;
    for (uint32_t a = l; a < nacc; a += 64u) {
      const unsigned long long oa = s_ones[a], va = oa * (N - oa);
      const long long d = (long long)(N * A.both[j * kBothCols + s_col[a]]) - (long long)(oa * oc);
      const unsigned long long g = (unsigned long long)(d < 0 ? -d : d);
      bad = bad || !(((g * g) << shift) < va * vc);
    }
    if (__builtin_amdgcn_ballot_w64(bad) != 0ull) continue;
    if (l == 0) {
      A.state[1u + nacc] = c; A.state[1u + kPattern + nacc] = round; A.taken[c] = 1;
      s_ones[nacc] = (uint32_t)oc; s_col[nacc] = kPattern + j;
    }
    ++nacc;
    __syncthreads();
  }
  if (l == 0) A.state[0] = nacc;
}

// what a learner's calls need besides its own data: the selection's scratch
struct LearnWs : TodWs {
  static constexpr int kSlot = kWsLearn;
  DevBuf ones, order, state, taken, both;
};

bool in_disc(int x, int y) { return x * x + y * y <= kPatternRadius2; }

// the built-in candidate set: G = the disc's points with even coordinates, (y, x) ascending; every pair i < j at squared distance >= 16
void builtin_candidates(std::vector<int8_t>* out) {
  std::vector<int8_t> gx, gy;
  for (int y = -12; y <= 12; y += 2)
    for (int x = -12; x <= 12; x += 2)
      if (in_disc(x, y)) { gx.push_back((int8_t)x); gy.push_back((int8_t)y); }
  for (size_t i = 0; i < gx.size(); ++i)
    for (size_t j = i + 1; j < gx.size(); ++j) {
      const int dx = gx[i] - gx[j], dy = gy[i] - gy[j];
      if (dx * dx + dy * dy >= 16) { out->push_back(gx[i]); out->push_back(gy[i]); out->push_back(gx[j]); out->push_back(gy[j]); }
    }
}

}  // namespace

struct todhip_pattern_learner {
  std::vector<int8_t> cand;                                // M x 4
  uint32_t M = 0, cap = 0, N = 0, row_words = 0;
  DevBuf d_cand, rows, kp;                                 // the candidates, the response matrix, the keypoints' records
};

extern "C" {

int todhip_pattern_learn_begin(todhip_ctx* ctx, const int8_t* candidates, uint32_t n_candidates, uint32_t capacity_keypoints,
                               todhip_pattern_learner** out) {
  if (out) *out = nullptr;
  if (capacity_keypoints == 0 || capacity_keypoints > kMaxKeypoints) return TODHIP_EINVAL;
  if (candidates) {
    if (n_candidates < kMinCandidates || n_candidates > kMaxCandidates) return TODHIP_EINVAL;
    for (uint32_t c = 0; c < n_candidates; ++c)
      if (!in_disc(candidates[4 * c], candidates[4 * c + 1]) || !in_disc(candidates[4 * c + 2], candidates[4 * c + 3])) return TODHIP_EINVAL;
  }
  if (!ctx || !out) return TODHIP_EINVAL;
  TOD_HIP(hipSetDevice(ctx->device));
  todhip_pattern_learner* L = new (std::nothrow) todhip_pattern_learner();
  if (!L) return TODHIP_ENOMEM;
  if (candidates) L->cand.assign(candidates, candidates + (size_t)n_candidates * 4);
  else builtin_candidates(&L->cand);
  L->M = (uint32_t)(L->cand.size() / 4); L->cap = capacity_keypoints; L->row_words = (capacity_keypoints + 63u) / 64u;
  const size_t row_bytes = (size_t)L->M * L->row_words * 8;
  hipError_t e = L->d_cand.reserve(L->cand.size());
  if (e == hipSuccess) e = L->rows.reserve(row_bytes);
  if (e == hipSuccess) e = L->kp.reserve((size_t)L->cap * sizeof(LearnKp));
  if (e == hipSuccess) e = hipMemcpyAsync(L->d_cand.p, L->cand.data(), L->cand.size(), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemsetAsync(L->rows.p, 0, row_bytes, ctx->stream);   // padding bits are zero from here on
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) { ctx->last_hip_error = (int)e; delete L; return TODHIP_EHIP; }
  *out = L;
  return TODHIP_OK;
}

int todhip_pattern_learn_add_view_device(todhip_ctx* ctx, todhip_pattern_learner* L, const void* d_gray, const void* d_mask, uint32_t H,
                                         uint32_t W, uint32_t stride, uint32_t n_features, uint32_t n_levels, float scale_factor,
                                         uint32_t* n_added) {
  if (n_added) *n_added = 0;
  if (!ctx || !L || !d_gray || stride < W) return TODHIP_EINVAL;
  TOD_HIP(hipSetDevice(ctx->device));
  Stages S;
  const int rc = tod_orb_stages(ctx, reinterpret_cast<const uint8_t*>(d_gray), reinterpret_cast<const uint8_t*>(d_mask), H, W, stride,
                                n_features, n_levels, scale_factor, &S);
  if (rc != TODHIP_OK) return rc;
  const uint32_t add = std::min(S.n, L->cap - L->N);
  if (add == 0 || S.want_max == 0) return TODHIP_OK;
  hipStream_t st = ctx->stream;
  const uint32_t n0 = L->N, n1 = n0 + add;
  SteerArgs A;
  std::memset(&A, 0, sizeof(A));
  A.sel = S.sel; A.level_counts = S.level_counts; std::memcpy(A.umax, S.umax, sizeof(A.umax));
  A.sel_fs = S.sel_fs; A.room = add; A.out = L->kp.as<LearnKp>() + n0;
  hipLaunchKernelGGL(steer_kernel, dim3((S.want_max + 3u) / 4u, n_levels), dim3(256), 0, st, S.T, A);
  const uint32_t pieces = ((n1 + 63u) >> 6) - (n0 >> 6);
  hipLaunchKernelGGL(response_kernel, dim3(pieces, (L->M + kRespCands - 1u) / kRespCands), dim3(256), 0, st, L->kp.as<LearnKp>(),
                     S.blur, S.fs, L->d_cand.as<int8_t>(), L->M, n0, n1, L->rows.as<unsigned long long>(), L->row_words);
  TOD_HIP(hipGetLastError());
  TOD_HIP(hipStreamSynchronize(st));                       // the ORB workspace is free for the context's next call
  L->N = n1;
  if (n_added) *n_added = add;
  return TODHIP_OK;
}

int todhip_pattern_learn_add_view(todhip_ctx* ctx, todhip_pattern_learner* L, const uint8_t* gray, const uint8_t* mask, uint32_t H,
                                  uint32_t W, uint32_t stride, uint32_t n_features, uint32_t n_levels, float scale_factor,
                                  uint32_t* n_added) {
  if (n_added) *n_added = 0;
  if (!ctx || !L || !gray || stride < W || H == 0 || W == 0) return TODHIP_EINVAL;
  TOD_HIP(hipSetDevice(ctx->device));
  const uint8_t *d_gray = nullptr, *d_mask = nullptr;                    // in the ORB workspace, both at row pitch W
  if (const int rc = tod_orb_stage_host_view(ctx, gray, mask, H, W, stride, &d_gray, &d_mask)) return rc;
  return todhip_pattern_learn_add_view_device(ctx, L, d_gray, d_mask, H, W, W, n_features, n_levels, scale_factor, n_added);
}

int todhip_pattern_learn_responses(todhip_ctx* ctx, todhip_pattern_learner* L, uint32_t first, uint32_t count, uint32_t* words) {
  if (!ctx || !L || !words || first > L->M || count > L->M - first) return TODHIP_EINVAL;
  TOD_HIP(hipSetDevice(ctx->device));
  const size_t w32 = (L->N + 31u) / 32u;
  if (count == 0 || w32 == 0) return TODHIP_OK;
  TOD_HIP(hipMemcpy2DAsync(words, w32 * 4, L->rows.as<unsigned long long>() + (size_t)first * L->row_words, (size_t)L->row_words * 8,
                           w32 * 4, count, hipMemcpyDeviceToHost, ctx->stream));
  TOD_HIP(hipStreamSynchronize(ctx->stream));
  return TODHIP_OK;
}

int todhip_pattern_learn_finish(todhip_ctx* ctx, todhip_pattern_learner* L, int order, int8_t pattern[1024], uint32_t chosen[256],
                                uint8_t round_of[256], todhip_pattern_stats* stats) {
  if (order != TODHIP_PATTERN_ORDER_RANK && order != TODHIP_PATTERN_ORDER_MATCHER) return TODHIP_EINVAL;
  if (!ctx || !L || !pattern || L->N == 0) return TODHIP_EINVAL;
  TOD_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  LearnWs* ws = tod_ws<LearnWs>(ctx);
  const uint32_t M = L->M, N = L->N, words = (N + 63u) / 64u;
  TOD_HIP(ws->ones.reserve((size_t)M * 4)); TOD_HIP(ws->order.reserve((size_t)M * 4)); TOD_HIP(ws->taken.reserve(M));
  TOD_HIP(ws->state.reserve(kStateWords * 4)); TOD_HIP(ws->both.reserve((size_t)kBlock * kBothCols * 4));
  std::vector<uint32_t> ones(M), ord(M);
  hipLaunchKernelGGL(ones_kernel, dim3((M + 3u) / 4u), dim3(256), 0, st, L->rows.as<unsigned long long>(), L->row_words, words, M,
                     ws->ones.as<uint32_t>());
  TOD_HIP(hipGetLastError());
  TOD_HIP(hipMemcpyAsync(ones.data(), ws->ones.p, (size_t)M * 4, hipMemcpyDeviceToHost, st));
  TOD_HIP(hipStreamSynchronize(st));
  // candidate order: v descending, ties by ascending candidate
  std::vector<uint64_t> v(M);
  for (uint32_t c = 0; c < M; ++c) v[c] = (uint64_t)ones[c] * (N - ones[c]);
  std::iota(ord.begin(), ord.end(), 0u);
  std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return v[a] > v[b]; });
  uint32_t n_pos = 0;
  while (n_pos < M && v[ord[n_pos]] > 0) ++n_pos;
  TOD_HIP(hipMemcpyAsync(ws->order.p, ord.data(), (size_t)M * 4, hipMemcpyHostToDevice, st));
  TOD_HIP(hipMemsetAsync(ws->state.p, 0, kStateWords * 4, st));
  TOD_HIP(hipMemsetAsync(ws->taken.p, 0, M, st));
  Walk A;
  A.rows = L->rows.as<unsigned long long>(); A.row_words = L->row_words; A.words = words;
  A.order = ws->order.as<uint32_t>(); A.n_pos = n_pos; A.ones = ws->ones.as<uint32_t>(); A.N = N;
  A.state = ws->state.as<uint32_t>(); A.taken = ws->taken.as<uint8_t>(); A.both = ws->both.as<uint32_t>();
  uint32_t state[kStateWords] = {};
  static const uint32_t kShift[4] = {6, 4, 2, 0};          // |corr| < 1/8, 1/4, 1/2, 1
  for (uint32_t r = 0; r < 4 && state[0] < kPattern; ++r) {
    for (uint32_t blk = 0; blk * kBlock < n_pos; ++blk) {
      hipLaunchKernelGGL(both_block_kernel, dim3(kBlock), dim3(256), 0, st, A, blk);
      hipLaunchKernelGGL(resolve_block_kernel, dim3(1), dim3(64), 0, st, A, blk, kShift[r], r + 1u);
    }
    TOD_HIP(hipGetLastError());
    TOD_HIP(hipMemcpyAsync(state, ws->state.p, sizeof(state), hipMemcpyDeviceToHost, st));
    TOD_HIP(hipStreamSynchronize(st));
  }
  // rounds 5 and 6 need no statistics: what is left with v > 0, then the constants, each in candidate order
  uint32_t n = state[0];
  std::vector<uint8_t> taken(M, 0);
  for (uint32_t r = 0; r < n; ++r) taken[state[1 + r]] = 1;
  for (uint32_t pos = 0; pos < M && n < kPattern; ++pos)
    if (!taken[ord[pos]]) { state[1 + n] = ord[pos]; state[1 + kPattern + n] = pos < n_pos ? 5u : 6u; ++n; }
  static const uint32_t E[8] = {0, 4, 1, 5, 2, 6, 3, 7};
  todhip_pattern_stats s = {};
  s.n_keypoints = N; s.n_candidates = M;
  for (uint32_t r = 0; r < kPattern; ++r) {
    const uint32_t c = state[1 + r], round = state[1 + kPattern + r];
    const uint32_t pos = order == TODHIP_PATTERN_ORDER_MATCHER ? 32u * E[r / 32u] + r % 32u : r;
    std::memcpy(pattern + 4 * pos, &L->cand[4 * (size_t)c], 4);
    if (chosen) chosen[r] = c;
    if (round_of) round_of[r] = (uint8_t)round;
    s.accepted_in_round[round - 1u] += 1u;
  }
  if (stats) *stats = s;
  return TODHIP_OK;
}

void todhip_pattern_learn_free(todhip_ctx* ctx, todhip_pattern_learner* L) {
  if (!L) return;
  if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); }
  delete L;
}

}  // extern "C"
