// todhip_model_compact: merge near-duplicate rows of a trained model in place (definition: include/todhip.h). The greedy
// rule is sequential in the rows and wide in the partners, as the pattern learner's selection is (orb_learn.hip): the rows go in
// blocks of kB, and per block MC1 tests the block against every row kept so far (a lane per kept row), MC2 settles the block itself
// in one wave and appends what it keeps to the front. Nothing is read on the host between the blocks: the kept count lives in the
// workspace, MC1's grid is sized by its upper bound (the block's first row) and the surplus workgroups leave at once.
#include <algorithm>
#include <cmath>

#include "model.h"

#pragma clang fp contract(off)   // d2 is rounded operation by operation, whatever flags the file is built with

namespace {

// Block rows: one wave of MC2 holds a block with a row per lane, the conflicts inside a block fit one 64-bit mask per row, and MC1's
// per-row minima are one 64-lane atomic per wave. A larger block would save launches and need a multi-wave walk for them.
constexpr uint32_t kB = 64;
constexpr uint32_t kPartners = 256;            // kept rows per MC1 workgroup
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kMaxRows = 1u << 18;

// conflict(i, j) of the header: a's row against b's, symmetric (dx only changes sign)
__device__ __forceinline__ bool rows_conflict(const uint32_t a[8], float ax, float ay, float az, const uint32_t* b, float bx, float by,
                                              float bz, uint32_t max_ham, float r2) {
  uint32_t h = 0;
#pragma unroll
  for (int w = 0; w < 8; ++w) h += (uint32_t)__popc(a[w] ^ b[w]);
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  const float d2 = (dx * dx + dy * dy) + dz * dz;
  return h <= max_ham && d2 <= r2;           // a NaN anywhere: false
}

// a descriptor row is 32 bytes at a 32-byte-aligned address: two 16-byte loads
__device__ __forceinline__ void load_desc(const uint32_t* desc, size_t row, uint32_t d[8]) {
  const uint4 a = reinterpret_cast<const uint4*>(desc)[2 * row], b = reinterpret_cast<const uint4*>(desc)[2 * row + 1];
  d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
}

// the block's rows [first, first + cnt), cnt <= kB, into LDS (44 bytes a row)
__device__ __forceinline__ void stage_block(const uint32_t* desc, const float* pts, uint32_t first, uint32_t cnt, uint32_t nthreads,
                                            uint32_t* s_d, float* s_p) {
  for (uint32_t i = threadIdx.x; i < cnt * 8u; i += nthreads) s_d[i] = desc[(size_t)first * 8 + i];
  for (uint32_t i = threadIdx.x; i < cnt * 3u; i += nthreads) s_p[i] = pts[(size_t)first * 3 + i];
}

// MC1. Workgroup g: the kept rows [g * kPartners, ...) of the compacted front, one per lane and held in registers, against the block's
// rows from LDS. min_idx[r] <- the lowest kept row that conflicts with block row r (kNone: none). Lanes of a wave hold ascending
// partners, so a wave's minimum for a row is the first set bit of the ballot; lane r keeps row r's and the wave ends in one atomicMin.
__global__ __launch_bounds__(kPartners) void conflict_block_kernel(const uint32_t* __restrict__ desc, const float* __restrict__ pts,
                                                                   uint32_t first, uint32_t cnt, const uint32_t* __restrict__ state,
                                                                   uint32_t max_ham, float r2, uint32_t* min_idx) {
  __shared__ uint32_t s_d[kB * 8];
  __shared__ float s_p[kB * 3];
  const uint32_t kept = state[0];                            // <= first: the partners never overlap the block
  if (blockIdx.x * kPartners >= kept) return;                // the grid covers `first` partners, an upper bound
  stage_block(desc, pts, first, cnt, kPartners, s_d, s_p);
  __syncthreads();
  const uint32_t p = blockIdx.x * kPartners + threadIdx.x, lane = threadIdx.x & 63u;
  if (p - lane >= kept) return;                              // a whole wave beyond the front (no barrier follows)
  const bool live = p < kept;
  uint32_t d[8] = {};
  float x = 0.f, y = 0.f, z = 0.f;
  if (live) {
    load_desc(desc, p, d);
    x = pts[(size_t)p * 3]; y = pts[(size_t)p * 3 + 1]; z = pts[(size_t)p * 3 + 2];
  }
  uint32_t mine = kNone;
  for (uint32_t r = 0; r < cnt; ++r) {
    const bool c = live && rows_conflict(d, x, y, z, s_d + 8u * r, s_p[3u * r], s_p[3u * r + 1u], s_p[3u * r + 2u], max_ham, r2);
    const unsigned long long m = __builtin_amdgcn_ballot_w64(c);
    if (lane == r && m != 0ull) mine = (p - lane) + (uint32_t)__builtin_ctzll(m);
  }
  if (mine != kNone) atomicMin(&min_idx[lane], mine);
}

// MC2. One wave, lane l = block row first + l. The conflicts inside the block (bit j of a lane's mask: it conflicts with block row
// j < l), then the rows in order: kept iff MC1 found no kept row and no row of the block kept before it conflicts.
__global__ __launch_bounds__(kB) void resolve_block_kernel(uint32_t* desc, float* pts, uint32_t first, uint32_t cnt, uint32_t* state,
                                                           uint32_t max_ham, float r2, uint32_t* min_idx, uint32_t* support) {
  __shared__ uint32_t s_d[kB * 8];
  __shared__ float s_p[kB * 3];
  __shared__ uint32_t s_sup[kB];
  const uint32_t l = threadIdx.x, kept0 = state[0];
  const bool live = l < cnt;
  uint32_t d[8] = {};
  float x = 0.f, y = 0.f, z = 0.f;
  uint32_t mn = kNone;
  if (live) {
    load_desc(desc, first + l, d);
    x = pts[(size_t)(first + l) * 3]; y = pts[(size_t)(first + l) * 3 + 1]; z = pts[(size_t)(first + l) * 3 + 2];
    mn = min_idx[l];
  }
  min_idx[l] = kNone;                                        // as the next block's MC1 expects it
#pragma unroll
  for (int w = 0; w < 8; ++w) s_d[8u * l + w] = d[w];
  s_p[3u * l] = x; s_p[3u * l + 1u] = y; s_p[3u * l + 2u] = z;
  s_sup[l] = 1u;
  __syncthreads();
  unsigned long long cm = 0ull;
  for (uint32_t j = 0; j < cnt; ++j) {
    const bool c = live && j < l && rows_conflict(d, x, y, z, s_d + 8u * j, s_p[3u * j], s_p[3u * j + 1u], s_p[3u * j + 2u], max_ham, r2);
    if (c) cm |= 1ull << j;
  }
  unsigned long long keep = 0ull;                            // uniform: every lane walks the same rows
  for (uint32_t r = 0; r < cnt; ++r) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)cm, (int)r);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(cm >> 32), (int)r);
    const uint32_t m = (uint32_t)__builtin_amdgcn_readlane((int)mn, (int)r);
    if (m == kNone && ((((unsigned long long)hi << 32) | lo) & keep) == 0ull) keep |= 1ull << r;
  }
  const bool is_kept = live && ((keep >> l) & 1ull) != 0ull;
  // a dropped row counts for its lowest conflicting kept row: MC1's where there is one (kept rows of earlier blocks all lie below
  // this block's; their support was stored by an earlier launch), else the first kept row of this block that conflicts
  if (live && !is_kept) {
    if (mn != kNone) atomicAdd(&support[mn], 1u);
    else atomicAdd(&s_sup[__builtin_ctzll(cm & keep)], 1u);
  }
  __syncthreads();
  if (is_kept) {
    // In place: the destination kept0 + (kept rows of the block before l) is <= first + l and >= kept0, so a store lands on the old
    // front's end, on a dropped row of an earlier block or inside this block, never at or above the next block's first row. Only this
    // block can be overwritten before it is read, and all of it is in registers since the barrier above.
    const size_t o = (size_t)kept0 + (uint32_t)__popcll(keep & ((1ull << l) - 1ull));
#pragma unroll
    for (int w = 0; w < 8; ++w) desc[o * 8 + w] = d[w];
    pts[o * 3] = x; pts[o * 3 + 1] = y; pts[o * 3 + 2] = z;
    support[o] = s_sup[l];
  }
  if (l == 0) state[0] = kept0 + (uint32_t)__popcll(keep);
}

struct CompactWs : TodWs {
  static constexpr int kSlot = kWsCompact;
  DevBuf state, min_idx, support;                            // 4 words ([0]: rows kept so far); kB words; a word per row
};

}  // namespace

extern "C" int todhip_model_compact(todhip_ctx* ctx, todhip_model* m, float merge_dist, uint32_t max_hamming, uint32_t* rows_before,
                                    uint32_t* rows_after, uint32_t* support, uint32_t* n_support) {
  if (!ctx || !m || !(merge_dist >= 0.f) || std::isinf(merge_dist) || max_hamming > 256u || (support && !n_support)) return TODHIP_EINVAL;
  TOD_HIP(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  uint32_t n = 0;
  TOD_HIP(hipMemcpyAsync(&n, m->small.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  TOD_HIP(hipStreamSynchronize(st));
  if (n > kMaxRows || n > m->cap) return TODHIP_EINVAL;
  if (rows_before) *rows_before = n;
  uint32_t kept = 0;
  if (n) {
    CompactWs* ws = tod_ws<CompactWs>(ctx);
    TOD_HIP(ws->state.reserve(4 * sizeof(uint32_t))); TOD_HIP(ws->min_idx.reserve(kB * sizeof(uint32_t)));
    TOD_HIP(ws->support.reserve((size_t)n * sizeof(uint32_t)));
    TOD_HIP(hipMemsetAsync(ws->state.p, 0, 4 * sizeof(uint32_t), st));
    TOD_HIP(hipMemsetAsync(ws->min_idx.p, 0xFF, kB * sizeof(uint32_t), st));
    const float r2 = merge_dist * merge_dist;
    for (uint32_t first = 0; first < n; first += kB) {
      const uint32_t cnt = std::min(kB, n - first), grid = (first + kPartners - 1u) / kPartners;
      if (grid)
        hipLaunchKernelGGL(conflict_block_kernel, dim3(grid), dim3(kPartners), 0, st, m->desc.as<uint32_t>(), m->pts.as<float>(), first,
                           cnt, ws->state.as<uint32_t>(), max_hamming, r2, ws->min_idx.as<uint32_t>());
      hipLaunchKernelGGL(resolve_block_kernel, dim3(1), dim3(kB), 0, st, m->desc.as<uint32_t>(), m->pts.as<float>(), first, cnt,
                         ws->state.as<uint32_t>(), max_hamming, r2, ws->min_idx.as<uint32_t>(), ws->support.as<uint32_t>());
    }
    TOD_HIP(hipGetLastError());
    TOD_HIP(hipMemcpyAsync(m->small.p, ws->state.p, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    TOD_HIP(hipMemcpyAsync(&kept, ws->state.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    TOD_HIP(hipStreamSynchronize(st));
  }
  if (rows_after) *rows_after = kept;
  if (support) {
    const uint32_t room = *n_support;
    *n_support = kept;
    if (room < kept) return TODHIP_ECAPACITY;
    if (kept) {
      TOD_HIP(hipMemcpyAsync(support, tod_ws<CompactWs>(ctx)->support.p, (size_t)kept * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      TOD_HIP(hipStreamSynchronize(st));
    }
  } else if (n_support) {
    *n_support = kept;
  }
  return TODHIP_OK;
}
