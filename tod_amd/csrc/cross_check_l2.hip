// The cross-check filter over a float DB on gfx950 (todhip_cross_check_l2_device, todhip_set_l2_cross_check; definition:
// include/todhip.h, predicates: cross_check.h and l2_filters.h): todhip_cross_check_device's definition word for word, with
// d(q, g) = the binary32 bits of the defining d2 (l2_d2.h) in place of the Hamming distance. The test kernel is this file's, the
// frames, the marking and the compaction X2 are cross_check.hip's (cross_check_frames.h).
//
// A translation unit of its own because it is compiled with -fno-slp-vectorize (Makefile): with the SLP vectorizer on, hipcc pairs
// the sums of two queries in flight into v_pk_* instructions and keeps every component of the lane's DB row twice, as a (x, x)
// register pair -- 256 registers for the row alone, and the kernel spills. The flag changes the register numbering of
// cross_check.hip's Hamming kernels, which stay as they are, so it is not set there.
#include <algorithm>
#include <cstdint>

#include "ctx.h"
#include "cross_check.h"
#include "cross_check_frames.h"
#include "l2_d2.h"
#include "l2_filters.h"
#include "row_ops.h"

namespace {

#include "match_keys.h"

// X1L, the test over float rows (todhip_cross_check_l2_device): d(q, g) = the bits of the defining d2 (l2_d2.h), which costs 128 x
// (subtract, multiply, add) on one dependent accumulator instead of X1's 8 xor + 8 bcnt, so the work is cut the other way as well:
// work item = (a block of 256 consecutive slots of ONE frame) x (chunk c of that frame's valid queries, chunk_q rows each, the host
// picks the chunk count so that one frame's launch fills the device). A live lane holds its DB row in 128 VGPRs and its own d; the
// chunk's queries pass through LDS in tiles of kL2TileQueries, every lane reads the same address (a broadcast ds_read_b128), and
// kL2Flight queries are in flight per lane on independent accumulators so that one add chain's latency hides behind the others.
// Exact early exit, every kL2ExitDims dimensions: a sequential binary32 sum of squares never decreases, so once every unbeaten lane
// of the wave has partial > d (strictly) for all queries in flight, none of them can beat anyone of the wave and their remaining
// dimensions are skipped -- the partial sums then fail cross_check_beats exactly as the full ones would (a lane's own query never
// has partial > d). A beaten match is marked as X1 marks it (queryIdx = -1). The chunks of a slot only ever store that one value and
// read imgIdx / trainIdx, counts and descriptors: no workspace, no atomic, no order between chunks.
constexpr uint32_t kL2TileQueries = 32;      // query rows per LDS image: 16 KB
constexpr uint32_t kL2Flight = 4;            // queries in flight per lane
constexpr uint32_t kL2ExitDims = 32;         // dimensions between two early-exit tests
constexpr uint32_t kL2MinChunk = 16;         // fewest query rows worth a work item of their own (beside the 128-float row load)
constexpr uint32_t kL2Vec = tod::kL2Dim / 4u;   // float4 per row

// no load moves above this point, neither in the optimizer (the empty asm) nor in the instruction scheduler (the barrier)
#define L2_LOADS_STAY_BEHIND() do { asm volatile("" ::: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)

__global__ __launch_bounds__(kBlock, 2) void cross_check_l2_test_kernel(const float* __restrict__ q_desc, uint32_t nq, uint32_t Q, int mode,
                                                                     FrameLimits lim, const uint32_t* __restrict__ d_frame_nq,
                                                                     uint32_t blocks_per_frame, uint32_t n_chunks, uint32_t chunk_q,
                                                                     uint32_t stride, const uint32_t* __restrict__ counts,
                                                                     todhip_dmatch* matches, const float* __restrict__ db_rows,
                                                                     const uint32_t* __restrict__ obj_off, uint32_t n_objs) {
  __shared__ __attribute__((aligned(16))) float s_q[kL2TileQueries * tod::kL2Dim];
  const uint32_t item = blockIdx.x / n_chunks, chunk = blockIdx.x - item * n_chunks;
  const uint32_t f = item / blocks_per_frame, blk = item - f * blocks_per_frame, tid = threadIdx.x;
  const tod::CrossCheckRange r = valid_range(f, nq, Q, mode, lim, d_frame_nq);
  if (blk * kBlock >= (r.hi - r.lo) * stride) return;                           // (block-uniform) behind the valid queries
  const uint32_t c_lo = r.lo + chunk * chunk_q;                                  // (chunk < n_chunks <= Q / chunk_q + 1: no overflow)
  if (c_lo >= r.hi) return;                                                     // (block-uniform) the chunk is behind them too
  const uint32_t c_hi = min(r.hi, c_lo + chunk_q);
  const uint32_t t = blk * kBlock + tid;                                        // slot of the frame's slot space
  const uint32_t ql = t / stride, j = t - ql * stride;
  const uint32_t q = r.lo + ql;
  const bool live = q < r.hi && j < min(counts[q], stride);
  const size_t slot = (size_t)q * stride + j;

  // the row the match names and the query's own distance to it, as X1. A lane without a named row loads row 0 beside query r.lo
  // instead (both exist) and is never looked at: the loads stand outside every branch, so that the 128 registers of the row are
  // written once and never merged with anything.
  bool named = false;
  uint32_t g = 0;
  if (live) {
    const int img = matches[slot].imgIdx, train = matches[slot].trainIdx;
    if ((uint32_t)img < n_objs && train >= 0) {
      const uint32_t at = obj_off[img] + (uint32_t)train;
      named = at >= obj_off[img] && at < obj_off[img + 1];
      if (named) g = at;
    }
  }
  float4 row[kL2Vec];
  float d_f = 0.f;
  {
    const float4* rp = reinterpret_cast<const float4*>(db_rows + (size_t)g * tod::kL2Dim);
    const float4* qp = reinterpret_cast<const float4*>(q_desc + (size_t)(named ? q : r.lo) * tod::kL2Dim);
    // the own distance in a rolled loop BEFORE the row settles in its registers: unrolled beside the row's loads, its 32 loads of the
    // query are all hoisted (256 registers in flight and the row spilled); the row comes from the cache the second time
#pragma unroll 2
    for (uint32_t v = 0; v < kL2Vec; ++v) d_f = d2_step4(d_f, qp[v], rp[v]);
#pragma unroll
    for (uint32_t v = 0; v < kL2Vec; ++v) row[v] = rp[v];
  }
  const uint32_t d = tod::l2_d2_bits(d_f);
  bool beaten = false;
  for (uint32_t base = c_lo; base < c_hi; base += kL2TileQueries) {
    // (the barrier also says: everybody has finished with the previous image)
    if (__syncthreads_and(!named || beaten)) break;
    const uint32_t n = min(kL2TileQueries, c_hi - base);
    {
      const float4* src = reinterpret_cast<const float4*>(q_desc + (size_t)base * tod::kL2Dim);
      float4* dst = reinterpret_cast<float4*>(s_q);
      for (uint32_t i = tid; i < n * kL2Vec; i += kBlock) dst[i] = src[i];
    }
    __syncthreads();
    if (__ballot(named && !beaten) == 0ull) continue;                           // (wave-uniform)
    for (uint32_t i = 0; i < n; i += kL2Flight) {
      // a short last group repeats the tile's last query: the same pair tested again
      uint32_t qi[kL2Flight];
      float acc[kL2Flight];
#pragma unroll
      for (uint32_t u = 0; u < kL2Flight; ++u) { qi[u] = min(i + u, n - 1u); acc[u] = 0.f; }
      // the queries' next four dimensions are read while the present four are summed; the scheduling barrier keeps the compiler
      // from hoisting more reads than that (all 128 of a group otherwise: 512 registers, which it then spills)
      float4 cur[kL2Flight], nxt[kL2Flight];
#pragma unroll
      for (uint32_t u = 0; u < kL2Flight; ++u) cur[u] = *reinterpret_cast<const float4*>(s_q + qi[u] * tod::kL2Dim);
#pragma unroll
      for (uint32_t v0 = 0; v0 < kL2Vec; v0 += kL2ExitDims / 4u) {
#pragma unroll
        for (uint32_t v = v0; v < v0 + kL2ExitDims / 4u; ++v) {
          if (v + 1u < kL2Vec) {
#pragma unroll
            for (uint32_t u = 0; u < kL2Flight; ++u) nxt[u] = *reinterpret_cast<const float4*>(s_q + qi[u] * tod::kL2Dim + 4u * (v + 1u));
          }
#pragma unroll
          for (uint32_t u = 0; u < kL2Flight; ++u) acc[u] = d2_step4(acc[u], cur[u], row[v]);
          L2_LOADS_STAY_BEHIND();
#pragma unroll
          for (uint32_t u = 0; u < kL2Flight; ++u) cur[u] = nxt[u];
        }
        if (v0 + kL2ExitDims / 4u < kL2Vec) {
          bool open = false;                                                    // can one of the queries in flight still beat this lane?
#pragma unroll
          for (uint32_t u = 0; u < kL2Flight; ++u) open = open || !(acc[u] > d_f);
          if (__ballot(named && !beaten && open) == 0ull) break;                // (wave-uniform)
        }
      }
#pragma unroll
      for (uint32_t u = 0; u < kL2Flight; ++u)
        beaten = beaten || tod::cross_check_beats(tod::l2_d2_bits(acc[u]), base + qi[u], d, q);
      if (__ballot(named && !beaten) == 0ull) break;
    }
  }
  if (live && (beaten || !named)) matches[slot].queryIdx = -1;
}

// X1L over rows of kL2DimNarrow = 64 floats (desc_bytes 256). A sibling, not a template: built from one body shared with the kernel
// above, that kernel comes out scheduled differently (2352 instructions for 2359), and it is to stay instruction for instruction what
// it was. The same work items, tiles, flight and exit test; the lane's row is 64 VGPRs and the LDS image 8 KB. (Its name does not
// contain the other's: tests/test_l2_filters_cpu.py finds that one by name.)
constexpr uint32_t kL2NarrowVec = tod::kL2DimNarrow / 4u;   // float4 per row

__global__ __launch_bounds__(kBlock, 2) void cross_check_l2_narrow_kernel(const float* __restrict__ q_desc, uint32_t nq, uint32_t Q, int mode,
                                                                     FrameLimits lim, const uint32_t* __restrict__ d_frame_nq,
                                                                     uint32_t blocks_per_frame, uint32_t n_chunks, uint32_t chunk_q,
                                                                     uint32_t stride, const uint32_t* __restrict__ counts,
                                                                     todhip_dmatch* matches, const float* __restrict__ db_rows,
                                                                     const uint32_t* __restrict__ obj_off, uint32_t n_objs) {
  __shared__ __attribute__((aligned(16))) float s_q[kL2TileQueries * tod::kL2DimNarrow];
  const uint32_t item = blockIdx.x / n_chunks, chunk = blockIdx.x - item * n_chunks;
  const uint32_t f = item / blocks_per_frame, blk = item - f * blocks_per_frame, tid = threadIdx.x;
  const tod::CrossCheckRange r = valid_range(f, nq, Q, mode, lim, d_frame_nq);
  if (blk * kBlock >= (r.hi - r.lo) * stride) return;                           // (block-uniform) behind the valid queries
  const uint32_t c_lo = r.lo + chunk * chunk_q;                                  // (chunk < n_chunks <= Q / chunk_q + 1: no overflow)
  if (c_lo >= r.hi) return;                                                     // (block-uniform) the chunk is behind them too
  const uint32_t c_hi = min(r.hi, c_lo + chunk_q);
  const uint32_t t = blk * kBlock + tid;                                        // slot of the frame's slot space
  const uint32_t ql = t / stride, j = t - ql * stride;
  const uint32_t q = r.lo + ql;
  const bool live = q < r.hi && j < min(counts[q], stride);
  const size_t slot = (size_t)q * stride + j;

  // the row the match names and the query's own distance to it, as X1. A lane without a named row loads row 0 beside query r.lo
  // instead (both exist) and is never looked at: the loads stand outside every branch, so that the 64 registers of the row are
  // written once and never merged with anything.
  bool named = false;
  uint32_t g = 0;
  if (live) {
    const int img = matches[slot].imgIdx, train = matches[slot].trainIdx;
    if ((uint32_t)img < n_objs && train >= 0) {
      const uint32_t at = obj_off[img] + (uint32_t)train;
      named = at >= obj_off[img] && at < obj_off[img + 1];
      if (named) g = at;
    }
  }
  float4 row[kL2NarrowVec];
  float d_f = 0.f;
  {
    const float4* rp = reinterpret_cast<const float4*>(db_rows + (size_t)g * tod::kL2DimNarrow);
    const float4* qp = reinterpret_cast<const float4*>(q_desc + (size_t)(named ? q : r.lo) * tod::kL2DimNarrow);
    // the own distance in a rolled loop BEFORE the row settles in its registers, as above; the row comes from the cache the second time
#pragma unroll 2
    for (uint32_t v = 0; v < kL2NarrowVec; ++v) d_f = d2_step4(d_f, qp[v], rp[v]);
#pragma unroll
    for (uint32_t v = 0; v < kL2NarrowVec; ++v) row[v] = rp[v];
  }
  const uint32_t d = tod::l2_d2_bits(d_f);
  bool beaten = false;
  for (uint32_t base = c_lo; base < c_hi; base += kL2TileQueries) {
    // (the barrier also says: everybody has finished with the previous image)
    if (__syncthreads_and(!named || beaten)) break;
    const uint32_t n = min(kL2TileQueries, c_hi - base);
    {
      const float4* src = reinterpret_cast<const float4*>(q_desc + (size_t)base * tod::kL2DimNarrow);
      float4* dst = reinterpret_cast<float4*>(s_q);
      for (uint32_t i = tid; i < n * kL2NarrowVec; i += kBlock) dst[i] = src[i];
    }
    __syncthreads();
    if (__ballot(named && !beaten) == 0ull) continue;                           // (wave-uniform)
    for (uint32_t i = 0; i < n; i += kL2Flight) {
      // a short last group repeats the tile's last query: the same pair tested again
      uint32_t qi[kL2Flight];
      float acc[kL2Flight];
#pragma unroll
      for (uint32_t u = 0; u < kL2Flight; ++u) { qi[u] = min(i + u, n - 1u); acc[u] = 0.f; }
      // the queries' next four dimensions are read while the present four are summed; the scheduling barrier keeps the compiler
      // from hoisting more reads than that (all 64 of a group otherwise)
      float4 cur[kL2Flight], nxt[kL2Flight];
#pragma unroll
      for (uint32_t u = 0; u < kL2Flight; ++u) cur[u] = *reinterpret_cast<const float4*>(s_q + qi[u] * tod::kL2DimNarrow);
#pragma unroll
      for (uint32_t v0 = 0; v0 < kL2NarrowVec; v0 += kL2ExitDims / 4u) {
#pragma unroll
        for (uint32_t v = v0; v < v0 + kL2ExitDims / 4u; ++v) {
          if (v + 1u < kL2NarrowVec) {
#pragma unroll
            for (uint32_t u = 0; u < kL2Flight; ++u) nxt[u] = *reinterpret_cast<const float4*>(s_q + qi[u] * tod::kL2DimNarrow + 4u * (v + 1u));
          }
#pragma unroll
          for (uint32_t u = 0; u < kL2Flight; ++u) acc[u] = d2_step4(acc[u], cur[u], row[v]);
          L2_LOADS_STAY_BEHIND();
#pragma unroll
          for (uint32_t u = 0; u < kL2Flight; ++u) cur[u] = nxt[u];
        }
        if (v0 + kL2ExitDims / 4u < kL2NarrowVec) {
          bool open = false;                                                    // can one of the queries in flight still beat this lane?
#pragma unroll
          for (uint32_t u = 0; u < kL2Flight; ++u) open = open || !(acc[u] > d_f);
          if (__ballot(named && !beaten && open) == 0ull) break;                // (wave-uniform)
        }
      }
#pragma unroll
      for (uint32_t u = 0; u < kL2Flight; ++u)
        beaten = beaten || tod::cross_check_beats(tod::l2_d2_bits(acc[u]), base + qi[u], d, q);
      if (__ballot(named && !beaten) == 0ull) break;
    }
  }
  if (live && (beaten || !named)) matches[slot].queryIdx = -1;
}

// the two float DBs: rows of kL2Dim or of kL2DimNarrow floats
bool narrow_float_db(const todhip_ctx* ctx) { return ctx->desc_bytes == tod::kL2DimNarrow * 4u; }
bool float_db(const todhip_ctx* ctx) { return ctx->desc_bytes == tod::kL2Dim * 4u || narrow_float_db(ctx); }

}  // namespace

int tod_cross_check_l2(todhip_ctx* ctx, const void* d_q, uint32_t nq, uint32_t Q, const uint32_t* frame_nq, uint32_t stride,
                       uint32_t* d_counts, todhip_dmatch* d_matches, float* d_xyz) {
  if ((uint64_t)nq * stride > 0x7FFFFFFFull) return TODHIP_EINVAL;              // slots are counted in 32 bits
  const uint32_t n_frames = tod::cross_check_n_frames(nq, Q);
  FrameLimitArgs a;
  if (int rc = tod_cross_check_frame_limits(ctx, frame_nq, n_frames, &a)) return rc;
  const uint32_t frame_rows = Q < nq ? Q : nq;
  const uint32_t bpf = (uint32_t)(((uint64_t)frame_rows * stride + kBlock - 1) / kBlock);
  // chunks of a frame's queries: as many as bring the launch to two blocks (8 waves: the kernel's two per SIMD) on every CU, as
  // far as chunks of kL2MinChunk rows go; a call of many frames gets there without cutting
  const uint32_t items = n_frames * bpf, want = 2u * (uint32_t)ctx->n_cu;
  const uint32_t max_chunks = (frame_rows + kL2MinChunk - 1u) / kL2MinChunk;
  const uint32_t n_chunks = std::max(1u, std::min(max_chunks, (want + items - 1u) / items));
  const uint32_t chunk_q = (frame_rows + n_chunks - 1u) / n_chunks;
  const dim3 block(kBlock);
  hipLaunchKernelGGL(narrow_float_db(ctx) ? cross_check_l2_narrow_kernel : cross_check_l2_test_kernel, dim3(items * n_chunks), block, 0,
                     ctx->stream, reinterpret_cast<const float*>(d_q), nq, Q,
                     a.mode, a.lim, a.d_frame_nq, bpf, n_chunks, chunk_q, stride, d_counts, d_matches, ctx->db_desc.as<float>(),
                     ctx->db_obj_off.as<uint32_t>(), ctx->n_objs);
  tod_cross_check_compact(ctx, nq, Q, a, stride, d_counts, d_matches, d_xyz);
  TOD_HIP(hipGetLastError());
  return TODHIP_OK;
}

extern "C" int todhip_cross_check_l2_device(todhip_ctx* ctx, const void* d_q_desc, uint32_t nq, uint32_t frame_queries,
                                            const uint32_t* frame_nq, uint32_t stride, void* d_counts, void* d_matches,
                                            void* d_matches_xyz) {
  if (!ctx || !d_q_desc || !d_counts || !d_matches || !d_matches_xyz) return TODHIP_EINVAL;
  if (nq == 0 || frame_queries == 0 || stride == 0 || stride > 1024) return TODHIP_EINVAL;
  if (ctx->total_rows == 0) return TODHIP_ENODB;
  if (!float_db(ctx)) return TODHIP_EINVAL;                                    // a binary DB: todhip_cross_check_device
  if (ctx->shard_rows != ctx->total_rows) return TODHIP_EINVAL;                // the rows the matches name are not all resident
  TOD_HIP(hipSetDevice(ctx->device));
  return tod_cross_check_l2(ctx, d_q_desc, nq, frame_queries, frame_nq, stride, reinterpret_cast<uint32_t*>(d_counts),
                            reinterpret_cast<todhip_dmatch*>(d_matches), reinterpret_cast<float*>(d_matches_xyz));
}

extern "C" int todhip_set_l2_cross_check(todhip_ctx* ctx, uint32_t frame_queries) {
  if (!ctx) return TODHIP_EINVAL;
  // a binary DB has no float rows to test against, a shard of a DB does not hold every row a match names (switching off always works)
  if (frame_queries && ctx->total_rows && (!float_db(ctx) || ctx->shard_rows != ctx->total_rows)) return TODHIP_EINVAL;
  ctx->l2_cross_check_q = frame_queries;
  return TODHIP_OK;
}
