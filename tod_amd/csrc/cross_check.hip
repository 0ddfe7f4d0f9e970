// The cross-check filter on gfx950 (todhip_cross_check_device, todhip_set_cross_check; definition: include/todhip.h, predicate:
// cross_check.h): of a match output in the fixed-stride device layout, a match stays only where its query is the nearest valid query
// of its frame to the DB row the match names. cv::BFMatcher(normType, crossCheck = true) for every stride, per frame of a batch.
//
// The reverse search runs over the frame's QUERIES, not over DB rows: (kept matches) x (queries of the frame) distances, a few
// thousandths of the DB pass's count, so the vector ALU does it and no DB-pass kernel is involved. This file shares ctx.h, row_ops.h
// and match_keys.h (the block size) with the matcher and nothing else. The float forms' test kernel is cross_check_l2.hip's; it shares
// the frames' transport and X2 with this file through cross_check_frames.h.
//
// X1 cross_check_test_kernel     one lane = one slot of a frame's slot space (query-major, `stride` slots per query; a block is 256
//                                consecutive slots of ONE frame, blocks behind the frame's valid queries return at once). A live lane
//                                (slot < counts[q]) loads its DB row once into 8 / 16 VGPRs -- from the resident full shard, whatever
//                                selection is active: the match names a row of the full DB -- and its own query's distance to it. The
//                                frame's valid query descriptors then pass through LDS in chunks of 64; every lane of the block reads
//                                the same query at the same time, so the LDS reads are broadcasts: per pair 2 / 4 ds_read_b128, 8 / 16
//                                v_xor, 8 / 16 accumulating v_bcnt, one lexicographic test (cross_check_beats). A lane is beaten as
//                                soon as one (d', q') < (d, q) turns up; a wave leaves a chunk's loop when none of its lanes is still
//                                unbeaten (tested every 8 queries), the block leaves the frame when none of its waves is. A beaten
//                                match is marked in place (queryIdx = -1: the slot is either overwritten by X2 or ends behind the new
//                                count, where the definition leaves it unspecified), so the filter needs no workspace per slot.
// X2 cross_check_compact_kernel  one wave = one query: the unmarked matches of its first counts[q] slots move to the front in order, 64
//                                slots at a time by ballot prefix, each xyz beside its match; counts[q] = survivors, 0 for a query
//                                behind its frame's valid range. A chunk is read whole before any of it is written, and a destination
//                                is never ahead of its source, so the compaction is in place.
#include <cstdint>

#include "ctx.h"
#include "cross_check.h"
#include "cross_check_frames.h"
#include "row_ops.h"

namespace {

#include "match_keys.h"

constexpr uint32_t kChunkQueries = 64;       // query descriptors per LDS image: 2 KB at 32 bytes, 4 KB at 64 (static LDS)
constexpr uint32_t kTestEvery = 8;           // queries between two "is anybody of this wave still unbeaten" tests

struct CrossCheckWs : TodWs {
  static constexpr int kSlot = kWsCrossCheck;
  DevBuf frame_nq;
};

template <int WORDS> struct RowRegs;
template <> struct RowRegs<8> {
  uint4 a, b;
  __device__ __forceinline__ void load(const uint32_t* p) { a = reinterpret_cast<const uint4*>(p)[0]; b = reinterpret_cast<const uint4*>(p)[1]; }
  __device__ __forceinline__ uint32_t distance(const uint32_t (&qw)[8]) const { return hamming256(a, b, qw); }
};
template <> struct RowRegs<16> {
  uint4 a, b, c, d;
  __device__ __forceinline__ void load(const uint32_t* p) {
    a = reinterpret_cast<const uint4*>(p)[0]; b = reinterpret_cast<const uint4*>(p)[1];
    c = reinterpret_cast<const uint4*>(p)[2]; d = reinterpret_cast<const uint4*>(p)[3];
  }
  __device__ __forceinline__ uint32_t distance(const uint32_t (&qw)[16]) const { return hamming512(a, b, c, d, qw); }
};

// X1. blocks_per_frame blocks per frame; db_rows: row 0 of the full DB, WORDS dwords per row (16-byte aligned); q_desc: the nq query
// rows in the resident bit order (4-byte aligned, as the DB pass takes them)
template <int WORDS>
__global__ __launch_bounds__(kBlock) void cross_check_test_kernel(const uint32_t* __restrict__ q_desc, uint32_t nq, uint32_t Q, int mode,
                                                                  FrameLimits lim, const uint32_t* __restrict__ d_frame_nq,
                                                                  uint32_t blocks_per_frame, uint32_t stride,
                                                                  const uint32_t* __restrict__ counts, todhip_dmatch* matches,
                                                                  const uint32_t* __restrict__ db_rows,
                                                                  const uint32_t* __restrict__ obj_off, uint32_t n_objs) {
  __shared__ __attribute__((aligned(16))) uint32_t s_q[kChunkQueries * WORDS];
  const uint32_t f = blockIdx.x / blocks_per_frame, tid = threadIdx.x;
  const uint32_t t = (blockIdx.x - f * blocks_per_frame) * kBlock + tid;      // slot of the frame's slot space
  const tod::CrossCheckRange r = valid_range(f, nq, Q, mode, lim, d_frame_nq);
  const uint32_t ql = t / stride, j = t - ql * stride;
  if ((blockIdx.x - f * blocks_per_frame) * kBlock >= (r.hi - r.lo) * stride) return;   // (block-uniform) behind the valid queries
  const uint32_t q = r.lo + ql;
  const bool live = q < r.hi && j < min(counts[q], stride);
  const size_t slot = (size_t)q * stride + j;

  // the row the match names, and the query's own distance to it. A slot that names no row of the DB (not what any match call
  // leaves) is dropped without a read.
  RowRegs<WORDS> row = {};
  uint32_t d = 0;
  bool named = false;
  if (live) {
    const todhip_dmatch m = matches[slot];
    if ((uint32_t)m.imgIdx < n_objs && m.trainIdx >= 0) {
      const uint32_t g = obj_off[m.imgIdx] + (uint32_t)m.trainIdx;
      named = g >= obj_off[m.imgIdx] && g < obj_off[m.imgIdx + 1];
      if (named) {
        row.load(db_rows + (size_t)g * WORDS);
        uint32_t qw[WORDS];
#pragma unroll
        for (int w = 0; w < WORDS; ++w) qw[w] = q_desc[(size_t)q * WORDS + w];
        d = row.distance(qw);
      }
    }
  }
  bool beaten = false;
  for (uint32_t base = r.lo; base < r.hi; base += kChunkQueries) {
    // (the barrier also says: everybody has finished with the previous image)
    if (__syncthreads_and(!named || beaten)) break;
    const uint32_t n = min(kChunkQueries, r.hi - base);
    for (uint32_t i = tid; i < n * WORDS; i += kBlock) s_q[i] = q_desc[(size_t)base * WORDS + i];
    __syncthreads();
    if (__ballot(named && !beaten) == 0ull) continue;                           // (wave-uniform)
    for (uint32_t i = 0; i < n; ++i) {
      uint32_t qw[WORDS];
#pragma unroll
      for (int w = 0; w < WORDS; w += 4) {
        const uint4 v = *reinterpret_cast<const uint4*>(s_q + i * WORDS + w);
        qw[w] = v.x; qw[w + 1] = v.y; qw[w + 2] = v.z; qw[w + 3] = v.w;
      }
      beaten = beaten || tod::cross_check_beats(row.distance(qw), base + i, d, q);
      if ((i % kTestEvery) == kTestEvery - 1u && __ballot(named && !beaten) == 0ull) break;
    }
  }
  if (live && (beaten || !named)) matches[slot].queryIdx = -1;
}

// X2. one wave per query
__global__ __launch_bounds__(kBlock) void cross_check_compact_kernel(uint32_t nq, uint32_t Q, int mode, FrameLimits lim,
                                                                     const uint32_t* __restrict__ d_frame_nq, uint32_t stride,
                                                                     uint32_t* counts, todhip_dmatch* matches, float* xyz) {
  const uint32_t q = blockIdx.x * kWavesPerBlock + threadIdx.x / 64u, lane = threadIdx.x % 64u;
  if (q >= nq) return;
  const tod::CrossCheckRange r = valid_range(tod::cross_check_frame(q, Q), nq, Q, mode, lim, d_frame_nq);
  if (q >= r.hi) {                                                              // not a valid query of its frame
    if (lane == 0) counts[q] = 0u;
    return;
  }
  const uint32_t c = min(counts[q], stride);
  todhip_dmatch* M = matches + (size_t)q * stride;
  float* X = xyz + (size_t)q * stride * 3;
  uint32_t out = 0;
  for (uint32_t base = 0; base < c; base += 64u) {
    const uint32_t j = base + lane;
    todhip_dmatch m = {};
    float x0 = 0.f, x1 = 0.f, x2 = 0.f;
    if (j < c) { m = M[j]; x0 = X[3 * j]; x1 = X[3 * j + 1]; x2 = X[3 * j + 2]; }
    const bool keep = j < c && m.queryIdx >= 0;
    const unsigned long long mask = __ballot(keep);                             // (every lane's loads of this chunk are behind it)
    const uint32_t pos = out + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (keep && pos != j) { M[pos] = m; X[3 * pos] = x0; X[3 * pos + 1] = x1; X[3 * pos + 2] = x2; }
    out += (uint32_t)__popcll(mask);
  }
  if (lane == 0) counts[q] = out;
}

}  // namespace

int tod_cross_check_frame_limits(todhip_ctx* ctx, const uint32_t* frame_nq, uint32_t n_frames, FrameLimitArgs* out) {
  if (frame_nq && n_frames <= kArgFrames) {
    out->mode = kLimitArg;
    for (uint32_t f = 0; f < n_frames; ++f) out->lim.n[f] = frame_nq[f];
  } else if (frame_nq) {
    // pageable source: the runtime has taken the bytes when the call returns, and the copy runs behind the kernels of an earlier call
    CrossCheckWs* ws = tod_ws<CrossCheckWs>(ctx);
    TOD_HIP(ws->frame_nq.reserve((size_t)n_frames * sizeof(uint32_t)));
    TOD_HIP(hipMemcpyAsync(ws->frame_nq.p, frame_nq, (size_t)n_frames * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    out->mode = kLimitDev;
    out->d_frame_nq = ws->frame_nq.as<uint32_t>();
  }
  return TODHIP_OK;
}

void tod_cross_check_compact(todhip_ctx* ctx, uint32_t nq, uint32_t Q, const FrameLimitArgs& a, uint32_t stride, uint32_t* d_counts,
                             todhip_dmatch* d_matches, float* d_xyz) {
  hipLaunchKernelGGL(cross_check_compact_kernel, dim3((nq + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlock), 0, ctx->stream, nq, Q, a.mode,
                     a.lim, a.d_frame_nq, stride, d_counts, d_matches, d_xyz);
}

int tod_cross_check(todhip_ctx* ctx, const void* d_q, uint32_t nq, uint32_t Q, const uint32_t* frame_nq, uint32_t stride,
                    uint32_t* d_counts, todhip_dmatch* d_matches, float* d_xyz) {
  if ((uint64_t)nq * stride > 0x7FFFFFFFull) return TODHIP_EINVAL;              // slots are counted in 32 bits
  const bool wide = ctx->desc_bytes == 64;
  const uint32_t n_frames = tod::cross_check_n_frames(nq, Q);
  FrameLimitArgs a;
  if (int rc = tod_cross_check_frame_limits(ctx, frame_nq, n_frames, &a)) return rc;
  if (!wide && ctx->bit_order_on) {            // the stored rows are permuted: the queries follow them, the distances do not change
    int rc = tod_bit_order_queries(ctx, d_q, nq, &d_q);
    if (rc != TODHIP_OK) return rc;
  }
  const uint32_t* q = reinterpret_cast<const uint32_t*>(d_q);
  const uint32_t frame_rows = Q < nq ? Q : nq;
  const uint32_t bpf = (uint32_t)(((uint64_t)frame_rows * stride + kBlock - 1) / kBlock);   // (nq * stride < 2^31: checked by the caller)
  const dim3 grid(n_frames * bpf), block(kBlock);
  if (wide)
    hipLaunchKernelGGL(cross_check_test_kernel<16>, grid, block, 0, ctx->stream, q, nq, Q, a.mode, a.lim, a.d_frame_nq, bpf, stride, d_counts,
                       d_matches, ctx->db_desc.as<uint32_t>(), ctx->db_obj_off.as<uint32_t>(), ctx->n_objs);
  else
    hipLaunchKernelGGL(cross_check_test_kernel<8>, grid, block, 0, ctx->stream, q, nq, Q, a.mode, a.lim, a.d_frame_nq, bpf, stride, d_counts,
                       d_matches, ctx->db_desc.as<uint32_t>(), ctx->db_obj_off.as<uint32_t>(), ctx->n_objs);
  tod_cross_check_compact(ctx, nq, Q, a, stride, d_counts, d_matches, d_xyz);
  TOD_HIP(hipGetLastError());
  return TODHIP_OK;
}

extern "C" int todhip_cross_check_device(todhip_ctx* ctx, const void* d_q_desc, uint32_t nq, uint32_t frame_queries,
                                         const uint32_t* frame_nq, uint32_t stride, void* d_counts, void* d_matches,
                                         void* d_matches_xyz) {
  if (!ctx || !d_q_desc || !d_counts || !d_matches || !d_matches_xyz) return TODHIP_EINVAL;
  if (nq == 0 || frame_queries == 0 || stride == 0 || stride > 1024) return TODHIP_EINVAL;
  if (ctx->total_rows == 0) return TODHIP_ENODB;
  if (ctx->desc_bytes != 32 && ctx->desc_bytes != 64) return TODHIP_EINVAL;    // a float DB
  if (ctx->shard_rows != ctx->total_rows) return TODHIP_EINVAL;                // the rows the matches name are not all resident
  TOD_HIP(hipSetDevice(ctx->device));
  return tod_cross_check(ctx, d_q_desc, nq, frame_queries, frame_nq, stride, reinterpret_cast<uint32_t*>(d_counts),
                         reinterpret_cast<todhip_dmatch*>(d_matches), reinterpret_cast<float*>(d_matches_xyz));
}

extern "C" int todhip_set_cross_check(todhip_ctx* ctx, uint32_t frame_queries) {
  if (!ctx) return TODHIP_EINVAL;
  // a float DB has no Hamming rows to test against, a shard of a DB does not hold every row a match names (switching off always works)
  if (frame_queries && ctx->total_rows && (ctx->desc_bytes == 512 || ctx->desc_bytes == 256 || ctx->shard_rows != ctx->total_rows)) return TODHIP_EINVAL;
  ctx->cross_check_q = frame_queries;
  return TODHIP_OK;
}
