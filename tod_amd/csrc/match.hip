// Stage B on gfx950: exact brute-force Hamming k-NN of the frame descriptors against the
// device-resident object database, radius truncation, (imgIdx, trainIdx) resolution and the
// match -> 3D gather.  Replaces DescriptorMatcher::process (reference
// src/detection/DescriptorMatcher.cpp:195-252; the k-NN call at :211 is FLANN-LSH there,
// an exact search with the order (distance asc, global row asc) here -- decision D1).
//
// K4  hamming_topk_tiles   one lane = one query descriptor held in 8 VGPRs; the DB rows of the
//                          block's tile are wave-uniform, so they are fetched with scalar loads
//                          (s_load_dwordx8 through the scalar cache) and every xor takes its DB
//                          word straight from an SGPR: 8 v_xor + 8 accumulating v_bcnt per pair,
//                          no LDS traffic and no cross-lane work in the inner loop. Each lane keeps
//                          its k best (distance, row) keys in registers; four rows share one
//                          min3/min/compare so the top-k test costs 0.75 VALU op per pair.
//                          Partial-distance elimination: the distance over the first 128 bits is a lower
//                          bound of the full one, so when it already reaches the running limit (k-th best so
//                          far, a bound published by another tile, or radius + 1 -- rows beyond the radius
//                          never survive DescriptorMatcher.cpp:212-220) for all 4 rows x 64 queries of a
//                          group, the second half of those rows is never touched. Exact for any data; how
//                          often it fires depends on the data (always, but for ~1e-4 of the groups, on
//                          descriptors with independent bits and radius 35).
// K4x hamming_topk_mfma    the same search on the matrix cores (fp4 x fp4 MFMAs, exact): match_fp4.h, match_mfma.h; and
//     hamming_topk_fp4rows the same pass over the resident fp4 copy of the rows, the default from 4 query blocks per wave on: match_fp4rows.h.
// K4m merge_tiles_kernel   per query: merge the per-tile lists into k global keys.
// K4f finalize_kernel      per query: merge shard lists, radius cut, object lookup, 3D gather.
// This file is the matcher's one translation unit: the engine choice, the timing ring and the tod_match_* entry points. The rest
// is included below: match_keys.h (constants, sorted lists, the pick over lists), match_valu.h (K4), match_fp4.h + match_mfma.h + match_fp4rows.h
// (K4x: block primitives and list helpers, the pass over the packed rows, the pass over their fp4 copy), match_merge.h (K4m, K4s, K4f), match_plan.h (tiling, workspaces, merge launch: shared with match_wide.hip),
// match_launch.h (knobs, launchers); with ctx.h: match_tiles.h, match_split.h, KernelTimer, dispatch_k.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ctx.h"
#include "row_ops.h"

namespace {

#include "match_keys.h"
#include "match_valu.h"
#include "match_fp4.h"
#include "match_mfma.h"
#include "match_pair_pack.h"
#include "match_fp4rows.h"
#include "match_merge.h"
#include "match_plan.h"
#include "match_launch.h"

// 0: K4 on the VALU, 1: K4x on the matrix cores. todhip_set_matcher_engine() decides; while it says "auto" the
// environment variable TODHIP_K4_ENGINE=valu|mfma does (whole test suites can be run on either engine that way).
int k4_engine(const todhip_ctx* ctx, uint32_t nq) {
  if (ctx->matcher_engine == TODHIP_ENGINE_VALU) return 0;
  if (ctx->matcher_engine == TODHIP_ENGINE_MFMA) return 1;
  if (match_env().engine == 'v') return 0;
  if (match_env().engine == 'm') return 1;
  // Measured (tools/k4_engines.py, ms per launch K4 | K4x): 16 000 x 1M 3.2 | 1.1 on independent bits and 5.7 | 1.35 on this
  // repo's ORB descriptors; 1000 x 1M 0.25 | 0.085; 1000 x 100k 0.035 | 0.021; 500 x 5000 0.008 | 0.013. The matrix form
  // pays from ~2^24 pairs on; below, a wave's fixed start-up costs more than it saves. (Few queries over a big DB are
  // matrix-engine work too: both engines pad to 64 query columns, and 8 MFMAs per KB of rows keep up with HBM.)
  return (uint64_t)nq * tod_db_n_rows(ctx) >= (1ull << 24) ? 1 : 0;
}

}  // namespace

int tod_timing_drain(todhip_ctx* ctx, uint64_t keep) {
  while (ctx->ev_head - ctx->ev_tail > keep) {
    const int i = (int)(ctx->ev_tail % todhip_ctx::kEvPairs);
    TOD_HIP(hipEventSynchronize(ctx->evp[2 * i + 1]));
    float ms = 0.f;
    TOD_HIP(hipEventElapsedTime(&ms, ctx->evp[2 * i], ctx->evp[2 * i + 1]));
    ctx->counters.last_match_kernel_ms = ms;
    ctx->counters.sum_match_kernel_ms += ms;
    ctx->counters.n_match_kernel_launches += 1;
    ++ctx->ev_tail;
  }
  return TODHIP_OK;
}
int tod_timing_begin(todhip_ctx* ctx, int* slot) {
  int rc = tod_timing_drain(ctx, todhip_ctx::kEvPairs - 1);
  if (rc != TODHIP_OK) return rc;
  *slot = (int)(ctx->ev_head % todhip_ctx::kEvPairs);
  TOD_HIP(hipEventRecord(ctx->evp[2 * *slot], ctx->stream));
  return TODHIP_OK;
}
int tod_timing_end(todhip_ctx* ctx, int slot) {
  TOD_HIP(hipEventRecord(ctx->evp[2 * slot + 1], ctx->stream));
  ++ctx->ev_head;
  return TODHIP_OK;
}

// the search over the active rows (tod_db_rows): d_q is already in the resident bit order
static int match_lists_active(todhip_ctx* ctx, const void* d_q, uint32_t nq, uint32_t k, uint32_t radius, uint64_t* d_lists,
                              uint32_t* n_lists) {
  if (tod_lsh_enabled(ctx)) return tod_lsh_lists(ctx, d_q, nq, k, d_lists, n_lists);   // todhip_set_lsh: candidates from the index only
  if (ctx->ratio > 0.f) radius = 256u;   // the ratio test needs the true second neighbour, however far: no radius bound in the search
  const uint32_t* q = reinterpret_cast<const uint32_t*>(d_q);
  return dispatch_k(k, [&](auto K) { return launch_topk<decltype(K)::value>(ctx, q, nq, radius, d_lists, n_lists); });
}

// Per-query candidate lists of this shard, at either binary width: d_lists[n_lists][nq][k], each ascending, keys distance << 32 |
// global row, padding ~0. n_lists <= kMergeGroups.
int tod_match_lists(todhip_ctx* ctx, const void* d_q, uint32_t nq, uint32_t k, uint32_t radius, uint64_t* d_lists,
                    uint32_t* n_lists) {
  const bool wide = ctx->desc_bytes == 64;   // 512-bit rows: match_wide.hip. No bit order (db_bitorder.hip leaves those rows as loaded), no LSH index
  if ((!wide && ctx->desc_bytes != 32) || k == 0 || k > 8 || nq == 0) return TODHIP_EINVAL;
  if (wide && tod_lsh_enabled(ctx)) return TODHIP_EINVAL;
  if (!wide && ctx->bit_order_on) {          // todhip_set_db_bit_order: the rows are stored in another bit order, the queries follow them
    int rc = tod_bit_order_queries(ctx, d_q, nq, &d_q);
    if (rc != TODHIP_OK) return rc;
  }
  if (tod_db_n_rows(ctx) == 0) {             // no selected row in this shard: no DB pass, one list of padding keys (what an empty shard
    TOD_HIP(hipMemsetAsync(d_lists, 0xFF, (size_t)nq * k * sizeof(uint64_t), ctx->stream));   // contributes, tod_match_shard_keys)
    *n_lists = 1;
    return TODHIP_OK;
  }
  int rc = wide ? tod_wide_lists_active(ctx, d_q, nq, k, radius, d_lists, n_lists) : match_lists_active(ctx, d_q, nq, k, radius, d_lists, n_lists);
  if (rc != TODHIP_OK || !ctx->sel_on) return rc;
  return tod_view_remap(ctx, d_lists, (size_t)*n_lists * nq * k);   // todhip_db_select_objects: view rows -> rows of the full DB
}

size_t tod_match_lists_bytes(uint32_t nq, uint32_t k) { return (size_t)kMergeGroups * nq * k * sizeof(uint64_t); }

int tod_match_shard_keys(todhip_ctx* ctx, const void* d_q, uint32_t nq, uint32_t k, uint32_t radius, uint64_t* d_keys) {
  if (nq == 0) return TODHIP_OK;
  if (tod_db_n_rows(ctx) == 0) {   // an empty shard (or one without a selected row) contributes only padding keys
    TOD_HIP(hipMemsetAsync(d_keys, 0xFF, (size_t)nq * k * sizeof(uint64_t), ctx->stream));
    return TODHIP_OK;
  }
  TOD_HIP(ctx->m_keys.reserve(tod_match_lists_bytes(nq, k)));
  uint32_t n_lists = 0;
  int rc = tod_match_lists(ctx, d_q, nq, k, radius, ctx->m_keys.as<uint64_t>(), &n_lists);
  if (rc != TODHIP_OK) return rc;
  hipLaunchKernelGGL(select_keys_kernel, dim3((nq + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream,
                     ctx->m_keys.as<uint64_t>(), n_lists, nq, k, d_keys);
  TOD_HIP(hipGetLastError());
  return TODHIP_OK;
}

int tod_match_finalize(todhip_ctx* ctx, const uint64_t* d_keys_all, uint32_t n_shards, uint32_t nq, uint32_t k_in, uint32_t k_out,
                       uint32_t radius, uint32_t* d_counts, todhip_dmatch* d_matches, float* d_xyz, hipStream_t stream) {
  if (nq == 0) return TODHIP_OK;
  const uint32_t blocks = (nq + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(finalize_kernel, dim3(blocks), dim3(kBlock), 0, stream ? stream : ctx->stream, d_keys_all, n_shards, nq, k_in, k_out,
                     radius, ctx->ratio, ctx->db_obj_off.as<uint32_t>(), ctx->n_objs, ctx->db_pts.as<float>(), d_counts, d_matches,
                     d_xyz);
  TOD_HIP(hipGetLastError());
  return TODHIP_OK;
}

#ifdef TOD_K4X_COUNT_WALKS
// diagnostics build only: {32 x 32 blocks tested, blocks whose best dot product beat a threshold (16 rows walked)} since the last reset
extern "C" int todhip_debug_k4x_walks(unsigned long long out[2], int reset) {
  unsigned long long zero[2] = {0ull, 0ull};
  if (hipDeviceSynchronize() != hipSuccess) return TODHIP_EHIP;
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_k4x_blocks), sizeof(zero)) != hipSuccess) return TODHIP_EHIP;
  if (reset && hipMemcpyToSymbol(HIP_SYMBOL(g_k4x_blocks), zero, sizeof(zero)) != hipSuccess) return TODHIP_EHIP;
  return TODHIP_OK;
}
#endif
