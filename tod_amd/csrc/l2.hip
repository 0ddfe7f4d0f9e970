// Float-descriptor matcher on gfx950 (BASELINE.json configs[3]: "SIFT-128 float descriptors, L2 brute force as an
// MFMA bf16 GEMM"). Not a reference feature: DescriptorMatcher serves binary descriptors through FLANN-LSH only and
// throws for other index types (src/detection/DescriptorMatcher.cpp:154-188). What is kept from the reference is the
// result shape of DescriptorMatcher::process (:195-252): k nearest rows per query over the concatenated DB, truncated
// at the first distance > radius (:212-220), (imgIdx, trainIdx) by object prefix sums, the 3D point of each match.
//
// Exact result from an approximate GEMM -- filter and refine:
//   score(q, r) = |r|^2 - 2 <q^, r^>          q^, r^ = bf16 roundings, product on the matrix cores (f32 accumulate)
//   |score + |q|^2 - d2(q, r)| <= eps(q)      eps(q) = 2^-6 (1 + 2^-6) |q| Rmax + 2^-14 (|q| + Rmax)^2, Rmax = max |r|
//   (l2_bound.h states eps and derives it: bf16 keeps 8 significant bits, so rounding moves every COMPONENT by up to u = 2^-8 of
//   its magnitude; -2 <q^, r^> is then off by at most (4 u + 2 u^2) |q||r| = 2^-6 (1 + 2^-9) |q||r| by Cauchy-Schwarz on each of the
//   three error terms, and inputs exist that reach it. The second term covers every f32 rounding: the f32 norms, the matrix cores'
//   accumulation of the 128 products onto |r|^2, and the sequential f32 sum that DEFINES d2, see include/todhip.h.
//   tests/l2_bound_host_test.cpp holds the inequality against binary64; domain: finite components, normal f32 squared norms.)
//   pass 0  seed(q) >= A_k from a sample of the DB                  (the k-th smallest of per-partition minima, or of per-lane lists)
//   pass 1  A_k(q) = k-th smallest score over the DB                (GEMM + per-lane top-8 in registers; only scores
//                                                                    below the seed are ever inserted)
//   pass 2  candidates = { r : score <= A_k + 2 eps }                (same GEMM; a lane's candidates go to its private slot)
//           every row of the true top-k is a candidate: the k rows of the smallest scores have d2 <= A_k + |q|^2 + eps, so the k-th
//           smallest d2, T_k, is at most that, and a row with d2 <= T_k scores at most d2 - |q|^2 + eps <= A_k + 2 eps
//   DBs of >= 64k rows skip pass 1: the sample is an evenly spaced quarter of the DB (at most 64k rows) and seed + 2 eps
//   is used as the threshold of pass 2 -- seed >= A_k, so the candidates are a superset (rows of rank <= ~k N / n_sample
//   plus the eps band) and pass 3 returns the same result from it
//   pass 3  exact d2 of the candidates in the defining order (sequential f32, no fma), k smallest by (d2, row);
//           a query whose candidate lists overflowed is redone by an exact scan of the whole DB
//
// One translation unit, headers by concern; this file is the host side (workspace, launches, the C entry points):
//   l2_plan.h     host, no HIP: shared constants, L2Knobs (the environment), L2Plan = geometry, seed-pass decision, buffer sizes
//   l2_bound.h    host and device, plain C++: the bf16 rounding and eps(q), with the derivation
//   l2_prepare.h  l2_prepare_kernel: bf16 images of the DB (A-fragment order) and of the queries, norms, eps
//   l2_gemm.h     L2G  l2_gemm_kernel<PASS, KT>: wave = (DB chunk, 4 query tiles of 32), the DB streams through a per-wave ring in LDS,
//                 the accumulator IS the score; CandSink and the epilogues of passes 0, 1, 2
//   l2_refine.h   l2_threshold_kernel, pass 3 (l2_rerank_kernel, l2_exact_scan_kernel), l2_finalize_kernel, shared device helpers
//   l2_radius.h   the radius search's kernels (todhip_match_l2_radius*): LT, LR, LS, LE around the same DB pass
//   l2_sharded.h  the sharded forms' kernels (todhip_match_l2[_radius]_shard_device, todhip_merge_l2[_radius]_shards_device[_on]): SK, SR, LK, LM
//   l2_trace.h    host: the wave-trace report of TODHIP_L2_TRACE
//   l2_d2.h       the defining distance d2_exact (shared with cross_check_l2.hip); l2_filters.h: the ratio test's predicate
//                 (todhip_set_l2_ratio_test), evaluated by l2_finalize_kernel and l2_merge_knn_kernel<K>
// Two row widths: desc_bytes 512 = 128 x f32 and desc_bytes 256 = 64 x f32 (SURF, KAZE). The kernels that touch a row take the
// width as a template argument (l2_prepare_kernel has a sibling); l2_kernels(ctx) below is the one place that picks between them.
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "ctx.h"
#include "row_ops.h"
#include "l2_plan.h"
#include "l2_prepare.h"
#include "l2_gemm.h"
#include "l2_refine.h"
#include "l2_radius.h"
#include "l2_sharded.h"
#include "l2_trace.h"

namespace {

// Every buffer is its own allocation: no call site computes an offset into one. "per query" = L2Plan::nq_pad entries.
struct L2Ws : TodWs {
  static constexpr int kSlot = kWsL2;
  DevBuf db_bf16, db_norm, scal;              // the DB: bf16 image in A-fragment order, |row|^2; scal[0] = bits of Rmax^2
  DevBuf q_bf16, q_eps, q_norm;               // per query: bf16 image scaled by -2, eps, |q|^2
  DevBuf thr, seed, scan_marks;               // per query: pass 2's threshold; pass 0's seed (k-NN); 1 = the scan answers it whatever the DB pass finds (radius)
  DevBuf slots, slot_cnt, cand, cand_cnt;     // CandSink (l2_gemm.h); cand_cnt is zeroed by the query preparation
  DevBuf flags;                               // per query: 1 = its candidate lists overflowed (or scan_marks said so), the exact scan answers it
  DevBuf part, keys;                          // passes 0 and 1: [partition][query][kTop] scores (pass 2: the wave trace); the result keys
  DevBuf shard_counts, shard_in_radius;       // per query: what LR / LS count for the radius search's sharded form (SR reads them)
};

const L2Knobs& l2_knobs() {                                 // the environment, read once
  auto number = [](const char* name) { return getenv(name) ? (uint32_t)atoi(getenv(name)) : 0u; };
  auto is_set = [](const char* name) { return getenv(name) != nullptr; };
  static const L2Knobs knobs{number("TODHIP_L2_CHUNK_ROUNDS"), number("TODHIP_L2_SAMPLE_TILES"), number("TODHIP_L2_SEED_CHUNKS"),
                            is_set("TODHIP_L2_NO_CANDIDATES"), is_set("TODHIP_L2_TRACE"), is_set("TODHIP_L2_EXACT_SCAN")};
  return knobs;
}

// The one dispatcher on the row width: every kernel that touches a row of D floats, for D = kDim or kDimNarrow. The signatures do not
// depend on D, so a launch site reads the resident DB's table (l2_kernels(ctx)) and is otherwise what it was; the kernels that see
// keys, scores or counters only (threshold, finalize, emit, the shard and merge kernels) are not in it.
using L2Gemm = decltype(&l2_gemm_kernel<2, 4, kDim>);
struct L2Kernels {
  uint32_t dim;
  decltype(&l2_prepare_kernel) prepare;
  L2Gemm pass1_kt1, pass1_kt4, pass1_kt8, pass2;
  decltype(&l2_rerank_kernel<kDim>) rerank;
  decltype(&l2_exact_scan_kernel<kDim>) exact_scan;
  decltype(&l2_radius_threshold_kernel<kDim>) radius_threshold;
  decltype(&l2_radius_refine_kernel<kDim>) radius_refine;
  decltype(&l2_radius_scan_kernel<kDim>) radius_scan;
  L2Gemm pass1(uint32_t kt) const { return kt == 1u ? pass1_kt1 : kt == 4u ? pass1_kt4 : pass1_kt8; }
};
template <uint32_t D>
constexpr L2Kernels l2_kernels_of(decltype(&l2_prepare_kernel) prepare) {
  return {D, prepare, l2_gemm_kernel<1, 1, D>, l2_gemm_kernel<1, 4, D>, l2_gemm_kernel<1, 8, D>, l2_gemm_kernel<2, 4, D>, l2_rerank_kernel<D>,
          l2_exact_scan_kernel<D>, l2_radius_threshold_kernel<D>, l2_radius_refine_kernel<D>, l2_radius_scan_kernel<D>};
}
// (a context that holds no float DB never gets here: l2_db_check stands before every call)
const L2Kernels& l2_kernels(const todhip_ctx* ctx) {
  static const L2Kernels wide = l2_kernels_of<kDim>(l2_prepare_kernel), narrow = l2_kernels_of<kDimNarrow>(l2_prepare_narrow_kernel);
  return l2_dim_of(ctx->desc_bytes) == kDimNarrow ? narrow : wide;
}

// What every call that runs the DB pass (l2_gemm_kernel<2, 4>) over nq queries starts with: the buffers the pass reads and writes,
// and the queries' bf16 image pre-scaled by -2 (a power of two: no extra rounding), |q|^2, eps and zeroed shared counters.
int l2_pass_begin(todhip_ctx* ctx, L2Ws* ws, const L2Plan& P, const float* d_q, uint32_t nq) {
  const std::pair<DevBuf*, size_t> bufs[] = {{&ws->cand_cnt, P.cand_cnt_bytes}, {&ws->flags, P.flags_bytes}, {&ws->q_bf16, P.q_bf16_bytes},
                                             {&ws->q_eps, P.q_eps_bytes}, {&ws->q_norm, P.q_norm_bytes}, {&ws->thr, P.thr_bytes},
                                             {&ws->cand, P.cand_bytes}, {&ws->slots, P.slots_bytes}, {&ws->slot_cnt, P.slot_cnt_bytes}};
  for (const auto& b : bufs) TOD_HIP(b.first->reserve(b.second));
  hipLaunchKernelGGL(l2_kernels(ctx).prepare, dim3((P.nq_pad + 3u) / 4u), dim3(256), 0, ctx->stream, d_q, nq, P.nq_pad, -2.0f,
                     ws->q_bf16.as<uint16_t>(), ws->q_norm.as<float>(), (uint32_t*)nullptr, 0, (const uint32_t*)ws->scal.as<uint32_t>(),
                     ws->q_eps.as<float>(), ws->cand_cnt.as<uint32_t>());
  return TODHIP_OK;
}

// One launch of l2_gemm_kernel over the plan's query blocks. tiles: what differs between the launches -- the seed pass runs over
// a sample (n tiles, every stride-th of the DB's, in grid_x chunks of per_chunk), the other passes over the plan's chunks of the
// whole DB. part: where passes 0 and 1 leave their lists (pass 2: the wave trace, or null); thr: the seed that limits pass 1
// (or null), pass 2's candidate threshold; sink: pass 2's candidate containers.
struct L2Tiles { uint32_t n, per_chunk, stride, grid_x; };
L2Tiles l2_all_tiles(const L2Plan& P) { return {P.n_tiles, P.tiles_per_chunk, 1u, P.n_chunks}; }

void l2_launch_gemm(L2Gemm kernel, todhip_ctx* ctx, const L2Ws* ws, const L2Plan& P, L2Tiles tiles, float* part, const float* thr,
                    bool sink) {
  hipLaunchKernelGGL(kernel, dim3(tiles.grid_x, P.q_blocks), dim3(256), 0, ctx->stream, ws->db_bf16.as<uint16_t>(),
                     ws->db_norm.as<float>(), tiles.n, tiles.per_chunk, tiles.stride, ws->q_bf16.as<uint16_t>(), P.nq_pad, part, thr,
                     sink ? ws->slots.as<uint32_t>() : nullptr, sink ? ws->slot_cnt.as<uint32_t>() : nullptr,
                     sink ? ws->cand.as<uint32_t>() : nullptr, sink ? ws->cand_cnt.as<uint32_t>() : nullptr);
}

// the k-NN search up to its keys (ws->keys: [nq][k], l2_rerank_kernel's layout). The timing bracket, one per call, is around
// l2_gemm_kernel<2, 4> on the one-GEMM path and around pass 1's GEMM on the classic path
int l2_keys(todhip_ctx* ctx, const float* d_q, uint32_t nq, uint32_t k) {
  L2Ws* ws = tod_ws<L2Ws>(ctx);
  hipStream_t st = ctx->stream;
  const uint32_t n = (uint32_t)ctx->shard_rows;
  const L2Knobs& knobs = l2_knobs();
  const L2Kernels& K = l2_kernels(ctx);
  const L2Plan P = l2_plan(n, nq, k, (uint32_t)ctx->n_cu, knobs, K.dim);
  TOD_HIP(ws->keys.reserve(P.keys_bytes));
  if (knobs.exact_scan) {
    hipLaunchKernelGGL(K.exact_scan, dim3(nq), dim3(256), 0, st, d_q, nq, ctx->db_desc.as<float>(), n, k,
                       (const uint32_t*)nullptr, ws->keys.as<uint64_t>());
    TOD_HIP(hipGetLastError());
    return TODHIP_OK;
  }
  if (int rc = l2_pass_begin(ctx, ws, P, d_q, nq)) return rc;
  TOD_HIP(ws->part.reserve(P.part_bytes));
  TOD_HIP(ws->seed.reserve(P.seed_bytes));
  // out = (k_eff-th smallest of n_parts partitions' lists, capped by seed_in) + margin * eps, for the first n_real queries
  auto threshold = [&](uint32_t n_parts, uint32_t n_real, const float* seed_in, float margin, float* out) {
    hipLaunchKernelGGL(l2_threshold_kernel, dim3((P.nq_pad + 3u) / 4u), dim3(256), 0, st, ws->part.as<float>(), n_parts, n_real, P.nq_pad,
                       P.k_eff, seed_in, ws->q_eps.as<float>(), margin, out);
  };
  const float* seed = nullptr;
  if (P.seed_pass) {
    l2_launch_gemm(K.pass1(P.kt0), ctx, ws, P, {P.sample_tiles, P.s_tpc, P.sample_stride, P.s_used}, ws->part.as<float>(), nullptr, false);
    if (P.fast) threshold(2u * P.s_used, nq, nullptr, P.margin, ws->thr.as<float>());
    else { threshold(2u * P.s_used, P.nq_pad, nullptr, 0.f, ws->seed.as<float>()); seed = ws->seed.as<float>(); }
  }
  KernelTimer timer{ctx};
  if (int rc = timer.begin()) return rc;
  if (!P.one_gemm()) {
    l2_launch_gemm(K.pass1(P.kt1), ctx, ws, P, l2_all_tiles(P), ws->part.as<float>(), seed, false);
    if (int rc = timer.end()) return rc;
    threshold(P.n_parts, nq, seed, P.margin, ws->thr.as<float>());
  }
  l2_launch_gemm(K.pass2, ctx, ws, P, l2_all_tiles(P), knobs.trace ? ws->part.as<float>() : nullptr, ws->thr.as<float>(), true);
  if (P.one_gemm()) { if (int rc = timer.end()) return rc; }
  if (knobs.trace) { if (int rc = l2_trace_report(ctx, ws->part.p, P.q_blocks, P.n_chunks)) return rc; }
  hipLaunchKernelGGL(K.rerank, dim3((nq + 3u) / 4u), dim3(256), 0, st, d_q, nq, ctx->db_desc.as<float>(),
                     ws->slots.as<uint32_t>(), ws->slot_cnt.as<uint32_t>(), P.n_parts, ws->cand.as<uint32_t>(),
                     ws->cand_cnt.as<uint32_t>(), k, ws->keys.as<uint64_t>(), ws->flags.as<uint32_t>());
  hipLaunchKernelGGL(K.exact_scan, dim3(nq), dim3(256), 0, st, d_q, nq, ctx->db_desc.as<float>(), n, k,
                     (const uint32_t*)ws->flags.as<uint32_t>(), ws->keys.as<uint64_t>());
  TOD_HIP(hipGetLastError());
  return TODHIP_OK;
}

// The radius search up to its keys: LT, the DB pass, LR, LS (l2_radius.h) over the resident rows (there is at least one). ws->keys:
// [nq][mpq], the first d_counts[q] of a row valid, rows numbered within the shard. d_counts / d_in_radius: device memory (d_in_radius
// may be null).
int l2_radius_keys(todhip_ctx* ctx, const float* d_q, uint32_t nq, float radius, uint32_t mpq, uint32_t* d_counts, uint32_t* d_in_radius) {
  TOD_HIP(hipSetDevice(ctx->device));
  L2Ws* ws = tod_ws<L2Ws>(ctx);
  hipStream_t st = ctx->stream;
  const float* db = ctx->db_desc.as<float>();
  const L2Kernels& K = l2_kernels(ctx);
  const L2Plan P = l2_plan((uint32_t)ctx->shard_rows, nq, mpq, (uint32_t)ctx->n_cu, l2_knobs(), K.dim);
  TOD_HIP(ws->keys.reserve(P.keys_bytes));
  if (int rc = l2_pass_begin(ctx, ws, P, d_q, nq)) return rc;
  TOD_HIP(ws->scan_marks.reserve(P.scan_marks_bytes));
  hipLaunchKernelGGL(K.radius_threshold, dim3((P.nq_pad + 255u) / 256u), dim3(256), 0, st, d_q, nq, P.nq_pad, radius,
                     ws->q_eps.as<float>(), ws->thr.as<float>(), ws->scan_marks.as<uint32_t>());
  KernelTimer timer{ctx};
  if (int rc = timer.begin()) return rc;
  l2_launch_gemm(K.pass2, ctx, ws, P, l2_all_tiles(P), nullptr, ws->thr.as<float>(), true);
  if (int rc = timer.end()) return rc;
  hipLaunchKernelGGL(K.radius_refine, dim3(nq), dim3(256), 0, st, d_q, db, ws->slots.as<uint32_t>(), ws->slot_cnt.as<uint32_t>(),
                     P.n_parts, ws->cand.as<uint32_t>(), ws->cand_cnt.as<uint32_t>(), ws->scan_marks.as<uint32_t>(), radius, mpq,
                     ws->keys.as<uint64_t>(), d_counts, d_in_radius, ws->flags.as<uint32_t>());
  hipLaunchKernelGGL(K.radius_scan, dim3(nq), dim3(256), 0, st, d_q, db, (uint32_t)ctx->shard_rows, ws->flags.as<uint32_t>(), radius,
                     mpq, ws->keys.as<uint64_t>(), d_counts, d_in_radius);
  TOD_HIP(hipGetLastError());
  return TODHIP_OK;
}

// The radius search up to its outputs: l2_radius_keys, then LE. d_matches / d_xyz: device memory, or pinned host memory for the
// matches of the host form.
int l2_radius_search(todhip_ctx* ctx, const float* d_q, uint32_t nq, float radius, uint32_t mpq, uint32_t* d_counts,
                     todhip_dmatch* d_matches, float* d_xyz, uint32_t* d_in_radius) {
  if (int rc = l2_radius_keys(ctx, d_q, nq, radius, mpq, d_counts, d_in_radius)) return rc;
  L2Ws* ws = tod_ws<L2Ws>(ctx);
  hipStream_t st = ctx->stream;
  const size_t slots = (size_t)nq * mpq;
  hipLaunchKernelGGL(l2_radius_emit_kernel, dim3((uint32_t)((slots + 255u) / 256u)), dim3(256), 0, st, ws->keys.as<uint64_t>(), d_counts, nq,
                     mpq, ctx->db_obj_off.as<uint32_t>(), ctx->n_objs, ctx->db_pts.as<float>(), d_matches, d_xyz);
  TOD_HIP(hipGetLastError());
  return TODHIP_OK;
}

// the DB every float call needs: not empty, 128 or 64 x f32; the unsharded calls: the whole of it resident
int l2_db_check(const todhip_ctx* ctx, bool sharded = false) {
  if (ctx->total_rows == 0) return TODHIP_ENODB;
  return l2_dim_of(ctx->desc_bytes) == 0u || (!sharded && ctx->shard_rows != ctx->total_rows) ? TODHIP_EINVAL : TODHIP_OK;
}

int l2_radius_args(const todhip_ctx* ctx, uint32_t nq, float radius, uint32_t mpq, bool sharded = false) {
  if (nq == 0 || mpq == 0 || mpq > kL2MaxPerQuery || !(radius > 0.f) || !std::isfinite(radius)) return TODHIP_EINVAL;
  return l2_db_check(ctx, sharded);
}

// LK or LM on `stream` (null: the context's) behind the argument checks of the two merges. They read the context's object table and
// model points only. KNN: width = k and the radius cuts; otherwise width = max_per_query and the keys carry the shards' counts.
template <bool KNN>
int l2_merge_shards(todhip_ctx* ctx, hipStream_t stream, const void* d_keys_all, uint32_t n_shards, uint32_t nq, uint32_t width, float radius,
                    void* d_counts, void* d_matches, void* d_xyz, void* d_in_radius) {
  if (!ctx || !d_keys_all || !d_counts || !d_matches || !d_xyz) return TODHIP_EINVAL;
  if (nq == 0 || width == 0 || width > (KNN ? kTop : kL2MaxPerQuery) || n_shards == 0 || n_shards > kMaxMergeShards) return TODHIP_EINVAL;
  if (KNN && !(radius > 0.f)) return TODHIP_EINVAL;
  if (KNN && ctx->l2_ratio > 0.f && width < 2) return TODHIP_EINVAL;              // the test needs the second nearest row
  if (int rc = l2_db_check(ctx, true)) return rc;
  TOD_HIP(hipSetDevice(ctx->device));
  hipStream_t st = stream ? stream : ctx->stream;
  const uint64_t* keys = reinterpret_cast<const uint64_t*>(d_keys_all);
  uint32_t* counts = reinterpret_cast<uint32_t*>(d_counts);
  todhip_dmatch* matches = reinterpret_cast<todhip_dmatch*>(d_matches);
  float* xyz = reinterpret_cast<float*>(d_xyz);
  if (KNN) {
    dispatch_k(width, [&](auto kc) {
      hipLaunchKernelGGL(l2_merge_knn_kernel<decltype(kc)::value>, dim3((nq + kMergeBlock - 1u) / kMergeBlock), dim3(kMergeBlock), 0, st, keys,
                         n_shards, nq, radius, ctx->l2_ratio, ctx->db_obj_off.as<uint32_t>(), ctx->n_objs, ctx->db_pts.as<float>(), counts, matches, xyz);
      return TODHIP_OK;
    });
  } else {
    const ShardMergeGrid g = shard_merge_grid(n_shards, nq, width);
    hipLaunchKernelGGL(g.staged ? l2_merge_radius_kernel<true> : l2_merge_radius_kernel<false>, dim3(g.blocks), dim3(kMergeBlock), 0, st, keys,
                       n_shards, nq, width, g.qpb, ctx->db_obj_off.as<uint32_t>(), ctx->n_objs, ctx->db_pts.as<float>(), counts,
                       reinterpret_cast<uint32_t*>(d_in_radius), matches, xyz);
  }
  TOD_HIP(hipGetLastError());
  return TODHIP_OK;
}

}  // namespace

// called by todhip_db_load for 128 or 64 x f32 rows (already resident in ctx->db_desc): bf16 image, norms, Rmax
int tod_l2_db_prepare(todhip_ctx* ctx) {
  L2Ws* ws = tod_ws<L2Ws>(ctx);
  const uint32_t n = (uint32_t)ctx->shard_rows, n_pad = l2_pad_rows(n);
  TOD_HIP(ws->db_bf16.reserve((size_t)std::max(n_pad, kTileRows) * l2_dim_of(ctx->desc_bytes) * 2));
  TOD_HIP(ws->db_norm.reserve((size_t)std::max(n_pad, kTileRows) * 4));
  TOD_HIP(ws->scal.reserve(64));
  TOD_HIP(hipMemsetAsync(ws->scal.p, 0, 64, ctx->stream));
  if (n_pad)
    hipLaunchKernelGGL(l2_kernels(ctx).prepare, dim3((n_pad + 3u) / 4u), dim3(256), 0, ctx->stream, ctx->db_desc.as<float>(), n,
                       n_pad, 1.0f, ws->db_bf16.as<uint16_t>(), ws->db_norm.as<float>(), ws->scal.as<uint32_t>(), 1,
                       (const uint32_t*)nullptr, (float*)nullptr, (uint32_t*)nullptr);
  TOD_HIP(hipGetLastError());
  return TODHIP_OK;
}

extern "C" {

int todhip_set_l2_ratio_test(todhip_ctx* ctx, float ratio) {
  if (!ctx || !tod::l2_ratio_valid(ratio)) return TODHIP_EINVAL;
  ctx->l2_ratio = ratio;
  return TODHIP_OK;
}

int todhip_match_l2_shard_device(todhip_ctx* ctx, const void* d_q_desc, uint32_t nq, uint32_t k, void* d_keys) {
  if (!ctx || !d_q_desc || !d_keys || nq == 0 || k == 0 || k > kTop) return TODHIP_EINVAL;
  if (ctx->l2_ratio > 0.f && k < 2) return TODHIP_EINVAL;   // the merge's ratio test needs every shard's second nearest row
  int rc = l2_db_check(ctx, true);
  if (rc != TODHIP_OK) return rc;
  TOD_HIP(hipSetDevice(ctx->device));
  const uint64_t* keys = nullptr;                           // no resident row: padding only
  if (ctx->shard_rows != 0) {
    rc = l2_keys(ctx, reinterpret_cast<const float*>(d_q_desc), nq, k);
    if (rc != TODHIP_OK) return rc;
    keys = tod_ws<L2Ws>(ctx)->keys.as<uint64_t>();
  }
  const size_t slots = (size_t)nq * k;
  hipLaunchKernelGGL(l2_shard_keys_kernel, dim3((uint32_t)((slots + 255u) / 256u)), dim3(256), 0, ctx->stream, keys, slots,
                     (uint32_t)ctx->shard_first, reinterpret_cast<uint64_t*>(d_keys));
  TOD_HIP(hipGetLastError());
  ctx->counters.last_nq = nq; ctx->counters.last_k = k;
  return TODHIP_OK;
}

int todhip_merge_l2_shards_device_on(todhip_ctx* ctx, void* hip_stream, const void* d_keys_all, uint32_t n_shards, uint32_t nq, uint32_t k,
                                     float radius, void* d_counts, void* d_matches, void* d_matches_xyz) {
  if (!ctx || !hip_stream) return TODHIP_EINVAL;
  return l2_merge_shards<true>(ctx, reinterpret_cast<hipStream_t>(hip_stream), d_keys_all, n_shards, nq, k, radius, d_counts, d_matches,
                               d_matches_xyz, nullptr);
}

int todhip_merge_l2_shards_device(todhip_ctx* ctx, const void* d_keys_all, uint32_t n_shards, uint32_t nq, uint32_t k, float radius,
                                  void* d_counts, void* d_matches, void* d_matches_xyz) {
  return l2_merge_shards<true>(ctx, nullptr, d_keys_all, n_shards, nq, k, radius, d_counts, d_matches, d_matches_xyz, nullptr);
}

int todhip_match_l2_radius_shard_device(todhip_ctx* ctx, const void* d_q_desc, uint32_t nq, float radius, uint32_t max_per_query,
                                        void* d_keys) {
  if (!ctx || !d_q_desc || !d_keys) return TODHIP_EINVAL;
  int rc = l2_radius_args(ctx, nq, radius, max_per_query, true);
  if (rc != TODHIP_OK) return rc;
  TOD_HIP(hipSetDevice(ctx->device));
  L2Ws* ws = tod_ws<L2Ws>(ctx);
  const uint32_t* d_in = nullptr;                           // no resident row: every query's count is 0
  if (ctx->shard_rows != 0) {
    TOD_HIP(ws->shard_counts.reserve((size_t)nq * sizeof(uint32_t)));
    TOD_HIP(ws->shard_in_radius.reserve((size_t)nq * sizeof(uint32_t)));
    rc = l2_radius_keys(ctx, reinterpret_cast<const float*>(d_q_desc), nq, radius, max_per_query, ws->shard_counts.as<uint32_t>(),
                        ws->shard_in_radius.as<uint32_t>());
    if (rc != TODHIP_OK) return rc;
    d_in = ws->shard_in_radius.as<uint32_t>();
  }
  const size_t slots = (size_t)nq * (max_per_query + 1u);
  hipLaunchKernelGGL(l2_radius_shard_keys_kernel, dim3((uint32_t)((slots + 255u) / 256u)), dim3(256), 0, ctx->stream, ws->keys.as<uint64_t>(),
                     ws->shard_counts.as<uint32_t>(), d_in, nq, max_per_query, (uint32_t)ctx->shard_first, reinterpret_cast<uint64_t*>(d_keys));
  TOD_HIP(hipGetLastError());
  ctx->counters.last_nq = nq; ctx->counters.last_k = max_per_query;
  return TODHIP_OK;
}

int todhip_merge_l2_radius_shards_device_on(todhip_ctx* ctx, void* hip_stream, const void* d_keys_all, uint32_t n_shards, uint32_t nq,
                                            uint32_t max_per_query, void* d_counts, void* d_matches, void* d_matches_xyz, void* d_in_radius) {
  if (!ctx || !hip_stream) return TODHIP_EINVAL;
  return l2_merge_shards<false>(ctx, reinterpret_cast<hipStream_t>(hip_stream), d_keys_all, n_shards, nq, max_per_query, 0.f, d_counts,
                                d_matches, d_matches_xyz, d_in_radius);
}

int todhip_merge_l2_radius_shards_device(todhip_ctx* ctx, const void* d_keys_all, uint32_t n_shards, uint32_t nq, uint32_t max_per_query,
                                         void* d_counts, void* d_matches, void* d_matches_xyz, void* d_in_radius) {
  return l2_merge_shards<false>(ctx, nullptr, d_keys_all, n_shards, nq, max_per_query, 0.f, d_counts, d_matches, d_matches_xyz, d_in_radius);
}

int todhip_match_l2_radius_device(todhip_ctx* ctx, const void* d_q_desc, uint32_t nq, float radius, uint32_t max_per_query, void* d_counts,
                                  void* d_matches, void* d_matches_xyz, void* d_in_radius) {
  if (!ctx || !d_q_desc || !d_counts || !d_matches || !d_matches_xyz) return TODHIP_EINVAL;
  int rc = l2_radius_args(ctx, nq, radius, max_per_query);
  if (rc != TODHIP_OK) return rc;
  rc = l2_radius_search(ctx, reinterpret_cast<const float*>(d_q_desc), nq, radius, max_per_query, reinterpret_cast<uint32_t*>(d_counts),
                        reinterpret_cast<todhip_dmatch*>(d_matches), reinterpret_cast<float*>(d_matches_xyz),
                        reinterpret_cast<uint32_t*>(d_in_radius));
  if (rc == TODHIP_OK) { ctx->counters.last_nq = nq; ctx->counters.last_k = max_per_query; }
  return rc;
}

int todhip_match_l2_radius(todhip_ctx* ctx, const float* q_desc, uint32_t nq, float radius, uint32_t max_per_query, uint32_t* row_ptr,
                           todhip_dmatch* matches, float* matches_xyz, uint32_t* n_matches, uint32_t* in_radius) {
  if (!ctx || !q_desc || !row_ptr || !matches || !matches_xyz || !n_matches) return TODHIP_EINVAL;
  int rc = l2_radius_args(ctx, nq, radius, max_per_query);
  if (rc != TODHIP_OK) return rc;
  TOD_HIP(hipSetDevice(ctx->device));
  const size_t nm = (size_t)nq * max_per_query;
  TOD_HIP(ctx->m_q.reserve((size_t)nq * ctx->desc_bytes));
  TOD_HIP(ctx->m_counts.reserve(2u * (size_t)nq * sizeof(uint32_t)));
  uint32_t* d_counts = ctx->m_counts.as<uint32_t>();
  uint32_t* d_in = d_counts + nq;
  // the emit kernel writes the kept matches straight into pinned host memory, as todhip_match_radius's does; the two count arrays
  // are read by kernels and come over with one copy
  TOD_HIP(ctx->h_stage.reserve(2u * (size_t)nq * sizeof(uint32_t) + nm * sizeof(todhip_dmatch) + nm * 3 * sizeof(float)));
  uint32_t* h_counts = ctx->h_stage.as<uint32_t>();
  uint32_t* h_in = h_counts + nq;
  todhip_dmatch* h_m = reinterpret_cast<todhip_dmatch*>(h_in + nq);
  float* h_xyz = reinterpret_cast<float*>(h_m + nm);
  TOD_HIP(hipMemcpyAsync(ctx->m_q.p, q_desc, (size_t)nq * ctx->desc_bytes, hipMemcpyHostToDevice, ctx->stream));
  rc = l2_radius_search(ctx, ctx->m_q.as<float>(), nq, radius, max_per_query, d_counts, h_m, h_xyz, d_in);
  if (rc != TODHIP_OK) return rc;
  TOD_HIP(hipMemcpyAsync(h_counts, d_counts, 2u * (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  TOD_HIP(hipStreamSynchronize(ctx->stream));
  if (in_radius) std::memcpy(in_radius, h_in, (size_t)nq * sizeof(uint32_t));
  uint64_t total = 0;
  for (uint32_t qi = 0; qi < nq; ++qi) { row_ptr[qi] = (uint32_t)total; total += h_counts[qi]; }
  row_ptr[nq] = (uint32_t)total;                            // nq * max_per_query < 2^32 matches or the reserve above has failed
  const uint32_t capacity = *n_matches;
  *n_matches = (uint32_t)total;
  ctx->counters.last_nq = nq;
  ctx->counters.last_k = max_per_query;
  if (total > capacity) return TODHIP_ECAPACITY;            // row_ptr, in_radius and the needed count are the caller's already
  ctx->counters.last_matches = tod_pack_csr(h_counts, h_m, h_xyz, nq, max_per_query, row_ptr, matches, matches_xyz);
  return TODHIP_OK;
}

int todhip_match_l2_device(todhip_ctx* ctx, const void* d_q_desc, uint32_t nq, uint32_t k, float radius, void* d_counts,
                           void* d_matches, void* d_matches_xyz) {
  if (!ctx || !d_q_desc || !d_counts || !d_matches || !d_matches_xyz) return TODHIP_EINVAL;
  if (k == 0 || k > kTop || !(radius > 0.f)) return TODHIP_EINVAL;
  int rc = l2_db_check(ctx);
  if (rc != TODHIP_OK || nq == 0) return rc;
  TOD_HIP(hipSetDevice(ctx->device));
  // the ratio test judges the two nearest rows: k == 1 searches two and returns one (todhip_match's k_in / k_out)
  const uint32_t k_in = ctx->l2_ratio > 0.f ? std::max(k, 2u) : k;
  rc = l2_keys(ctx, reinterpret_cast<const float*>(d_q_desc), nq, k_in);
  if (rc != TODHIP_OK) return rc;
  L2Ws* ws = tod_ws<L2Ws>(ctx);
  hipLaunchKernelGGL(l2_finalize_kernel, dim3((nq + 255u) / 256u), dim3(256), 0, ctx->stream, ws->keys.as<uint64_t>(), nq, k_in, k, radius,
                     ctx->l2_ratio, ctx->db_obj_off.as<uint32_t>(), ctx->n_objs, ctx->db_pts.as<float>(),
                     reinterpret_cast<uint32_t*>(d_counts), reinterpret_cast<todhip_dmatch*>(d_matches),
                     reinterpret_cast<float*>(d_matches_xyz));
  TOD_HIP(hipGetLastError());
  ctx->counters.last_nq = nq; ctx->counters.last_k = k;
  if (ctx->l2_cross_check_q)                                // todhip_set_l2_cross_check: behind the ratio test and the radius cut
    return tod_cross_check_l2(ctx, d_q_desc, nq, ctx->l2_cross_check_q, nullptr, k, reinterpret_cast<uint32_t*>(d_counts),
                              reinterpret_cast<todhip_dmatch*>(d_matches), reinterpret_cast<float*>(d_matches_xyz));
  return TODHIP_OK;
}

int todhip_match_l2(todhip_ctx* ctx, const float* q_desc, uint32_t nq, uint32_t k, float radius, uint32_t* row_ptr,
                    todhip_dmatch* matches, float* matches_xyz) {
  if (!ctx || (!q_desc && nq) || !row_ptr || (nq && (!matches || !matches_xyz))) return TODHIP_EINVAL;
  if (k == 0 || k > kTop || !(radius > 0.f)) return TODHIP_EINVAL;
  const int db = l2_db_check(ctx);
  if (db == TODHIP_ENODB) return db;
  row_ptr[0] = 0;
  if (nq == 0) return TODHIP_OK;                            // before the DB's type is looked at
  if (db != TODHIP_OK) return db;
  TOD_HIP(hipSetDevice(ctx->device));
  const size_t cap = (size_t)nq * k;
  TOD_HIP(ctx->m_q.reserve((size_t)nq * ctx->desc_bytes));
  TOD_HIP(ctx->m_counts.reserve((size_t)nq * 4));
  TOD_HIP(ctx->m_matches.reserve(cap * sizeof(todhip_dmatch)));
  TOD_HIP(ctx->m_xyz.reserve(cap * 12));
  TOD_HIP(hipMemcpyAsync(ctx->m_q.p, q_desc, (size_t)nq * ctx->desc_bytes, hipMemcpyHostToDevice, ctx->stream));
  int rc = todhip_match_l2_device(ctx, ctx->m_q.p, nq, k, radius, ctx->m_counts.p, ctx->m_matches.p, ctx->m_xyz.p);
  if (rc != TODHIP_OK) return rc;
  std::vector<uint32_t> counts(nq);
  std::vector<todhip_dmatch> m(cap);
  std::vector<float> x(cap * 3);
  TOD_HIP(hipMemcpyAsync(counts.data(), ctx->m_counts.p, (size_t)nq * 4, hipMemcpyDeviceToHost, ctx->stream));
  TOD_HIP(hipMemcpyAsync(m.data(), ctx->m_matches.p, cap * sizeof(todhip_dmatch), hipMemcpyDeviceToHost, ctx->stream));
  TOD_HIP(hipMemcpyAsync(x.data(), ctx->m_xyz.p, cap * 12, hipMemcpyDeviceToHost, ctx->stream));
  TOD_HIP(hipStreamSynchronize(ctx->stream));
  tod_pack_csr(counts.data(), m.data(), x.data(), nq, k, row_ptr, matches, matches_xyz);
  return TODHIP_OK;
}

}  // extern "C"
