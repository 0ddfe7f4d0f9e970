// Lowe's ratio test against another object (definition: include/todhip.h; predicate, limit and interval: ratio_other.h).
// A TOD model DB holds a surface point once per training view, so a correct match's two nearest rows are the same point twice and
// todhip_set_ratio_test throws it away; Lowe's paper takes the second neighbour from a DIFFERENT object. This file computes that
// neighbour's distance for every query and filters a fixed-stride match output with it. It stands beside the tuned kernels as
// match_radius.hip and cross_check.hip do and shares match_fp4.h's primitives with them, nothing else.
//
//   O1 other_setup_kernel      thread = query: the excluded object's interval of searched rows (from a table the host keeps per DB
//                              state: it reads no DB rows), and d_min[q] = min(limit, cap) -- every word of the output is written
//                              here. In the filter's form the object and the limit come from slot 0 of the query's matches.
//   O2 other_object_min_mfma   the DB pass. One wave = (DB tile, 32 QT queries), block_step_loop over the tile. Per lane and query
//                              block: a threshold and the excluded interval in tile-local rows. A block walks only when some lane's
//                              best dot product beats its threshold (block_reaches); the walk keeps the maximum over the rows inside
//                              the tile and outside the interval. Distances only: no rows, no lists, no ties. The bound travels
//                              through the output word: atomicMin once per share period and at the end, a relaxed load to tighten.
//                              A query whose limit is 0 (no kept match) or already reached elsewhere never walks.
//   O3 ratio_other_apply_kernel  thread = query: counts[q] = 0 where the predicate fails on slot 0 and d_min[q].
#include <algorithm>
#include <vector>

#include "ctx.h"
#include "ratio_other.h"
#include "row_ops.h"

namespace {

#include "match_keys.h"
#include "match_fp4.h"

constexpr uint32_t kNone = tod::kRatioOtherNone;
constexpr uint32_t kSharePeriod32 = 16u;                    // 32-row steps between two exchanges, as W1

struct OtherWs : TodWs {
  static constexpr int kSlot = kWsOther;
  std::vector<tod::RowInterval> h_obj_iv;                    // object -> its interval of searched rows (empty: none searched)
  DevBuf obj_iv;
  uint64_t iv_gen = 0;                                       // ctx->rows_gen the table was built at (0: never)
  DevBuf q_iv;                                               // per query: the excluded interval
  DevBuf d_min;                                              // the filter's own other-object minima
};

// O1. matches == nullptr: the primitive's form (excl[nq]; limit[nq] or nullptr = none). Otherwise the filter's form: the object and
// the limit of slot 0 (a query without a kept match: limit 0, nothing excluded, never walked).
__global__ __launch_bounds__(kBlock) void other_setup_kernel(uint32_t nq, const uint32_t* __restrict__ excl, const uint32_t* __restrict__ limit,
                                                             uint32_t cap, const uint32_t* __restrict__ counts,
                                                             const todhip_dmatch* __restrict__ matches, uint32_t stride, float ratio,
                                                             const tod::RowInterval* __restrict__ obj_iv, uint32_t n_objs,
                                                             tod::RowInterval* __restrict__ q_iv, uint32_t* __restrict__ d_min) {
  const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
  if (q >= nq) return;
  uint32_t o = kNone, lim = kNone;
  if (matches) {
    lim = 0u;
    if (counts[q] != 0u) {
      const todhip_dmatch m0 = matches[(size_t)q * stride];
      o = (uint32_t)m0.imgIdx;
      lim = tod::ratio_other_limit((uint32_t)m0.distance, ratio);
    }
  } else {
    o = excl[q];
    if (limit) lim = limit[q];
  }
  q_iv[q] = o < n_objs ? obj_iv[o] : tod::RowInterval{0u, 0u};   // kNone, or no object of this DB: no row is excluded
  d_min[q] = min(lim, cap);
}

// O2's block test. thr: dot > thr <=> d < the bound known to this lane. iv: tile-local, clamped to the tile.
template <bool IMAX>
__device__ __forceinline__ void other_block_test(const mfma_f32x16& acc, float& thr, uint32_t r_lane, uint32_t n_local, tod::RowInterval iv) {
  if (__builtin_amdgcn_ballot_w64(block_reaches<IMAX, false>(acc, thr)) == 0ull) return;
  float m = thr;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t row = r_lane + block_row(i);              // tile-local; r_lane = lane_row_base(step)
    const bool ok = row < n_local && tod::ratio_other_counts(row, iv);
    m = ok ? fmaxf(m, acc[i]) : m;
  }
  thr = m;                                                   // thresholds only ever tighten
}

// O2. Work item = (tile, query wave), consecutive items share a tile, as R1 and W1. IMAX: every d_min[q] is <= BITS / 2 when the
// kernel starts (the host's cap), so every threshold is >= 0.
template <int BITS, int QT, bool IMAX>
__global__ __launch_bounds__(kBlock, 2) void other_object_min_mfma(const uint32_t* __restrict__ db, const uint32_t* __restrict__ q,
                                                                   uint32_t n_rows, uint32_t nq, uint32_t rows_per_tile, uint32_t n_tiles,
                                                                   uint32_t n_qw, const tod::RowInterval* __restrict__ q_iv,
                                                                   uint32_t* d_min) {
  using W = RowBits<BITS>;
  const uint32_t item = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
  const uint32_t tile = item / n_qw, qw = item % n_qw;
  if (tile >= n_tiles) return;
  const uint32_t lane = threadIdx.x & 63u, c = lane & 31u, h = lane >> 5;
  const uint32_t q0 = qw * (32u * QT);
  const uint32_t row0 = tile * rows_per_tile;               // < n_rows: tile < n_tiles
  const uint32_t n_local = min(rows_per_tile, n_rows - row0);
  const Fp4Consts kc = fp4_consts();
  typename W::Frag qb[QT];
  float thr[QT];
  uint32_t seen[QT];                                        // the bound last read from (or written to) d_min, at most BITS + 1
  tod::RowInterval iv[QT];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const uint32_t qi = q0 + 32u * t + c;
    W::load_query_block(q, qi, nq, h, qb[t], kc);
    seen[t] = 0u;                                            // a padding query: dot > BITS never holds
    iv[t] = tod::RowInterval{0u, 0u};
    if (qi < nq) {
      seen[t] = min(d_min[qi], (uint32_t)BITS + 1u);         // kNone: every distance is below BITS + 1
      const tod::RowInterval g = q_iv[qi];
      iv[t] = tod::ratio_other_clamp(g.lo, g.hi, row0, n_local);
    }
    thr[t] = W::thr_of_limit(seen[t]);
  }
  // publish a lane's own minimum where it improves on what was seen (lanes l and l + 32 hold the two halves of a query's rows; both
  // publish), and with `reload` take what the other tiles have published since
  auto exchange = [&](bool reload) {
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      const uint32_t qi = q0 + 32u * t + c;
      if (qi >= nq) continue;
      const uint32_t mine = (uint32_t)(((float)BITS - thr[t]) * 0.5f);   // exact: thr is BITS - 2 d
      if (mine < seen[t]) atomicMin(d_min + qi, mine);
      if (reload) {
        seen[t] = min(__hip_atomic_load(d_min + qi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), (uint32_t)BITS + 1u);
        thr[t] = fmaxf(thr[t], W::thr_of_limit(seen[t]));
      }
    }
  };
  uint32_t next_share = 2u;                                 // first exchange after 64 rows, as K4
  block_step_loop<W, QT>(
      db, row0, n_local, c, h, qb, kc,
      [&](const mfma_f32x16& acc, int t, uint32_t r_lane) { other_block_test<IMAX>(acc, thr[t], r_lane, n_local, iv[t]); },
      [&](uint32_t step) {
        if (step + 1u < next_share) return;                 // wave-uniform
        next_share += kSharePeriod32;
        exchange(true);
      });
  exchange(false);
}

// O3
__global__ __launch_bounds__(kBlock) void ratio_other_apply_kernel(uint32_t nq, uint32_t stride, float ratio, const uint32_t* __restrict__ other_min,
                                                                   uint32_t* __restrict__ counts, const todhip_dmatch* __restrict__ matches) {
  const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
  if (q >= nq || counts[q] == 0u) return;
  const uint32_t d1 = (uint32_t)matches[(size_t)q * stride].distance;
  if (!tod::ratio_other_survives(d1, ratio, other_min[q])) counts[q] = 0u;
}

// object -> its interval in the numbering of the searched rows (the shard, or the selection's view), rebuilt when the rows changed
int object_intervals(todhip_ctx* ctx, OtherWs* ws) {
  if (ws->iv_gen == ctx->rows_gen) return TODHIP_OK;
  const uint32_t n = ctx->n_objs;
  ws->h_obj_iv.assign(n, tod::RowInterval{0u, 0u});
  if (ctx->sel_on) {
    const TodViewTables& s = ctx->sel;
    for (uint32_t j = 0; j < s.n_segs(); ++j) ws->h_obj_iv[s.seg_obj[j]] = tod::RowInterval{s.seg_view[j], s.seg_view[j + 1]};
  } else {
    for (uint32_t o = 0; o < n; ++o)
      ws->h_obj_iv[o] = tod::ratio_other_clamp(ctx->h_obj_off[o], ctx->h_obj_off[o + 1], ctx->shard_first, ctx->shard_rows);
  }
  TOD_HIP(ws->obj_iv.reserve((size_t)n * sizeof(tod::RowInterval)));
  // (pageable source that the workspace keeps: the copy runs behind the kernels of an earlier call that read the old table)
  TOD_HIP(hipMemcpyAsync(ws->obj_iv.p, ws->h_obj_iv.data(), (size_t)n * sizeof(tod::RowInterval), hipMemcpyHostToDevice, ctx->stream));
  ws->iv_gen = ctx->rows_gen;
  return TODHIP_OK;
}

template <int BITS, int QT>
int launch_other(todhip_ctx* ctx, const uint32_t* d_q, uint32_t nq, bool imax, const tod::RowInterval* q_iv, uint32_t* d_min) {
  const uint32_t n_rows = (uint32_t)tod_db_n_rows(ctx);
  const uint32_t n_qw = (nq + 32u * QT - 1u) / (32u * QT);
  // the radius pass's plan: about 16 waves per CU, tiles of at least 256 rows
  const Tiling t = tile_plan(n_rows, mfma_tile_rows(n_rows, (uint32_t)ctx->n_cu * 16u / n_qw, 256u, false), n_qw, kWavesPerBlock, 1u);
  if ((uint64_t)t.n_tiles * n_qw > 0x7FFFFFFFull) return TODHIP_EINVAL;   // the kernel numbers its work items in 32 bits
  auto kern = imax ? other_object_min_mfma<BITS, QT, true> : other_object_min_mfma<BITS, QT, false>;
  hipLaunchKernelGGL(kern, dim3(t.blocks), dim3(kBlock), 0, ctx->stream, reinterpret_cast<const uint32_t*>(tod_db_rows(ctx)), d_q, n_rows, nq,
                     t.rows_per_tile, t.n_tiles, n_qw, q_iv, d_min);
  TOD_HIP(hipGetLastError());
  return TODHIP_OK;
}

// O1 and O2 behind the argument checks. d_matches == nullptr: the primitive (d_excl, d_limit); otherwise the filter's form.
int other_min(todhip_ctx* ctx, const void* d_q, uint32_t nq, const uint32_t* d_excl, const uint32_t* d_limit, uint32_t cap,
              const uint32_t* d_counts, const todhip_dmatch* d_matches, uint32_t stride, float ratio, uint32_t* d_min) {
  OtherWs* ws = tod_ws<OtherWs>(ctx);
  if (int rc = object_intervals(ctx, ws)) return rc;
  TOD_HIP(ws->q_iv.reserve((size_t)nq * sizeof(tod::RowInterval)));
  tod::RowInterval* const q_iv = ws->q_iv.as<tod::RowInterval>();
  hipLaunchKernelGGL(other_setup_kernel, dim3((nq + kBlock - 1u) / kBlock), dim3(kBlock), 0, ctx->stream, nq, d_excl, d_limit, cap, d_counts,
                     d_matches, stride, ratio, ws->obj_iv.as<tod::RowInterval>(), ctx->n_objs, q_iv, d_min);
  TOD_HIP(hipGetLastError());
  if (tod_db_n_rows(ctx) == 0 || cap == 0u) return TODHIP_OK;   // an empty selection, a shard without a (selected) row: min(limit, cap)
  const bool wide = ctx->desc_bytes == 64;
  if (!wide && ctx->bit_order_on) {                         // todhip_set_db_bit_order: the queries follow the rows
    int rc = tod_bit_order_queries(ctx, d_q, nq, &d_q);
    if (rc != TODHIP_OK) return rc;
  }
  const uint32_t* q = reinterpret_cast<const uint32_t*>(d_q);
  // query blocks per wave: the radius pass's choice at 32 bytes, the wide pass's at 64 (DESIGN 6q has the register figures)
  if (wide) {
    const bool imax = cap <= 256u;
    if (nq <= 64u) return launch_other<512, 2>(ctx, q, nq, imax, q_iv, d_min);
    return launch_other<512, 4>(ctx, q, nq, imax, q_iv, d_min);
  }
  const bool imax = cap <= 128u;
  if (nq <= 64u) return launch_other<256, 2>(ctx, q, nq, imax, q_iv, d_min);
  if (nq <= 1024u) return launch_other<256, 4>(ctx, q, nq, imax, q_iv, d_min);
  return launch_other<256, 6>(ctx, q, nq, imax, q_iv, d_min);
}

void apply(todhip_ctx* ctx, float ratio, uint32_t nq, uint32_t stride, const uint32_t* d_other_min, uint32_t* d_counts,
           const todhip_dmatch* d_matches) {
  hipLaunchKernelGGL(ratio_other_apply_kernel, dim3((nq + kBlock - 1u) / kBlock), dim3(kBlock), 0, ctx->stream, nq, stride, ratio, d_other_min,
                     d_counts, d_matches);
}

bool ratio_ok(float ratio) { return ratio > 0.f && ratio <= 1.f; }   // (false for a NaN)

int binary_db(const todhip_ctx* ctx) {
  if (ctx->total_rows == 0) return TODHIP_ENODB;
  if (ctx->desc_bytes != 32 && ctx->desc_bytes != 64) return TODHIP_EINVAL;    // a float DB
  return TODHIP_OK;
}

}  // namespace

int tod_ratio_other(todhip_ctx* ctx, const void* d_q, uint32_t nq, float ratio, uint32_t max_d1, uint32_t stride, uint32_t* d_counts,
                    todhip_dmatch* d_matches) {
  OtherWs* ws = tod_ws<OtherWs>(ctx);
  TOD_HIP(ws->d_min.reserve((size_t)nq * sizeof(uint32_t)));
  // the limit of the largest possible d1: no query's limit is above it (the limit does not fall as d1 grows)
  const uint32_t cap = tod::ratio_other_limit(std::min(max_d1, ctx->desc_bytes * 8u), ratio);
  if (int rc = other_min(ctx, d_q, nq, nullptr, nullptr, cap, d_counts, d_matches, stride, ratio, ws->d_min.as<uint32_t>())) return rc;
  apply(ctx, ratio, nq, stride, ws->d_min.as<uint32_t>(), d_counts, d_matches);
  TOD_HIP(hipGetLastError());
  return TODHIP_OK;
}

extern "C" int todhip_other_object_min_device(todhip_ctx* ctx, const void* d_q_desc, uint32_t nq, const void* d_excl_obj, const void* d_limit,
                                              uint32_t limit_cap, void* d_min) {
  if (!ctx || !d_q_desc || !d_excl_obj || !d_min || nq == 0) return TODHIP_EINVAL;
  if (int rc = binary_db(ctx)) return rc;
  TOD_HIP(hipSetDevice(ctx->device));
  return other_min(ctx, d_q_desc, nq, reinterpret_cast<const uint32_t*>(d_excl_obj), reinterpret_cast<const uint32_t*>(d_limit), limit_cap,
                   nullptr, nullptr, 0u, 0.f, reinterpret_cast<uint32_t*>(d_min));
}

extern "C" int todhip_ratio_other_apply_device(todhip_ctx* ctx, float ratio, uint32_t nq, uint32_t stride, const void* d_other_min,
                                               void* d_counts, const void* d_matches) {
  if (!ctx || !d_other_min || !d_counts || !d_matches) return TODHIP_EINVAL;
  if (nq == 0 || stride == 0 || stride > 1024 || !ratio_ok(ratio)) return TODHIP_EINVAL;
  if (int rc = binary_db(ctx)) return rc;
  TOD_HIP(hipSetDevice(ctx->device));
  apply(ctx, ratio, nq, stride, reinterpret_cast<const uint32_t*>(d_other_min), reinterpret_cast<uint32_t*>(d_counts),
        reinterpret_cast<const todhip_dmatch*>(d_matches));
  TOD_HIP(hipGetLastError());
  return TODHIP_OK;
}

extern "C" int todhip_ratio_other_device(todhip_ctx* ctx, const void* d_q_desc, uint32_t nq, float ratio, uint32_t stride, void* d_counts,
                                         void* d_matches) {
  if (!ctx || !d_q_desc || !d_counts || !d_matches) return TODHIP_EINVAL;
  if (nq == 0 || stride == 0 || stride > 1024 || !ratio_ok(ratio)) return TODHIP_EINVAL;
  if (int rc = binary_db(ctx)) return rc;
  if (ctx->shard_rows != ctx->total_rows) return TODHIP_EINVAL;                // one shard's minimum is not the DB's: the two calls above
  TOD_HIP(hipSetDevice(ctx->device));
  return tod_ratio_other(ctx, d_q_desc, nq, ratio, ctx->desc_bytes * 8u, stride, reinterpret_cast<uint32_t*>(d_counts), reinterpret_cast<todhip_dmatch*>(d_matches));
}

extern "C" int todhip_set_ratio_test_other(todhip_ctx* ctx, float ratio) {
  if (!ctx || !(ratio >= 0.f) || ratio > 1.f) return TODHIP_EINVAL;
  // a float DB has no Hamming rows, one shard of several does not see every other object (switching off always works)
  if (ratio > 0.f && ctx->total_rows && (binary_db(ctx) != TODHIP_OK || ctx->shard_rows != ctx->total_rows)) return TODHIP_EINVAL;
  ctx->ratio_other = ratio;
  return TODHIP_OK;
}
