// The exact k-NN search over a DB of 64-byte (512-bit) binary descriptors -- BRISK, FREAK, AKAZE zero-padded from 61 bytes, BRIEF-64
// (definition: include/todhip.h). The reference's DescriptorMatcher cell hands whatever cv::Mat its FeatureDescriptor
// cell produced to a cv::DescriptorMatcher (DescriptorMatcher.cpp:195-252), at any width; this is the second binary width here.
// It stands beside hamming_topk_mfma (match_mfma.h), not in it: the 32-byte kernels are not touched.
//
//   W1 hamming_topk_wide     the DB pass, K4x's formulation on match_fp4.h's primitives. One wave = (DB tile, 32 QT queries); a
//                            32 x 32 block is 8 MFMAs (two 256-bit halves, dot = 512 - 2 d, exact in f32). Every lane keeps the k best
//                            partial keys (distance << 22 | tile-local row: the 10 bits a distance <= 512 needs) of its half of the
//                            rows, a block is tested against the lanes' thresholds (block_reaches, in the shadow of the next block's
//                            MFMAs) and only a block with a hit walks its 16 registers. Bounds travel between tiles through the
//                            per-query word of K4 / K4x. Whole blocks only: no split after the first 256 bits.
// Behind it everything is shared: merge_tiles_kernel (match_merge.h) widens the partial keys, and the lists go the way of the 32-byte
// search's (tod_match_lists, match.hip: the one wrapper of both widths; select_keys_kernel, finalize_kernel, the shard merge).
#include <algorithm>

#include "ctx.h"
#include "row_ops.h"

namespace {

#include "match_keys.h"
#include "match_fp4.h"
#include "match_merge.h"
#include "match_plan.h"

using W = RowBits<512>;

// The test of one accumulator block, as mfma_block_test: nothing unless some lane's best dot product beats its threshold, then the
// walk. The walk masks the rows behind the tile's end (the DB's last, partial step reads the slack). IMAX: thresholds are >= 0.
template <int K, bool IMAX>
__device__ __forceinline__ void wide_block_test(const mfma_f32x16& acc, float& thr, uint32_t r_lane, uint32_t n_local, uint32_t (&best)[K]) {
  if (__builtin_amdgcn_ballot_w64(block_reaches<IMAX, false>(acc, thr)) == 0ull) return;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t row = r_lane | block_row(i);              // r_lane = lane_row_base(step): the tile-local row
    const bool hit = acc[i] > thr && row < n_local;
    if (__builtin_amdgcn_ballot_w64(hit) != 0ull) {
      // key = distance << 22 | row: (512 - dot) * 2^21 is an exact integer <= 2^31 (dot is an even integer in [-512, 512])
      const uint32_t key = (uint32_t)((512.f - acc[i]) * 2097152.f) | row;
      topk_insert<K>(best, hit ? key : 0xFFFFFFFFu);
    }
  }
  thr = fmaxf(thr, W::thr_of_limit(best[K - 1] >> kLocalBits));   // thresholds only ever tighten
}

// W1. Work item = (tile, query wave), consecutive items share a tile. The loop over the tile's steps is match_fp4.h's
// block_step_loop; the test of a block is wide_block_test; behind a step the bounds are exchanged, and at the end the lists stored, by
// the functions hamming_topk_fp4rows uses (exchange_bounds, store_tile_lists).
// cut = radius + 1 (kNoLimit: none); IMAX: cut <= 256, every threshold >= 0. Output: K4's partial lists and flag bytes (match_merge.h
// reads them).
template <int K, int QT, bool IMAX>
__global__ __launch_bounds__(kBlock, 2) void hamming_topk_wide(const uint32_t* __restrict__ db, const uint32_t* __restrict__ q,
                                                               uint32_t n_rows, uint32_t nq, uint32_t nq_pad, uint32_t rows_per_tile,
                                                               uint32_t n_tiles, uint32_t n_qw, uint32_t n_qw64, uint32_t cut,
                                                               uint32_t share_period, uint32_t* __restrict__ part, uint32_t* bound,
                                                               uint8_t* __restrict__ stored) {
  static_assert(QT % 2 == 0 && QT >= 2, "two query blocks share a 64-query flag byte");
  const uint32_t item = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
  const uint32_t tile = item / n_qw, qw = item % n_qw;
  if (tile >= n_tiles) return;
  const uint32_t lane = threadIdx.x & 63u, c = lane & 31u, h = lane >> 5;
  const uint32_t q0 = qw * (32u * QT);
  const Fp4Consts kc = fp4_consts();
  W::Frag qb[QT];
  uint32_t best[QT][K], seen[QT];
  float thr[QT];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    W::load_query_block(q, q0 + 32u * t + c, nq, h, qb[t], kc);
#pragma unroll
    for (int j = 0; j < K; ++j) best[t][j] = 0xFFFFFFFFu;
    thr[t] = W::thr_of_limit(cut);
    seen[t] = 0xFFFFFFFFu;                                   // "nothing published"
  }
  const uint32_t row0 = tile * rows_per_tile;               // < n_rows: tile < n_tiles
  const uint32_t n_local = min(rows_per_tile, n_rows - row0);
  uint32_t next_share = 2u;                                 // first exchange after 64 rows, as K4
  block_step_loop<W, QT>(
      db, row0, n_local, c, h, qb, kc,
      [&](const mfma_f32x16& acc, int t, uint32_t r_lane) { wide_block_test<K, IMAX>(acc, thr[t], r_lane, n_local, best[t]); },
      [&](uint32_t step) {
        if (step + 1u < next_share) return;                 // wave-uniform
        next_share += share_period;
        exchange_bounds<K, QT>(bound, q0, c, nq, best, seen, thr, [](uint32_t limit) { return W::thr_of_limit(limit); }, [](int) {});
      });
  store_tile_lists<K, QT>(best, tile, q0, nq, nq_pad, n_qw64, lane, c, h, part, stored);
}

// One launch on the shared plan (match_plan.h): tiling, workspaces, the DB pass, the tile merge. The grid is linear: the kernel's
// work-item decode knows no XCDs.
template <int K, int QT>
int launch_wide(todhip_ctx* ctx, const uint32_t* d_q, uint32_t nq, uint32_t radius, uint64_t* d_lists, uint32_t* n_lists) {
  const uint32_t cut = radius >= 512u ? kNoLimit : radius + 1u;     // distances are <= 512: no cut beyond that
  const uint32_t n_rows = (uint32_t)tod_db_n_rows(ctx);
  const uint32_t n_qw = (nq + 32u * QT - 1u) / (32u * QT), n_qw64 = (nq + 63u) / 64u, nq_pad = n_qw64 * 64u;
  // about 16 waves per CU (two rounds of the 8 that fit), tiles of at least 256 rows: the radius pass's plan, not tuned further
  Tiling t;
  if (!finish_tiling(n_rows, mfma_tile_rows(n_rows, (uint32_t)ctx->n_cu * 16u / n_qw, 256u, false), n_qw, &t)) return TODHIP_EINVAL;
  if ((uint64_t)t.n_tiles * n_qw > 0x7FFFFFFFull) return TODHIP_EINVAL;   // the kernel numbers its work items in 32 bits
  uint8_t* const d_stored = prepare_lists<K>(ctx, t.n_tiles, nq_pad, n_qw64);
  if (!d_stored) return TODHIP_EHIP;
  KernelTimer timer{ctx};                                           // the DB pass between two events, as K4 / K4x / R1
  if (int rc = timer.begin()) return rc;
  auto kern = cut <= 256u ? hamming_topk_wide<K, QT, true> : hamming_topk_wide<K, QT, false>;
  hipLaunchKernelGGL(kern, dim3(t.blocks), dim3(kBlock), 0, ctx->stream, reinterpret_cast<const uint32_t*>(tod_db_rows(ctx)), d_q, n_rows, nq,
                     nq_pad, t.rows_per_tile, t.n_tiles, n_qw, n_qw64, cut, 16u, ctx->m_part.as<uint32_t>(), ctx->m_bound.as<uint32_t>(), d_stored);
  if (int rc = timer.end()) return rc;
  TOD_HIP(hipGetLastError());
  ctx->counters.last_block_split = 4;                               // whole blocks: the one form there is
  return launch_merge<K>(ctx, nq, nq_pad, t, d_stored, n_qw64, nullptr, d_lists, n_lists);
}

// Query blocks per wave: a block's expanded fragments are 32 registers at this width. Four blocks (128) beside the row (32), two
// accumulators (32), the packed rows in flight (8) and the lists (4 k) stay inside the 256 registers of two waves per SIMD up to
// k = 3 (255 registers at k = 3; k = 4 spills); from k = 4 on, and for the <= 64 queries of a small frame (no padding blocks), two.
template <int K>
int launch_wide_k(todhip_ctx* ctx, const uint32_t* d_q, uint32_t nq, uint32_t radius, uint64_t* d_lists, uint32_t* n_lists) {
  constexpr int kMaxQT = K <= 3 ? 4 : 2;
  if (nq <= 64u) return launch_wide<K, 2>(ctx, d_q, nq, radius, d_lists, n_lists);
  return launch_wide<K, kMaxQT>(ctx, d_q, nq, radius, d_lists, n_lists);
}

}  // namespace

// tod_match_lists' search at this width (ctx.h): the active rows, at least one; k in 1..8
int tod_wide_lists_active(todhip_ctx* ctx, const void* d_q, uint32_t nq, uint32_t k, uint32_t radius, uint64_t* d_lists, uint32_t* n_lists) {
  if (ctx->ratio > 0.f) radius = 512u;   // the ratio test needs the true second neighbour, however far: no radius bound in the search
  const uint32_t* q = reinterpret_cast<const uint32_t*>(d_q);
  return dispatch_k(k, [&](auto K) { return launch_wide_k<decltype(K)::value>(ctx, q, nq, radius, d_lists, n_lists); });
}
