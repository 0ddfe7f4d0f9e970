// todhip_match_radius[_device]: the true radius search -- every searched row within `radius` bits of a query, counted exactly, the
// nearest max_per_query of them returned (definition: include/todhip.h). The reference documents its `radius` as "for
// epsilon nearest neighbor search" (DescriptorMatcher.cpp:137) and says what it wanted at :201-220 ("Perform radius search. As this
// does not work for LSH on OpenCV 2.4, we first perform knn"); todhip_match restates that workaround, this file the intent
// (cv::DescriptorMatcher::radiusMatch).
//
//   R1 radius_collect_mfma   the DB pass. One wave = (DB tile, 32 QT queries), the distances of a 32 x 32 block on the matrix cores
//                            in K4x's +-1 fp4 form (match_fp4.h: dot = 256 - 2 d, exact). No lists, no bounds: a block is tested
//                            for "any dot >= 256 - 2 radius" (block_reaches, in the shadow of the next block's MFMAs) and only
//                            a block with a hit walks its 16 registers. A pair inside the radius adds 1 to hist[q][d], takes a
//                            position from the query's cursor and, while that is below the buffer's capacity C, stores its key
//                            (d << 32 | searched row) there. The cursor ends as |R(q)|, whatever C is.
//   R2 radius_select_kernel  one workgroup per query. |R(q)| <= C: the buffer holds all of R(q); a bitonic sort in LDS puts it in key
//                            order (keys are unique, so the order the atomics landed in does not matter). |R(q)| > C: an ordered
//                            rescan -- the workgroup streams the searched rows in ascending order, and a row at distance d goes to
//                            position cum_hist(d - 1) + (rows at d seen so far): a counting sort, exact under any number of ties.
//                            Only distances up to d* (the one at which cum_hist reaches max_per_query) take part, and the stream
//                            ends once max_per_query positions are filled. Both forms leave the query's first
//                            min(|R(q)|, max_per_query) keys at the head of its buffer.
//   R3 radius_emit_kernel    thread = output slot: searched row -> row of the full DB, then match_keys.h's store_match (object
//                            lookup and 3D gather, as K4f). Slots behind counts[q] are not written.
// Rows are numbered within what is searched (the shard, or the selection's view) until R3: both maps to the full DB are increasing,
// so the order (distance, searched row) is the order (distance, global row) of decision D1.
//
// Over a sharded DB (todhip_match_radius_shard_device + todhip_merge_radius_shards_device[_on]) a rank runs R1 and R2 on
// its shard and sends what they leave, and the owner of a query merges the ranks' answers:
//   S1 radius_shard_keys_kernel   instead of R3: the query's first max_per_query keys with rows of the full DB, padding, and |R_s(q)|.
//   M1 radius_merge_kernel        a rank merge of the shards' lists by binary search, then store_match. The global first
//                                 max_per_query lie inside the union of the per-shard first max_per_query.
#include <algorithm>

#include "ctx.h"
#include "row_ops.h"
#include "shard_merge.h"

namespace {

#include "match_keys.h"
#include "match_fp4.h"

constexpr uint32_t kMaxPerQuery = 1024;
constexpr uint32_t kMaxCap = 2048;                          // radius_capacity(kMaxPerQuery): R2's LDS image of one buffer (16 KB)
constexpr uint32_t kRescanRows = 4;                         // rows per thread in flight in R2's rescan

// C: a query's candidate buffer holds this many keys. Twice max_per_query, at least 64, rounded up to a power of two (the bitonic
// sort's size): a query that overflows has more than two full answers inside the radius, and the workspace stays nq * C * 8 bytes.
uint32_t radius_capacity(uint32_t max_per_query) {
  uint32_t c = 64;
  while (c < 2u * max_per_query) c <<= 1;
  return c;
}

struct RadiusWs : TodWs {
  static constexpr int kSlot = kWsRadius;
  DevBuf count;                                             // cursor[nq], then hist[nq][min(radius, 256) + 1]: one memset
  DevBuf cand;                                              // nq x C keys
  DevBuf counts, in_radius;                                 // the host form's device-side counts
};

struct CollectOut {
  uint32_t hist_stride, cap;
  uint32_t* cursor;
  uint32_t* hist;
  uint64_t* cand;
};

// The test of one accumulator block. thr = 256 - 2 min(radius, 256): dot >= thr <=> d <= radius. IMAX: radius < 128, thr > 0. The
// walk masks what the block test cannot: rows behind the tile's end (n_local) and the padding queries behind nq (q_ok).
template <bool IMAX>
__device__ __forceinline__ void radius_block_test(const mfma_f32x16& acc, float thr, uint32_t r_lane, uint32_t n_local, uint32_t row0,
                                                  uint32_t qi, bool q_ok, const CollectOut& o) {
  if (__builtin_amdgcn_ballot_w64(block_reaches<IMAX, true>(acc, thr)) == 0ull) return;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t row = r_lane + block_row(i);             // tile-local; r_lane = lane_row_base(step)
    const bool hit = acc[i] >= thr && row < n_local && q_ok;
    if (__builtin_amdgcn_ballot_w64(hit) == 0ull) continue;
    if (hit) {
      const uint32_t d = (uint32_t)((256.f - acc[i]) * 0.5f);          // exact: the dot product is an even integer in [-256, 256]
      atomicAdd(o.hist + (size_t)qi * o.hist_stride + d, 1u);           // d <= min(radius, 256) < hist_stride
      const uint32_t pos = atomicAdd(o.cursor + qi, 1u);
      if (pos < o.cap) o.cand[(size_t)qi * o.cap + pos] = ((uint64_t)d << 32) | (uint64_t)(row0 + row);
    }
  }
}

// R1. Work item = (tile, query wave), consecutive items share a tile (its rows come from L2 for all but the first reader). The
// loop over the tile's steps is match_fp4.h's block_step_loop; the test of a block is radius_block_test, nothing happens between steps.
template <int QT, bool IMAX>
__global__ __launch_bounds__(kBlock, 2) void radius_collect_mfma(const uint32_t* __restrict__ db, const uint32_t* __restrict__ q,
                                                                 uint32_t n_rows, uint32_t nq, uint32_t rows_per_tile, uint32_t n_tiles,
                                                                 uint32_t n_qw, float thr, CollectOut o) {
  using W = RowBits<256>;
  const uint32_t item = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
  const uint32_t tile = item / n_qw, qw = item % n_qw;
  if (tile >= n_tiles) return;
  const uint32_t lane = threadIdx.x & 63u, c = lane & 31u, h = lane >> 5;
  const uint32_t q0 = qw * (32u * QT);
  const Fp4Consts kc = fp4_consts();
  W::Frag qb[QT];
#pragma unroll
  for (int t = 0; t < QT; ++t) W::load_query_block(q, q0 + 32u * t + c, nq, h, qb[t], kc);
  const uint32_t row0 = tile * rows_per_tile;               // < n_rows: tile < n_tiles
  const uint32_t n_local = min(rows_per_tile, n_rows - row0);
  block_step_loop<W, QT>(
      db, row0, n_local, c, h, qb, kc,
      [&](const mfma_f32x16& acc, int t, uint32_t r_lane) {
        const uint32_t qi = q0 + 32u * t + c;
        radius_block_test<IMAX>(acc, thr, r_lane, n_local, row0, qi, qi < nq, o);
      },
      [](uint32_t) {});
}

// R2 (the comment at the head of the file). keys: the query's buffer, slots [min(n, C), C) still hold the fill value ~0.
__global__ __launch_bounds__(kBlock) void radius_select_kernel(const uint32_t* __restrict__ db, const uint32_t* __restrict__ q,
                                                               uint32_t n_rows, uint32_t radius, uint32_t max_per_query, uint32_t cap,
                                                               uint32_t hist_stride, const uint32_t* __restrict__ cursor,
                                                               const uint32_t* __restrict__ hist, uint64_t* __restrict__ cand,
                                                               uint32_t* __restrict__ counts, uint32_t* __restrict__ in_radius) {
  __shared__ uint64_t s_keys[kMaxCap];
  __shared__ uint32_t s_cum[257], s_run[257], s_dstar, s_written;
  const uint32_t qi = blockIdx.x, tid = threadIdx.x;
  const uint32_t n = cursor[qi];
  if (tid == 0) {
    counts[qi] = min(n, max_per_query);
    if (in_radius) in_radius[qi] = n;
  }
  if (n <= 1u) return;                                      // nothing, or one key that is in place
  uint64_t* const keys = cand + (size_t)qi * cap;
  if (n <= cap) {
    uint32_t P = 2;
    while (P < n) P <<= 1;                                  // <= cap; the slots behind n sort to the end (~0)
    for (uint32_t i = tid; i < P; i += kBlock) s_keys[i] = keys[i];
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1)
      for (uint32_t j = k >> 1; j > 0; j >>= 1) {
        for (uint32_t i = tid; i < P; i += kBlock) {
          const uint32_t l = i ^ j;
          if (l > i) {
            const uint64_t x = s_keys[i], y = s_keys[l];
            if (((i & k) == 0u) == (x > y)) { s_keys[i] = y; s_keys[l] = x; }
          }
        }
        __syncthreads();
      }
    const uint32_t n_out = min(n, max_per_query);
    for (uint32_t i = tid; i < n_out; i += kBlock) keys[i] = s_keys[i];
    return;
  }
  // ---- the ordered rescan: more rows inside the radius than the buffer holds (n > C >= 2 max_per_query)
  if (tid == 0) {
    uint32_t run = 0, dstar = hist_stride - 1u;
    bool found = false;
    for (uint32_t d = 0; d < hist_stride; ++d) {
      s_cum[d] = run;
      run += hist[(size_t)qi * hist_stride + d];
      if (!found && run >= max_per_query) { dstar = d; found = true; }
    }
    s_dstar = dstar;                                        // positions below max_per_query belong to distances <= dstar
    s_written = 0;
  }
  for (uint32_t d = tid; d < hist_stride; d += kBlock) s_run[d] = 0;
  __syncthreads();
  const uint32_t dstar = s_dstar, lane = tid & 63u, wave = tid >> 6;
  uint32_t qw[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) qw[w] = q[(size_t)qi * kWords + w];
  const uint4* const rows = reinterpret_cast<const uint4*>(db);
  for (uint64_t base = 0; base < n_rows; base += kBlock * kRescanRows) {
    uint32_t dist[kRescanRows];
#pragma unroll
    for (uint32_t u = 0; u < kRescanRows; ++u) {
      const uint64_t r = base + u * kBlock + tid;
      dist[u] = 0xFFFFu;
      if (r < n_rows) {
        const uint4 a = rows[2 * (size_t)r], b = rows[2 * (size_t)r + 1];
        dist[u] = hamming256(a, b, qw);
      }
    }
#pragma unroll
    for (uint32_t u = 0; u < kRescanRows; ++u) {
      const uint32_t d = dist[u];
      const uint64_t r = base + u * kBlock + tid;
      const bool need = d <= dstar;                         // dstar <= min(radius, 256): inside the radius
      if (!__syncthreads_or(need ? 1 : 0)) continue;
      for (uint32_t w = 0; w < (uint32_t)kWavesPerBlock; ++w) {   // ascending rows: the waves take turns, lanes rank by ballot
        if (wave == w) {
          uint64_t todo = __builtin_amdgcn_ballot_w64(need);
          while (todo) {
            const uint32_t leader = (uint32_t)__ffsll((unsigned long long)todo) - 1u;
            const uint32_t d0 = (uint32_t)__shfl((int)d, (int)leader);
            const bool mine = need && d == d0;
            const uint64_t same = __builtin_amdgcn_ballot_w64(mine);
            const uint32_t before = s_cum[d0] + s_run[d0], cnt = (uint32_t)__popcll(same);
            if (mine) {
              const uint32_t pos = before + (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
              if (pos < max_per_query) keys[pos] = ((uint64_t)d0 << 32) | r;
            }
            if (lane == leader) {
              s_run[d0] += cnt;
              s_written += before < max_per_query ? min(cnt, max_per_query - before) : 0u;
            }
            todo &= ~same;
          }
        }
        __syncthreads();
      }
      if (s_written >= max_per_query) return;               // (read behind a barrier, next written behind the next one: uniform)
    }
  }
}

// R3. cand: nq x cap keys whose first counts[q] are the query's answer, rows already those of the full DB but for first_row
__global__ __launch_bounds__(kBlock) void radius_emit_kernel(const uint64_t* __restrict__ cand, const uint32_t* __restrict__ counts,
                                                             uint32_t nq, uint32_t max_per_query, uint32_t cap, uint32_t first_row,
                                                             const uint32_t* __restrict__ obj_off, uint32_t n_objs,
                                                             const float* __restrict__ pts, todhip_dmatch* __restrict__ matches,
                                                             float* __restrict__ xyz) {
  const size_t slot = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t qi = (uint32_t)(slot / max_per_query), j = (uint32_t)(slot % max_per_query);
  if (qi >= nq || j >= counts[qi]) return;
  const uint64_t key = cand[(size_t)qi * cap + j];
  store_match(qi, (uint32_t)(key >> 32), (uint32_t)key + first_row, slot, obj_off, n_objs, pts, matches, xyz);
}

// S1. thread = slot of the nq x (max_per_query + 1) keys a shard sends: the first min(|R_s(q)|, max_per_query) keys of the query's
// buffer with rows of the full DB, padding behind them, |R_s(q)| in the last slot. Every slot is written. in_radius null: a shard
// without a searched row (cand is not read).
__global__ __launch_bounds__(kBlock) void radius_shard_keys_kernel(const uint64_t* __restrict__ cand, const uint32_t* __restrict__ in_radius,
                                                                   uint32_t nq, uint32_t max_per_query, uint32_t cap, uint32_t first_row,
                                                                   uint64_t* __restrict__ keys) {
  const size_t slot = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const uint32_t qi = (uint32_t)(slot / (max_per_query + 1u)), j = (uint32_t)(slot % (max_per_query + 1u));
  if (qi >= nq) return;
  const uint32_t n = in_radius ? in_radius[qi] : 0u;
  uint64_t v = ~0ull;
  if (j == max_per_query) v = n;
  else if (j < n) v = cand[(size_t)qi * cap + j] + first_row;           // (j < max_per_query; row + first_row < 2^32: no carry)
  keys[slot] = v;
}

// M1, the merge of the shards' radius answers: keys_all[n_shards][nq][max_per_query + 1] as S1 writes them. The rank merge by binary
// search of shard_merge.h (shard_rank_merge: its comment says why a position below max_per_query is right, how the threads share
// the elements of qpb queries, and what STAGED means), shared with the float keys' merge (l2_sharded.h); store_match resolves a key.
template <bool STAGED>
__global__ __launch_bounds__(kBlock) void radius_merge_kernel(const uint64_t* __restrict__ keys_all, uint32_t n_shards, uint32_t nq,
                                                              uint32_t max_per_query, uint32_t qpb, const uint32_t* __restrict__ obj_off,
                                                              uint32_t n_objs, const float* __restrict__ pts, uint32_t* __restrict__ counts,
                                                              uint32_t* __restrict__ in_radius, todhip_dmatch* __restrict__ matches,
                                                              float* __restrict__ xyz) {
  TOD_LATENCY_PRIO();   // latency-bound: win issue arbitration against the VALU-saturating matcher
  __shared__ uint64_t s_keys[STAGED ? kMergeLdsKeys : 1];
  shard_rank_merge<STAGED>(keys_all, n_shards, nq, max_per_query, qpb, counts, in_radius, s_keys, [&](uint64_t key, uint32_t qi, size_t at) {
    store_match(qi, (uint32_t)(key >> 32), (uint32_t)key, at, obj_off, n_objs, pts, matches, xyz);
  });
}

template <int QT>
void launch_collect(todhip_ctx* ctx, const uint32_t* d_q, uint32_t nq, uint32_t radius, const CollectOut& o) {
  const uint32_t n_rows = (uint32_t)tod_db_n_rows(ctx);
  const uint32_t n_qw = (nq + 32u * QT - 1u) / (32u * QT);
  // about 16 waves per CU (two rounds of the 8 that fit), tiles of at least 256 rows
  const Tiling t = tile_plan(n_rows, mfma_tile_rows(n_rows, (uint32_t)ctx->n_cu * 16u / n_qw, 256u, false), n_qw, kWavesPerBlock, 1u);   // no merge behind it
  const float thr = 256.f - 2.f * (float)std::min(radius, 256u);
  auto kern = radius < 128u ? radius_collect_mfma<QT, true> : radius_collect_mfma<QT, false>;
  hipLaunchKernelGGL(kern, dim3(t.blocks), dim3(kBlock), 0, ctx->stream, reinterpret_cast<const uint32_t*>(tod_db_rows(ctx)), d_q, n_rows, nq,
                     t.rows_per_tile, t.n_tiles, n_qw, thr, o);
}

// What R1 and R2 leave behind: nq x cap keys, the first min(|R(q)|, max_per_query) of a query's row its answer in key order, rows
// those of the full DB but for tod_db_first_row
struct RadiusKeys {
  const uint64_t* cand;
  uint32_t cap;
};

// R1 and R2 over the searched rows (there is at least one). d_counts / d_in_radius: where R2 writes min(|R(q)|, max_per_query) and
// |R(q)| (device memory; d_in_radius may be null).
int radius_keys(todhip_ctx* ctx, const void* d_q, uint32_t nq, uint32_t radius, uint32_t mpq, uint32_t* d_counts, uint32_t* d_in_radius,
                RadiusKeys* out) {
  const uint32_t n_rows = (uint32_t)tod_db_n_rows(ctx);
  if (ctx->bit_order_on) {                                  // todhip_set_db_bit_order: the queries follow the rows
    int rc = tod_bit_order_queries(ctx, d_q, nq, &d_q);
    if (rc != TODHIP_OK) return rc;
  }
  RadiusWs* ws = tod_ws<RadiusWs>(ctx);
  const uint32_t cap = radius_capacity(mpq), hist_stride = std::min(radius, 256u) + 1u;
  const size_t count_bytes = (size_t)nq * (1u + hist_stride) * sizeof(uint32_t), cand_bytes = (size_t)nq * cap * sizeof(uint64_t);
  TOD_HIP(ws->count.reserve(count_bytes));
  TOD_HIP(ws->cand.reserve(cand_bytes));
  TOD_HIP(hipMemsetAsync(ws->count.p, 0, count_bytes, ctx->stream));
  TOD_HIP(hipMemsetAsync(ws->cand.p, 0xFF, cand_bytes, ctx->stream));
  const CollectOut o{hist_stride, cap, ws->count.as<uint32_t>(), ws->count.as<uint32_t>() + nq, ws->cand.as<uint64_t>()};
  const uint32_t* q = reinterpret_cast<const uint32_t*>(d_q);
  KernelTimer timer{ctx};                                   // the DB pass between two events, as K4 / K4x
  if (int rc = timer.begin()) return rc;
  // query blocks per wave: two for a handful of queries, six (96 query registers beside no lists at all) for many frames' worth
  if (nq <= 64u) launch_collect<2>(ctx, q, nq, radius, o);
  else if (nq <= 1024u) launch_collect<4>(ctx, q, nq, radius, o);
  else launch_collect<6>(ctx, q, nq, radius, o);
  if (int rc = timer.end()) return rc;
  TOD_HIP(hipGetLastError());
  hipLaunchKernelGGL(radius_select_kernel, dim3(nq), dim3(kBlock), 0, ctx->stream, reinterpret_cast<const uint32_t*>(tod_db_rows(ctx)), q,
                     n_rows, radius, mpq, cap, hist_stride, o.cursor, o.hist, o.cand, d_counts, d_in_radius);
  TOD_HIP(hipGetLastError());
  if (ctx->sel_on) {                                        // view rows -> rows of the full DB (padding keys stay)
    int rc = tod_view_remap(ctx, o.cand, (size_t)nq * cap);
    if (rc != TODHIP_OK) return rc;
  }
  *out = RadiusKeys{o.cand, cap};
  return TODHIP_OK;
}

// Everything up to the outputs. d_counts / d_in_radius / d_matches / d_xyz: where the kernels write (device memory, or pinned host
// memory for the matches of the host form).
int radius_search(todhip_ctx* ctx, const void* d_q, uint32_t nq, uint32_t radius, uint32_t mpq, uint32_t* d_counts, todhip_dmatch* d_matches,
                  float* d_xyz, uint32_t* d_in_radius) {
  TOD_HIP(hipSetDevice(ctx->device));
  if (tod_db_n_rows(ctx) == 0) {                            // an empty selection, or a shard without a (selected) row
    TOD_HIP(hipMemsetAsync(d_counts, 0, (size_t)nq * sizeof(uint32_t), ctx->stream));
    if (d_in_radius) TOD_HIP(hipMemsetAsync(d_in_radius, 0, (size_t)nq * sizeof(uint32_t), ctx->stream));
    return TODHIP_OK;
  }
  RadiusKeys k;
  if (int rc = radius_keys(ctx, d_q, nq, radius, mpq, d_counts, d_in_radius, &k)) return rc;
  const size_t slots = (size_t)nq * mpq;
  hipLaunchKernelGGL(radius_emit_kernel, dim3((uint32_t)((slots + kBlock - 1u) / kBlock)), dim3(kBlock), 0, ctx->stream, k.cand, d_counts, nq,
                     mpq, k.cap, (uint32_t)tod_db_first_row(ctx), ctx->db_obj_off.as<uint32_t>(), ctx->n_objs, ctx->db_pts.as<float>(), d_matches,
                     d_xyz);
  TOD_HIP(hipGetLastError());
  return TODHIP_OK;
}

// The sharded form's first half: R1 and R2, then S1 into the caller's nq x (max_per_query + 1) keys
int radius_shard_keys(todhip_ctx* ctx, const void* d_q, uint32_t nq, uint32_t radius, uint32_t mpq, uint64_t* d_keys) {
  TOD_HIP(hipSetDevice(ctx->device));
  RadiusKeys k{nullptr, 0u};
  const uint32_t* d_in = nullptr;                           // no searched row: every query's count is 0
  if (tod_db_n_rows(ctx) != 0) {
    RadiusWs* ws = tod_ws<RadiusWs>(ctx);
    TOD_HIP(ws->counts.reserve((size_t)nq * sizeof(uint32_t)));
    TOD_HIP(ws->in_radius.reserve((size_t)nq * sizeof(uint32_t)));
    if (int rc = radius_keys(ctx, d_q, nq, radius, mpq, ws->counts.as<uint32_t>(), ws->in_radius.as<uint32_t>(), &k)) return rc;
    d_in = ws->in_radius.as<uint32_t>();
  }
  const size_t slots = (size_t)nq * (mpq + 1u);
  hipLaunchKernelGGL(radius_shard_keys_kernel, dim3((uint32_t)((slots + kBlock - 1u) / kBlock)), dim3(kBlock), 0, ctx->stream, k.cand, d_in, nq,
                     mpq, k.cap, (uint32_t)tod_db_first_row(ctx), d_keys);
  TOD_HIP(hipGetLastError());
  return TODHIP_OK;
}

// The sharded form's second half, M1 on `stream` (null: the context's). It reads the context's object table and model points only.
int radius_merge(todhip_ctx* ctx, hipStream_t stream, const uint64_t* d_keys_all, uint32_t n_shards, uint32_t nq, uint32_t mpq,
                 uint32_t* d_counts, todhip_dmatch* d_matches, float* d_xyz, uint32_t* d_in_radius) {
  TOD_HIP(hipSetDevice(ctx->device));
  const ShardMergeGrid g = shard_merge_grid(n_shards, nq, mpq);
  auto kern = g.staged ? radius_merge_kernel<true> : radius_merge_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(g.blocks), dim3(kBlock), 0, stream ? stream : ctx->stream, d_keys_all, n_shards, nq, mpq, g.qpb,
                     ctx->db_obj_off.as<uint32_t>(), ctx->n_objs, ctx->db_pts.as<float>(), d_counts, d_in_radius, d_matches, d_xyz);
  TOD_HIP(hipGetLastError());
  return TODHIP_OK;
}

int radius_args(const todhip_ctx* ctx, uint32_t nq, uint32_t radius, uint32_t mpq) {
  if (nq == 0 || radius == 0 || mpq == 0 || mpq > kMaxPerQuery) return TODHIP_EINVAL;
  if (ctx->total_rows == 0) return TODHIP_ENODB;
  if (ctx->desc_bytes != 32) return TODHIP_EINVAL;          // a float DB has no Hamming radius
  return TODHIP_OK;
}

// stream null: the context's
int merge_radius_shards(todhip_ctx* ctx, hipStream_t stream, const void* d_keys_all, uint32_t n_shards, uint32_t nq, uint32_t mpq,
                        void* d_counts, void* d_matches, void* d_xyz, void* d_in_radius) {
  if (!ctx || !d_keys_all || !d_counts || !d_matches || !d_xyz) return TODHIP_EINVAL;
  if (n_shards == 0 || n_shards > kMaxMergeShards) return TODHIP_EINVAL;
  int rc = radius_args(ctx, nq, 1u, mpq);                   // (the radius has done its work in the shards)
  if (rc != TODHIP_OK) return rc;
  return radius_merge(ctx, stream, reinterpret_cast<const uint64_t*>(d_keys_all), n_shards, nq, mpq, reinterpret_cast<uint32_t*>(d_counts),
                      reinterpret_cast<todhip_dmatch*>(d_matches), reinterpret_cast<float*>(d_xyz), reinterpret_cast<uint32_t*>(d_in_radius));
}

}  // namespace

extern "C" int todhip_match_radius_device(todhip_ctx* ctx, const void* d_q_desc, uint32_t nq, uint32_t radius, uint32_t max_per_query,
                                          void* d_counts, void* d_matches, void* d_matches_xyz, void* d_in_radius) {
  if (!ctx || !d_q_desc || !d_counts || !d_matches || !d_matches_xyz) return TODHIP_EINVAL;
  int rc = radius_args(ctx, nq, radius, max_per_query);
  if (rc != TODHIP_OK) return rc;
  rc = radius_search(ctx, d_q_desc, nq, radius, max_per_query, reinterpret_cast<uint32_t*>(d_counts),
                     reinterpret_cast<todhip_dmatch*>(d_matches), reinterpret_cast<float*>(d_matches_xyz),
                     reinterpret_cast<uint32_t*>(d_in_radius));
  if (rc == TODHIP_OK) { ctx->counters.last_nq = nq; ctx->counters.last_k = max_per_query; }
  return rc;
}

extern "C" int todhip_match_radius_shard_device(todhip_ctx* ctx, const void* d_q_desc, uint32_t nq, uint32_t radius, uint32_t max_per_query,
                                                void* d_keys) {
  if (!ctx || !d_q_desc || !d_keys) return TODHIP_EINVAL;
  int rc = radius_args(ctx, nq, radius, max_per_query);
  if (rc != TODHIP_OK) return rc;
  rc = radius_shard_keys(ctx, d_q_desc, nq, radius, max_per_query, reinterpret_cast<uint64_t*>(d_keys));
  if (rc == TODHIP_OK) { ctx->counters.last_nq = nq; ctx->counters.last_k = max_per_query; }
  return rc;
}

extern "C" int todhip_merge_radius_shards_device_on(todhip_ctx* ctx, void* hip_stream, const void* d_keys_all, uint32_t n_shards, uint32_t nq,
                                                    uint32_t max_per_query, void* d_counts, void* d_matches, void* d_matches_xyz,
                                                    void* d_in_radius) {
  if (!ctx || !hip_stream) return TODHIP_EINVAL;
  return merge_radius_shards(ctx, reinterpret_cast<hipStream_t>(hip_stream), d_keys_all, n_shards, nq, max_per_query, d_counts, d_matches,
                             d_matches_xyz, d_in_radius);
}

extern "C" int todhip_merge_radius_shards_device(todhip_ctx* ctx, const void* d_keys_all, uint32_t n_shards, uint32_t nq, uint32_t max_per_query,
                                                 void* d_counts, void* d_matches, void* d_matches_xyz, void* d_in_radius) {
  return merge_radius_shards(ctx, nullptr, d_keys_all, n_shards, nq, max_per_query, d_counts, d_matches, d_matches_xyz, d_in_radius);
}

extern "C" int todhip_match_radius(todhip_ctx* ctx, const uint8_t* q_desc, uint32_t nq, uint32_t radius, uint32_t max_per_query,
                                   uint32_t* row_ptr, todhip_dmatch* matches, float* matches_xyz, uint32_t* n_matches, uint32_t* in_radius) {
  if (!ctx || !q_desc || !row_ptr || !matches || !matches_xyz || !n_matches) return TODHIP_EINVAL;
  int rc = radius_args(ctx, nq, radius, max_per_query);
  if (rc != TODHIP_OK) return rc;
  TOD_HIP(hipSetDevice(ctx->device));
  RadiusWs* ws = tod_ws<RadiusWs>(ctx);
  const size_t nm = (size_t)nq * max_per_query;
  TOD_HIP(ctx->m_q.reserve((size_t)nq * 32u));
  TOD_HIP(ws->counts.reserve((size_t)nq * sizeof(uint32_t)));
  TOD_HIP(ws->in_radius.reserve((size_t)nq * sizeof(uint32_t)));
  // the emit kernel writes the kept matches straight into pinned host memory, as todhip_match's finalize does; the two count
  // arrays are read by kernels and come over with one copy each
  TOD_HIP(ctx->h_stage.reserve(2u * (size_t)nq * sizeof(uint32_t) + nm * sizeof(todhip_dmatch) + nm * 3 * sizeof(float)));
  uint32_t* h_counts = ctx->h_stage.as<uint32_t>();
  uint32_t* h_in = h_counts + nq;
  todhip_dmatch* h_m = reinterpret_cast<todhip_dmatch*>(h_in + nq);
  float* h_xyz = reinterpret_cast<float*>(h_m + nm);
  TOD_HIP(hipMemcpyAsync(ctx->m_q.p, q_desc, (size_t)nq * 32u, hipMemcpyHostToDevice, ctx->stream));
  rc = radius_search(ctx, ctx->m_q.p, nq, radius, max_per_query, ws->counts.as<uint32_t>(), h_m, h_xyz, ws->in_radius.as<uint32_t>());
  if (rc != TODHIP_OK) return rc;
  TOD_HIP(hipMemcpyAsync(h_counts, ws->counts.p, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  TOD_HIP(hipMemcpyAsync(h_in, ws->in_radius.p, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
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
