// The float matcher over a sharded DB (todhip_match_l2_shard_device + todhip_merge_l2_shards_device[_on], and the radius pair
// todhip_match_l2_radius_shard_device + todhip_merge_l2_radius_shards_device[_on]; definition: include/todhip.h).
// Included by l2.hip behind the searches it continues: a rank runs the k-NN search (l2_keys) or the radius search (l2_radius_keys)
// on its shard exactly as the unsharded calls do, up to ws->keys, and sends those keys instead of resolving them; the owner of a
// query merges the ranks' lists and resolves them with the unsharded calls' own writer (l2_write_match, l2_refine.h).
//   SK l2_shard_keys_kernel          instead of l2_finalize_kernel: rows of the shard -> rows of the full DB, padding kept
//   SR l2_radius_shard_keys_kernel   instead of LE: the first counts[q] keys with rows of the full DB, padding, |R_s(q)| in the last slot
//   LK l2_merge_knn_kernel<K>        thread = query: the k smallest of n_shards x k keys, then l2_finalize_kernel's cut and writer
//   LM l2_merge_radius_kernel<STAGED>  match_radius.hip's radius_merge_kernel over float keys: the rank merge itself and the geometry
//                                    of its launch are shard_merge.h's, shared by the two; only the writer differs
// A key is (binary32 bits of d2) << 32 | row. d2 >= 0, so the order of the bits is the order of the values; a shard's rows are
// consecutive rows of the full DB, so (d2, row of the shard) sorts as (d2, row of the full DB) and adding shard_first to a key cannot
// carry (row + shard_first < 2^32). Why the merged result is the unsharded one whatever each shard's Rmax, eps and path: every shard
// call ends in the EXACT keys of its rows (pass 3, the exact scan, LR or LS: the defining d2 in the defining order), the filter
// before it only decides how they are found. The union of exact per-shard answers is searched with integer comparisons alone.
// The row width (128 or 64 floats) is the context's: the searches these kernels continue pick their instantiations from
// ctx->desc_bytes (l2_kernels, l2.hip), and nothing here looks inside a row -- a key is a key at either width.
#pragma once

#include "shard_merge.h"

namespace {

// SK. thread = slot of the nq x k keys a shard sends. keys null: a shard without rows sends padding only. Every slot is written.
__global__ __launch_bounds__(256) void l2_shard_keys_kernel(const uint64_t* __restrict__ keys, size_t n_slots, uint32_t first_row,
                                                            uint64_t* __restrict__ out) {
  const size_t slot = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (slot >= n_slots) return;
  const uint64_t key = keys ? keys[slot] : ~0ull;
  out[slot] = key == ~0ull ? key : key + first_row;         // (row + first_row < 2^32: no carry into the distance)
}

// SR. thread = slot of the nq x (max_per_query + 1) keys a shard sends; keys: [nq][max_per_query] as LR / LS leave them, the first
// counts[q] of a row valid. in_radius null: a shard without rows (keys and counts are not read). Every slot is written.
__global__ __launch_bounds__(256) void l2_radius_shard_keys_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ counts,
                                                                   const uint32_t* __restrict__ in_radius, uint32_t nq, uint32_t mpq,
                                                                   uint32_t first_row, uint64_t* __restrict__ out) {
  const size_t slot = (size_t)blockIdx.x * 256u + threadIdx.x;
  const uint32_t qi = (uint32_t)(slot / (mpq + 1u)), j = (uint32_t)(slot % (mpq + 1u));
  if (qi >= nq) return;
  uint64_t v = ~0ull;
  if (j == mpq) v = in_radius ? in_radius[qi] : 0u;
  else if (in_radius && j < counts[qi]) v = keys[(size_t)qi * mpq + j] + first_row;
  out[slot] = v;
}

// a key of the k-NN form stands: it is a row, and its distance is not beyond the radius (l2_finalize_kernel's two tests)
__device__ __forceinline__ bool l2_key_stands(uint64_t key, float radius) { return key != ~0ull && !(l2_key_distance(key) > radius); }

// LK, the k-NN merge: keys_all [n_shards][nq][K] as SK writes them. thread = query, as l2_finalize_kernel, which it continues: the K
// smallest of the n_shards x K keys through an insertion list in registers (keys_insert's network, K long; keys are unique over the
// shards and a padding key passes through it without moving anything), then l2_finalize_kernel's walk -- a match per key until the
// first that does not stand. K is a template argument so that a shard's K keys are loaded before any is looked at and the list's
// length is the call's k, not kTop. Neighbouring threads read neighbouring rows of a shard's keys.
// ratio > 0 (todhip_set_l2_ratio_test; K >= 2 then, the host refuses K == 1): the two smallest keys of the union are the query's two
// nearest rows of the full DB, and l2_finalize_kernel's test on them decides whether the walk starts at all.
template <int K>
__global__ __launch_bounds__(256) void l2_merge_knn_kernel(const uint64_t* __restrict__ keys_all, uint32_t n_shards, uint32_t nq, float radius,
                                                           float ratio, const uint32_t* __restrict__ obj_off, uint32_t n_objs,
                                                           const float* __restrict__ pts, uint32_t* __restrict__ counts,
                                                           todhip_dmatch* __restrict__ matches, float* __restrict__ xyz) {
  TOD_LATENCY_PRIO();   // latency-bound, as the Hamming merges
  const uint32_t qi = blockIdx.x * kMergeBlock + threadIdx.x;
  if (qi >= nq) return;
  uint64_t best[K];
#pragma unroll
  for (int j = 0; j < K; ++j) best[j] = ~0ull;
#pragma unroll 2
  for (uint32_t s = 0; s < n_shards; ++s) {
    const uint64_t* lst = keys_all + ((size_t)s * nq + qi) * K;
    uint64_t v[K];
#pragma unroll
    for (int j = 0; j < K; ++j) v[j] = lst[j];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      uint64_t key = v[j];
#pragma unroll
      for (int i = 0; i < K; ++i) { const uint64_t lo = key < best[i] ? key : best[i]; key = key < best[i] ? best[i] : key; best[i] = lo; }
    }
  }
  uint32_t kept = 0;
  bool open = true;
  if (K >= 2 && ratio > 0.f) open = tod::l2_ratio_keeps(best[0], best[K >= 2 ? 1 : 0], ratio);
#pragma unroll
  for (int j = 0; j < K; ++j) {
    open = open && l2_key_stands(best[j], radius);
    if (open) { l2_write_match(best[j], l2_key_distance(best[j]), qi, (size_t)qi * K + j, obj_off, n_objs, pts, matches, xyz); ++kept; }
  }
  counts[qi] = kept;
}

// LM, the radius merge: keys_all [n_shards][nq][max_per_query + 1] as SR writes them. radius_merge_kernel's rank merge
// (shard_rank_merge, shard_merge.h) with l2_write_match, the unsharded calls' writer, behind it.
template <bool STAGED>
__global__ __launch_bounds__(256) void l2_merge_radius_kernel(const uint64_t* __restrict__ keys_all, uint32_t n_shards, uint32_t nq, uint32_t mpq,
                                                              uint32_t qpb, const uint32_t* __restrict__ obj_off, uint32_t n_objs,
                                                              const float* __restrict__ pts, uint32_t* __restrict__ counts,
                                                              uint32_t* __restrict__ in_radius, todhip_dmatch* __restrict__ matches,
                                                              float* __restrict__ xyz) {
  TOD_LATENCY_PRIO();   // latency-bound, as radius_merge_kernel
  __shared__ uint64_t s_keys[STAGED ? kMergeLdsKeys : 1];
  shard_rank_merge<STAGED>(keys_all, n_shards, nq, mpq, qpb, counts, in_radius, s_keys, [&](uint64_t key, uint32_t qi, size_t at) {
    l2_write_match(key, l2_key_distance(key), qi, at, obj_off, n_objs, pts, matches, xyz);
  });
}

}  // namespace
