// The device merge of per-shard radius answers, shared by match_radius.hip's radius_merge_kernel (Hamming keys) and l2_sharded.h's
// l2_merge_radius_kernel (float keys): the rank merge by binary search, and the geometry of its launch. A key is
// (distance << 32 | row of the full DB), a list is ascending with ~0 padding at its end, and keys are unique over the shards because
// the row is part of the key. The two kernels differ in how a key becomes a match (the writer they pass).
#pragma once
#include <cstdint>

namespace {

constexpr uint32_t kMergeBlock = 256;                       // threads of a merge workgroup
constexpr uint32_t kMergeLdsKeys = 4096;                    // 32 KB: the lists a workgroup searches in LDS
constexpr uint32_t kMaxMergeShards = 64;

// keys of an ascending list of n (padding ~0 at its end) that are below `key`
__device__ __forceinline__ uint32_t keys_below(const uint64_t* lst, uint32_t n, uint64_t key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (lst[mid] < key) lo = mid + 1u; else hi = mid;
  }
  return lo;
}

// The rank merge of one workgroup: keys_all [n_shards][nq][width + 1] -- per (shard, query) `width` ascending keys, ~0 padded, and the
// shard's count in the last slot. Element j of shard s stands at j + the keys below it in every other shard's list; the padding
// sorts last, so a search runs over all `width` slots. A list that was cut at `width` answers `width` for a key behind its cut; the
// position is then >= width, as the true one is. An element whose position is below `width` is one of the query's first `width`:
// write(key, query, output slot) puts it there. No sort, no atomics, each output slot has one writer. in_radius = the sum of the count
// slots (may be null), counts = min(in_radius, width).
// thread = (shard, slot) element of a query; E = n_shards * width elements per query. A workgroup takes qpb queries:
// floor(256 / E) while E <= 128 (width 5 on two shards: 25 queries), else one, its threads striding over the elements.
// STAGED: the workgroup's lists fit kMergeLdsKeys keys and are searched in LDS (s_keys); otherwise (up to 64 x 1024) in global memory.
template <bool STAGED, typename Write>
__device__ __forceinline__ void shard_rank_merge(const uint64_t* __restrict__ keys_all, uint32_t n_shards, uint32_t nq, uint32_t width,
                                                 uint32_t qpb, uint32_t* __restrict__ counts, uint32_t* __restrict__ in_radius,
                                                 uint64_t* s_keys, Write write) {
  const uint32_t tid = threadIdx.x, q0 = blockIdx.x * qpb;
  const uint32_t stride = width + 1u, elems = n_shards * width;
  const uint32_t n_here = min(qpb, nq - q0) * elems;        // elements of this workgroup's queries (q0 < nq by the grid)
  if (tid < qpb && q0 + tid < nq) {                         // the count slots
    uint64_t n = 0;
    for (uint32_t s = 0; s < n_shards; ++s) n += keys_all[((size_t)s * nq + q0 + tid) * stride + width];
    counts[q0 + tid] = n < width ? (uint32_t)n : width;
    if (in_radius) in_radius[q0 + tid] = (uint32_t)n;
  }
  if (STAGED) {                                             // image [query][shard][slot], n_here <= kMergeLdsKeys
    for (uint32_t i = tid; i < n_here; i += kMergeBlock) {
      const uint32_t ql = i / elems, e = i % elems, s = e / width, j = e % width;
      s_keys[i] = keys_all[((size_t)s * nq + q0 + ql) * stride + j];
    }
    __syncthreads();
  }
  for (uint32_t i = tid; i < n_here; i += kMergeBlock) {
    const uint32_t ql = i / elems, e = i % elems, s = e / width, j = e % width;
    const uint32_t qi = q0 + ql;
    const uint64_t key = STAGED ? s_keys[i] : keys_all[((size_t)s * nq + qi) * stride + j];
    if (key == ~0ull) continue;                             // padding
    uint32_t pos = j;
    for (uint32_t t = 0; t < n_shards && pos < width; ++t) {
      if (t == s) continue;
      if constexpr (STAGED) pos += keys_below(s_keys + ql * elems + t * width, width, key);
      else pos += keys_below(keys_all + ((size_t)t * nq + qi) * stride, width, key);
    }
    if (pos < width) write(key, qi, (size_t)qi * width + pos);
  }
}

// the launch of a rank merge: queries per workgroup, workgroups, and whether the lists are staged in LDS
struct ShardMergeGrid { uint32_t qpb, blocks; bool staged; };
inline ShardMergeGrid shard_merge_grid(uint32_t n_shards, uint32_t nq, uint32_t width) {
  const uint32_t elems = n_shards * width;                  // <= 64 * 1024
  const uint32_t qpb = elems <= kMergeBlock / 2 ? kMergeBlock / elems : 1u;
  return {qpb, (nq + qpb - 1u) / qpb, qpb * elems <= kMergeLdsKeys};
}

}  // namespace
