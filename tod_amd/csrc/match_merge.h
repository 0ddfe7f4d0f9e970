// Behind the DB pass of either engine: K4m, the per-tile lists merged into kMergeGroups lists of global keys (counting form and
// wave form); K4s, the k smallest of a shard's lists; K4f, the merge of the shards' lists with the radius truncation
// (DescriptorMatcher.cpp:212-220), the (imgIdx, trainIdx) lookup (:60-129) and the 3D gather (:231-244).
// Included by match.hip and match_wide.hip inside their anonymous namespaces, after match_keys.h.

// K4m: thread (query, group) merges the tiles t = group, group + G, ... ; keys become
// (distance << 32 | global_row), unique per row, so any merge order gives the same k smallest.
// Output layout [group][nq][K] == the [shard][nq][k] layout finalize_kernel consumes.
template <int K>
__global__ __launch_bounds__(kBlock) void merge_tiles_kernel(const uint32_t* __restrict__ part, uint32_t nq,
                                                             uint32_t nq_pad, uint32_t n_tiles,
                                                             uint32_t rows_per_tile, uint64_t first_global_row,
                                                             uint32_t n_groups, const uint8_t* __restrict__ stored,
                                                             uint32_t n_qw, uint64_t* __restrict__ keys,
                                                             const uint32_t* stat_src = nullptr, uint32_t* stat_dst = nullptr,
                                                             uint32_t stat_seq = 0) {
  TOD_LATENCY_PRIO();   // latency-bound: win issue arbitration against the VALU-saturating matcher
  const uint32_t qi = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t grp = blockIdx.y;
  if (stat_dst && qi == 0u && grp == 0u) {                  // the DB pass's half-block counters -> pinned host memory (K4xSplit, match_split.h)
    for (int i = 0; i < 4; ++i) stat_dst[i] = __hip_atomic_load(stat_src + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence_system();
    stat_dst[4] = stat_seq;
  }
  if (qi >= nq) return;
  uint64_t best[K];
#pragma unroll
  for (int j = 0; j < K; ++j) best[j] = ~0ull;
#pragma unroll 4
  for (uint32_t t = grp; t < n_tiles; t += n_groups) {
    if (stored[(size_t)t * n_qw + (qi >> 6)] != 0) continue;   // this tile kept nothing for the 64 queries around qi
    uint32_t pk[K];
#pragma unroll
    for (int j = 0; j < K; ++j) pk[j] = part[((size_t)t * K + j) * nq_pad + qi];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      uint64_t key = pk[j] == 0xFFFFFFFFu
                         ? ~0ull
                         : (((uint64_t)(pk[j] >> kLocalBits) << 32) |
                            (first_global_row + (uint64_t)t * rows_per_tile + (pk[j] & kLocalMask)));
#pragma unroll
      for (int s2 = 0; s2 < K; ++s2) {
        uint64_t lo = key < best[s2] ? key : best[s2];
        key = key < best[s2] ? best[s2] : key;
        best[s2] = lo;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < K; ++j) keys[((size_t)grp * nq + qi) * K + j] = best[j];
}

// K4m for a handful of queries (the <= 32-query regime: 8192 tiles, and merge_tiles_kernel's 16 queries x 16 groups = 256 threads walk
// 512 tiles each, 71 us behind a 217 us DB pass): one WAVE per (query, group), the group's tiles spread over its lanes, the lanes'
// lists merged by a butterfly of shuffles. Same keys, same output layout.
template <int K>
__global__ __launch_bounds__(kBlock) void merge_tiles_wave_kernel(const uint32_t* __restrict__ part, uint32_t nq, uint32_t nq_pad,
                                                                  uint32_t n_tiles, uint32_t rows_per_tile, uint64_t first_global_row,
                                                                  uint32_t n_groups, const uint8_t* __restrict__ stored, uint32_t n_qw,
                                                                  uint64_t* __restrict__ keys) {
  TOD_LATENCY_PRIO();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t qi = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6), grp = blockIdx.y;
  if (qi >= nq) return;                                     // (wave-uniform)
  uint64_t best[K];
#pragma unroll
  for (int j = 0; j < K; ++j) best[j] = ~0ull;
  for (uint32_t t = grp + n_groups * lane; t < n_tiles; t += n_groups * 64u) {
    if (stored[(size_t)t * n_qw + (qi >> 6)] != 0) continue;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const uint32_t pk = part[((size_t)t * K + j) * nq_pad + qi];
      uint64_t key = pk == 0xFFFFFFFFu ? ~0ull
                                       : (((uint64_t)(pk >> kLocalBits) << 32) | (first_global_row + (uint64_t)t * rows_per_tile + (pk & kLocalMask)));
#pragma unroll
      for (int s2 = 0; s2 < K; ++s2) { const uint64_t lo = key < best[s2] ? key : best[s2]; key = key < best[s2] ? best[s2] : key; best[s2] = lo; }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    uint64_t other[K];
#pragma unroll
    for (int j = 0; j < K; ++j) other[j] = __shfl_xor(best[j], off);
#pragma unroll
    for (int j = 0; j < K; ++j) {
      uint64_t key = other[j];
#pragma unroll
      for (int s2 = 0; s2 < K; ++s2) { const uint64_t lo = key < best[s2] ? key : best[s2]; key = key < best[s2] ? best[s2] : key; best[s2] = lo; }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < K; ++j) keys[((size_t)grp * nq + qi) * K + j] = best[j];
  }
}

// K4s: per query, the k smallest of n_lists ascending lists (layout [list][nq][k]) -> keys[nq][k].
__global__ __launch_bounds__(kBlock) void select_keys_kernel(const uint64_t* __restrict__ lists, uint32_t n_lists,
                                                             uint32_t nq, uint32_t k, uint64_t* __restrict__ keys) {
  TOD_LATENCY_PRIO();   // latency-bound: win issue arbitration against the VALU-saturating matcher
  const uint32_t qi = blockIdx.x * kBlock + threadIdx.x;
  if (qi >= nq) return;
  uint64_t last = 0;
  bool have_last = false;
  for (uint32_t j = 0; j < k; ++j) {
    const uint64_t nxt = next_key_over_lists(lists, n_lists, nq, qi, k, last, have_last);
    keys[(size_t)qi * k + j] = nxt;
    if (nxt == ~0ull) {
      for (uint32_t jj = j + 1; jj < k; ++jj) keys[(size_t)qi * k + jj] = ~0ull;
      break;
    }
    last = nxt;
    have_last = true;
  }
}

// K4f: merge the shard lists (layout [shard][nq][k]), truncate at the first distance > radius
// (DescriptorMatcher.cpp:212-220), map the global row to (imgIdx, trainIdx) through the object prefix
// sums (DB load order, :60-129) and gather the model point of every kept match (:231-244).
__global__ __launch_bounds__(kBlock) void finalize_kernel(const uint64_t* __restrict__ keys_all, uint32_t n_shards,
                                                          uint32_t nq, uint32_t k_in, uint32_t k_out, uint32_t radius, float ratio,
                                                          const uint32_t* __restrict__ obj_off, uint32_t n_objs,
                                                          const float* __restrict__ pts,
                                                          uint32_t* __restrict__ counts,
                                                          todhip_dmatch* __restrict__ matches,
                                                          float* __restrict__ xyz) {
  TOD_LATENCY_PRIO();   // latency-bound: win issue arbitration against the VALU-saturating matcher
  const uint32_t qi = blockIdx.x * kBlock + threadIdx.x;
  if (qi >= nq) return;
  // the k_out (for the ratio test: at least 2) smallest keys over all lists (next_key_over_lists)
  uint64_t picked[9];
  const uint32_t want = ratio > 0.f ? max(k_out, 2u) : k_out;
  uint32_t n_picked = 0;
  uint64_t last = 0;
  bool have_last = false;
  for (uint32_t j = 0; j < want; ++j) {
    const uint64_t nxt = next_key_over_lists(keys_all, n_shards, nq, qi, k_in, last, have_last);
    if (nxt == ~0ull) break;
    last = nxt;
    have_last = true;
    picked[n_picked++] = nxt;
  }
  // Lowe's ratio test on the two nearest neighbours (the block the reference leaves empty, DescriptorMatcher.cpp:223-227;
  // definition: include/todhip.h, todhip_set_ratio_test): an ambiguous query keeps nothing
  if (ratio > 0.f && n_picked >= 2u && !((float)(uint32_t)(picked[0] >> 32) < ratio * (float)(uint32_t)(picked[1] >> 32))) n_picked = 0;
  uint32_t kept = 0;
  for (uint32_t j = 0; j < n_picked && j < k_out; ++j) {
    const uint32_t d = (uint32_t)(picked[j] >> 32);
    if ((float)d > (float)radius) break;                    // radius truncation, :212-220 (float vs unsigned compare)
    store_match(qi, d, (uint32_t)picked[j], (size_t)qi * k_out + kept, obj_off, n_objs, pts, matches, xyz);
    ++kept;
  }
  counts[qi] = kept;
}
