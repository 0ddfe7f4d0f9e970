// What stands around the float matcher's DB pass: the threshold from the partitions' lists, pass 3 (the exact re-rank of the
// candidates and the exact scan for queries whose lists overflowed), the key -> match step, and the device helpers the radius search
// (l2_radius.h) shares with them. Included by l2.hip.
#pragma once

#include "l2_d2.h"
#include "l2_filters.h"

namespace {

// per query (one wave): k-th smallest score over the partitions' lists; scores at or above the seed were never
// recorded, so fewer than k entries mean A_k == seed. out = A_k + margin * eps
__global__ __launch_bounds__(256) void l2_threshold_kernel(const float* __restrict__ part, uint32_t n_parts, uint32_t nq,
                                                           uint32_t nq_pad, uint32_t k, const float* __restrict__ seed,
                                                           const float* __restrict__ eps, float margin, float* __restrict__ out) {
  const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6), l = threadIdx.x & 63u;
  if (q >= nq_pad) return;
  if (q >= nq) { if (l == 0) out[q] = -FLT_MAX; return; }   // padding queries collect nothing
  float best[kTop];
#pragma unroll
  for (uint32_t j = 0; j < kTop; ++j) best[j] = FLT_MAX;
  for (uint32_t p = l; p < n_parts; p += 64u) {
    const float* src = part + ((size_t)p * nq_pad + q) * kTop;
    for (uint32_t i = 0; i < kTop; ++i) {
      float v = src[i];
      if (v >= best[kTop - 1]) break;                       // lists are ascending
#pragma unroll
      for (uint32_t j = 0; j < kTop; ++j) { const float lo = fminf(best[j], v); v = fmaxf(best[j], v); best[j] = lo; }
    }
  }
  // k rounds of wave-min over the lanes' heads (values may repeat: pop one lane per round)
  float ak = FLT_MAX;
  for (uint32_t j = 0; j < k; ++j) {
    float v = best[0];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off));
    ak = v;
    const unsigned long long owners = __builtin_amdgcn_ballot_w64(best[0] == v);
    if (v != FLT_MAX && l == (uint32_t)__ffsll((long long)owners) - 1u) {
#pragma unroll
      for (uint32_t i = 0; i + 1 < kTop; ++i) best[i] = best[i + 1];
      best[kTop - 1] = FLT_MAX;
    }
  }
  if (seed) ak = fminf(ak, seed[q]);
  if (l == 0) out[q] = ak + margin * eps[q];
}

// (the defining distance, d2_exact: l2_d2.h)
static_assert(kDim == tod::kL2Dim, "l2_d2.h states the distance over kDim dimensions");
static_assert(kDimNarrow == tod::kL2DimNarrow, "... and over kDimNarrow dimensions");

__device__ __forceinline__ void keys_insert(uint64_t (&best)[kTop], uint64_t key) {
#pragma unroll
  for (uint32_t j = 0; j < kTop; ++j) { const uint64_t lo = key < best[j] ? key : best[j]; key = key < best[j] ? best[j] : key; best[j] = lo; }
}

// the k smallest keys of the wave's lanes' ascending lists -> out[0..k) (lane 0 writes)
__device__ __forceinline__ void wave_select(uint64_t (&best)[kTop], uint32_t k, uint64_t* out) {
  const uint32_t l = threadIdx.x & 63u;
  for (uint32_t j = 0; j < k; ++j) {
    uint64_t v = best[0];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint64_t o = ((uint64_t)__shfl_xor((uint32_t)(v >> 32), off) << 32) | __shfl_xor((uint32_t)v, off);
      v = o < v ? o : v;
    }
    if (l == 0) out[j] = v;
    if (best[0] == v && v != ~0ull) {                        // keys are unique: exactly one lane pops
#pragma unroll
      for (uint32_t i = 0; i + 1 < kTop; ++i) best[i] = best[i + 1];
      best[kTop - 1] = ~0ull;
    }
  }
}

// the first c rows of a partition's private slot (CandSink, l2_gemm.h) -> dst[at ..), as far as a list of kListCap goes
__device__ __forceinline__ void l2_copy_slot(const uint32_t* __restrict__ slot, uint32_t c, uint32_t* dst, uint32_t at) {
  const uint4* src = reinterpret_cast<const uint4*>(slot);
  const uint4 lo = src[0], hi = src[1];
  const uint32_t rows[kSlot] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
  for (uint32_t j = 0; j < kSlot; ++j) if (j < c && at + j < kListCap) dst[at + j] = rows[j];
}

// a query's candidates did not all fit (cnt: appended to its shared list, total: those and the slots'): the exact scan answers it
__device__ __forceinline__ bool l2_lists_overflowed(uint32_t cnt, uint32_t total) { return cnt > kCandCap || total > kListCap; }

__device__ __forceinline__ float l2_key_distance(uint64_t key) { return sqrtf(__uint_as_float((uint32_t)(key >> 32))); }

// key -> output slot `at` of query qi: object lookup (DescriptorMatcher.cpp:60-129 load order), 3D gather (:231-244)
__device__ __forceinline__ void l2_write_match(uint64_t key, float dist, uint32_t qi, size_t at, const uint32_t* __restrict__ obj_off,
                                               uint32_t n_objs, const float* __restrict__ pts, todhip_dmatch* __restrict__ matches,
                                               float* __restrict__ xyz) {
  const uint32_t row = (uint32_t)key;
  const uint32_t lo = object_of_row(obj_off, n_objs, row);
  todhip_dmatch m;
  m.queryIdx = (int)qi; m.trainIdx = (int)(row - obj_off[lo]); m.imgIdx = (int)lo; m.distance = dist;
  matches[at] = m;
  float* o = xyz + at * 3;
  o[0] = pts[(size_t)row * 3 + 0]; o[1] = pts[(size_t)row * 3 + 1]; o[2] = pts[(size_t)row * 3 + 2];
}

// pass 3: one wave per query. keys[q][k] = (f32 bits of d2) << 32 | row, ascending, ~0 padded. D: floats per row (kDim or kDimNarrow)
template <uint32_t D>
__global__ __launch_bounds__(256) void l2_rerank_kernel(const float* __restrict__ q, uint32_t nq, const float* __restrict__ db,
                                                        const uint32_t* __restrict__ slots, const uint32_t* __restrict__ slot_cnt,
                                                        uint32_t n_parts, const uint32_t* __restrict__ cand,
                                                        const uint32_t* __restrict__ cand_cnt, uint32_t k, uint64_t* __restrict__ keys,
                                                        uint32_t* __restrict__ overflow) {
  const uint32_t qi = blockIdx.x * 4u + (threadIdx.x >> 6), l = threadIdx.x & 63u;
  if (qi >= nq) return;
  const uint32_t cnt = cand_cnt[qi], w = threadIdx.x >> 6;
  // the query's candidate rows, gathered into one list in LDS first (the slots of 64 partitions at a time: counts, a wave
  // prefix sum, 32 bytes of rows per lane), so that the exact distances below are spread evenly over the lanes
  __shared__ uint32_t s_rows[4][kListCap];
  uint32_t total = 0;
  for (uint32_t p0 = 0; p0 < n_parts; p0 += 64u) {
    const uint32_t p = p0 + l;
    const uint32_t c = p < n_parts ? min(slot_cnt[(size_t)qi * n_parts + p], kSlot) : 0u;
    uint32_t incl = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const uint32_t t = __shfl_up(incl, off); if (l >= (uint32_t)off) incl += t; }
    if (c) l2_copy_slot(slots + ((size_t)qi * n_parts + p) * kSlot, c, s_rows[w], total + incl - c);
    total += __shfl(incl, 63);
  }
  for (uint32_t c = l; c < min(cnt, kCandCap); c += 64u)    // what did not fit a slot
    if (total + c < kListCap) s_rows[w][total + c] = cand[(size_t)qi * kCandCap + c];
  total += cnt;
  if (l2_lists_overflowed(cnt, total)) { if (l == 0) overflow[qi] = 1u; return; }   // redone by l2_exact_scan_kernel
  if (l == 0) overflow[qi] = 0u;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  uint64_t best[kTop];
#pragma unroll
  for (uint32_t j = 0; j < kTop; ++j) best[j] = ~0ull;
  for (uint32_t c = l; c < total; c += 64u) {
    const uint32_t row = s_rows[w][c];
    const float d2 = d2_exact<D>(q + (size_t)qi * D, db + (size_t)row * D);
    keys_insert(best, ((uint64_t)__float_as_uint(d2) << 32) | row);
  }
  wave_select(best, k, keys + (size_t)qi * k);
}

// fallback for queries whose candidate list overflowed (and the test hook's exact GPU reference): one block per
// query scans every DB row with the defining distance
template <uint32_t D>
__global__ __launch_bounds__(256) void l2_exact_scan_kernel(const float* __restrict__ q, uint32_t nq, const float* __restrict__ db,
                                                            uint32_t n, uint32_t k, const uint32_t* __restrict__ only_flagged,
                                                            uint64_t* __restrict__ keys) {
  __shared__ uint64_t s_keys[4][kTop];
  const uint32_t qi = blockIdx.x, tid = threadIdx.x, l = tid & 63u, w = tid >> 6;
  if (qi >= nq || (only_flagged && only_flagged[qi] == 0u)) return;
  uint64_t best[kTop];
#pragma unroll
  for (uint32_t j = 0; j < kTop; ++j) best[j] = ~0ull;
  for (uint32_t row = tid; row < n; row += 256u) {
    const float d2 = d2_exact<D>(q + (size_t)qi * D, db + (size_t)row * D);
    keys_insert(best, ((uint64_t)__float_as_uint(d2) << 32) | row);
  }
  wave_select(best, kTop, s_keys[w]);
  __syncthreads();
  if (w == 0) {
#pragma unroll
    for (uint32_t j = 0; j < kTop; ++j) best[j] = ~0ull;
    if (l < 4u * kTop) keys_insert(best, s_keys[l / kTop][l % kTop]);
    wave_select(best, k, keys + (size_t)qi * k);
  }
}

// ratio test (todhip_set_l2_ratio_test; ratio 0: off), radius cut (DescriptorMatcher.cpp:212-220 shape), object lookup (:60-129 load
// order), 3D gather (:231-244). keys: [nq][k_in]; the outputs have stride k_out <= k_in (k_in > k_out only for the ratio test with
// k == 1, which needs the second nearest row: todhip_match's k_in / k_out). While the test is on k_in >= 2 (the host sees to it).
__global__ __launch_bounds__(256) void l2_finalize_kernel(const uint64_t* __restrict__ keys, uint32_t nq, uint32_t k_in, uint32_t k_out,
                                                          float radius, float ratio, const uint32_t* __restrict__ obj_off, uint32_t n_objs,
                                                          const float* __restrict__ pts, uint32_t* __restrict__ counts,
                                                          todhip_dmatch* __restrict__ matches, float* __restrict__ xyz) {
  const uint32_t qi = blockIdx.x * 256u + threadIdx.x;
  if (qi >= nq) return;
  const uint64_t* lst = keys + (size_t)qi * k_in;
  uint32_t kept = 0;
  if (!(ratio > 0.f) || tod::l2_ratio_keeps(lst[0], lst[1], ratio)) {
    for (uint32_t j = 0; j < k_out; ++j) {
      const uint64_t key = lst[j];
      if (key == ~0ull) break;
      const float dist = l2_key_distance(key);
      if (dist > radius) break;
      l2_write_match(key, dist, qi, (size_t)qi * k_out + kept, obj_off, n_objs, pts, matches, xyz);
      ++kept;
    }
  }
  counts[qi] = kept;
}

}  // namespace
