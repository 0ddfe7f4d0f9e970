// todhip_match_l2_radius[_device]: the true L2 radius search over a float DB -- every row whose distance is not > radius, counted
// exactly, the nearest max_per_query of them in the order (d2, row). Included by l2.hip behind the k-NN call's kernels: the query
// preparation (l2_prepare.h), the DB pass (l2_gemm_kernel<2, 4>) and its candidate sink (l2_gemm.h), d2_exact, the slot copy, the
// overflow conditions and the match writer (l2_refine.h) are that call's, unchanged. Definition: include/todhip.h; DESIGN 6l.
//
// The k-NN call filters with a threshold that comes from a seed (A_k + 2 eps); this one filters with a threshold that comes from the
// radius, so it needs ONE pass over the DB and no seed GEMM:
//   LT  l2_radius_threshold_kernel   thr(q) from the radius, |q|^2 and eps(q)               one thread per query
//   L2G l2_gemm_kernel<2, 4>         candidates = { r : score(q, r) <= thr(q) }             l2_gemm.h's, as l2_keys launches it
//   LR  l2_radius_refine_kernel      exact d2 of the candidates, the cut, the count, a sort one workgroup per query
//   LS  l2_radius_scan_kernel        the same answer from every DB row in order             one workgroup per FLAGGED query
//   LE  l2_radius_emit_kernel        key -> match and 3D point                              one thread per output slot
//
// Why no row of R(q) is lost (the filter may only admit too much; LR decides with the defining arithmetic):
//   r in R(q)  <=>  NOT (sqrtf(d2) > radius)  <=>  sqrtf(d2) <= radius            (d2 is never NaN for finite descriptors; a d2
//                                                                                  that overflowed to +Inf is outside every radius)
//   sqrtf is correctly rounded, so its result is >= sqrt(d2) / (1 + 2^-24):       sqrt(d2) <= radius (1 + 2^-24), and
//       d2 <= radius^2 (1 + 2^-24)^2 < radius^2 (1 + 2^-22) <= r2_up              r2_up = radius^2 (1 + 2^-21), formed in binary64
//                                                                                  (its own rounding, 2^-52, is far inside the slack)
//   the filter's bound (l2_bound.h: eps(q) = 2^-6 (1 + 2^-6) |q| Rmax + 2^-14 (|q| + Rmax)^2, the bf16 rounding of every component by
//   up to 2^-8 of its magnitude and every f32 rounding included), |score + |q|^2 - d2| <= eps(q) with |q|^2 the exact norm, gives for
//   such a row
//       score <= d2 - |q|^2 + eps(q) <= r2_up - |q|^2 + eps(q)
//   thr(q) = r2_up - |q|^2 + 2 eps(q), rounded UP to binary32. |q|^2 is summed here in binary64 from the f32 query (relative error
//   below 2^-45; the f32 value the prepare kernel leaves behind is a shuffle-tree sum with a rounding of its own and is not used).
//   The second eps is the band pass 2 of the k-NN call uses too: it covers the f32 rounding inside eps(q) itself (|q| and Rmax
//   come from f32 norms, relative error ~2^-21 of eps) and the binary64 roundings above, each many orders below eps(q).
//   A looser threshold costs candidates, never rows. (This one-sided use needs a single eps; the second one is slack. It is what kept
//   this search exact while eps was half of what bf16 rounding can do -- 2^-7 for 2^-6, the one-sided error reached 1.9 of it --
//   and tests/test_l2_numerics_gpu.py::test_the_radius_search_on_the_triple pins it.)
// Padding DB rows carry the norm 3e38 and a zero bf16 image, so their score is 3e38. A threshold at or beyond kThrMax = 1e38 is not
// used: such a query (a radius whose square leaves the range in which scores separate real rows from padding) collects nothing in
// the DB pass and is FLAGGED, and LS answers it from the rows themselves -- exact whatever the radius, and no padding row is ever a
// candidate. Padding queries get -FLT_MAX like the k-NN call's.
//
// Flagged queries: thr beyond kThrMax, or the candidate lists overflowed under l2_rerank_kernel's two conditions. LS is exact under
// any number of equal distances and costs one read of the f32 DB per flagged query.
//
// Resources (gfx950, -O3; none of them uses scratch): DESIGN 6l.
#pragma once

namespace {

static_assert(kL2SortKeys >= kListCap, "LR sorts every candidate of a query that did not overflow");
constexpr float kThrMax = 1.0e38f;                        // below the padding rows' score (3e38)

// LT. force[q] = 1: the query is answered by LS (see the head comment). D here and below: floats per row (kDim or kDimNarrow)
template <uint32_t D>
__global__ __launch_bounds__(256) void l2_radius_threshold_kernel(const float* __restrict__ q, uint32_t nq, uint32_t nq_pad, float radius,
                                                                  const float* __restrict__ eps, float* __restrict__ thr,
                                                                  uint32_t* __restrict__ force) {
  const uint32_t qi = blockIdx.x * 256u + threadIdx.x;
  if (qi >= nq_pad) return;
  if (qi >= nq) { thr[qi] = -FLT_MAX; return; }             // padding queries collect nothing
  double n2 = 0.0;
  for (uint32_t i = 0; i < D; i += 4) {
    const float4 v = *reinterpret_cast<const float4*>(q + (size_t)qi * D + i);
    n2 += (double)v.x * v.x; n2 += (double)v.y * v.y; n2 += (double)v.z * v.z; n2 += (double)v.w * v.w;
  }
  const double r2_up = (double)radius * (double)radius * (1.0 + 0x1p-21);
  const double t = r2_up - n2 + 2.0 * (double)eps[qi];
  const bool beyond = !(t < (double)kThrMax);               // also an eps that overflowed
  thr[qi] = beyond ? -FLT_MAX : __double2float_ru(t);
  force[qi] = beyond ? 1u : 0u;
}

// ascending bitonic sort of s[0 .. n2), n2 a power of two, by the 256 threads of the block; ends behind a barrier
__device__ __forceinline__ void l2_block_sort(uint64_t* s, uint32_t n2) {
  for (uint32_t k = 2; k <= n2; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = threadIdx.x; i < n2; i += 256u) {
        const uint32_t p = i ^ j;
        if (p > i) {
          const uint64_t a = s[i], b = s[p];
          if ((a > b) == ((i & k) == 0u)) { s[i] = b; s[p] = a; }
        }
      }
      __syncthreads();
    }
  }
}

// the key of (query, row) when the row is inside the radius, the fill value otherwise
template <uint32_t D>
__device__ __forceinline__ uint64_t l2_radius_key(const float* __restrict__ q, const float* __restrict__ db, uint32_t row, float radius) {
  const float d2 = d2_exact<D>(q, db + (size_t)row * D);
  return sqrtf(d2) > radius ? ~0ull : ((uint64_t)__float_as_uint(d2) << 32) | row;
}

// what LR and LS leave behind for a query whose sorted keys stand in s[]: the first min(count, mpq) keys, the two counts
__device__ __forceinline__ void l2_radius_store(const uint64_t* s, uint32_t count, uint32_t qi, uint32_t mpq, uint64_t* __restrict__ keys,
                                                uint32_t* __restrict__ counts, uint32_t* __restrict__ in_radius) {
  const uint32_t kept = min(count, mpq);
  for (uint32_t j = threadIdx.x; j < kept; j += 256u) keys[(size_t)qi * mpq + j] = s[j];
  if (threadIdx.x == 0) { counts[qi] = kept; if (in_radius) in_radius[qi] = count; }
}

// LR. One workgroup per query: its candidate rows (the lanes' slots, then the shared list) into LDS, flagged under
// l2_rerank_kernel's two conditions; otherwise the exact key of every candidate, the count of real keys, a sort, the cut. Keys are
// unique (a row is one lane's in one chunk), so the result does not depend on the order in which the slots were appended.
template <uint32_t D>
__global__ __launch_bounds__(256) void l2_radius_refine_kernel(const float* __restrict__ q, const float* __restrict__ db,
                                                               const uint32_t* __restrict__ slots, const uint32_t* __restrict__ slot_cnt,
                                                               uint32_t n_parts, const uint32_t* __restrict__ cand,
                                                               const uint32_t* __restrict__ cand_cnt, const uint32_t* __restrict__ force,
                                                               float radius, uint32_t mpq, uint64_t* __restrict__ keys,
                                                               uint32_t* __restrict__ counts, uint32_t* __restrict__ in_radius,
                                                               uint32_t* __restrict__ flagged) {
  __shared__ uint64_t s_keys[kL2SortKeys];
  __shared__ uint32_t s_rows[kListCap];
  __shared__ uint32_t s_total, s_count;
  const uint32_t qi = blockIdx.x, tid = threadIdx.x;
  if (force[qi] != 0u) { if (tid == 0) flagged[qi] = 1u; return; }
  if (tid == 0) { s_total = 0u; s_count = 0u; }
  __syncthreads();
  for (uint32_t p = tid; p < n_parts; p += 256u) {
    const uint32_t c = min(slot_cnt[(size_t)qi * n_parts + p], kSlot);
    if (c == 0u) continue;
    l2_copy_slot(slots + ((size_t)qi * n_parts + p) * kSlot, c, s_rows, atomicAdd(&s_total, c));
  }
  __syncthreads();
  const uint32_t in_slots = s_total, cnt = cand_cnt[qi];
  for (uint32_t c = tid; c < min(cnt, kCandCap); c += 256u)   // what did not fit a slot
    if (in_slots + c < kListCap) s_rows[in_slots + c] = cand[(size_t)qi * kCandCap + c];
  const uint32_t total = in_slots + cnt;
  if (l2_lists_overflowed(cnt, total)) { if (tid == 0) flagged[qi] = 1u; return; }   // redone by LS
  if (tid == 0) flagged[qi] = 0u;
  __syncthreads();
  uint32_t n2 = 1u;
  while (n2 < total) n2 <<= 1;
  uint32_t mine = 0;
  for (uint32_t c = tid; c < n2; c += 256u) {
    const uint64_t key = c < total ? l2_radius_key<D>(q + (size_t)qi * D, db, s_rows[c], radius) : ~0ull;
    s_keys[c] = key;
    mine += key != ~0ull ? 1u : 0u;
  }
  if (mine) atomicAdd(&s_count, mine);
  __syncthreads();
  l2_block_sort(s_keys, n2);
  l2_radius_store(s_keys, s_count, qi, mpq, keys, counts, in_radius);
}

// LS. One workgroup per flagged query streams every DB row through the defining distance, 256 rows a slice. s_keys[0 .. 1024): the
// best so far, ascending, ~0 padded; s_keys[1024 + fill): the in-radius keys of the slices since the last sort that are below
// `worst`, the max_per_query-th best at that sort (later keys at or above it can never be among the first max_per_query). A slice's
// keys are appended in row order (ballot, prefix over the four waves), so the buffer's content is the same on every run; when the
// next slice might not fit, all 2048 keys are sorted and the lower half is the new best.
template <uint32_t D>
__global__ __launch_bounds__(256) void l2_radius_scan_kernel(const float* __restrict__ q, const float* __restrict__ db, uint32_t n,
                                                             const uint32_t* __restrict__ flagged, float radius, uint32_t mpq,
                                                             uint64_t* __restrict__ keys, uint32_t* __restrict__ counts,
                                                             uint32_t* __restrict__ in_radius) {
  __shared__ uint64_t s_keys[kL2SortKeys];
  __shared__ uint32_t s_wave[2][4];
  __shared__ uint32_t s_count;
  const uint32_t qi = blockIdx.x, tid = threadIdx.x, l = tid & 63u, w = tid >> 6;
  if (flagged[qi] == 0u) return;
  for (uint32_t i = tid; i < kL2SortKeys; i += 256u) s_keys[i] = ~0ull;
  if (tid == 0) s_count = 0u;
  __syncthreads();
  uint64_t worst = ~0ull;
  uint32_t fill = 0, mine = 0, par = 0;
  for (uint32_t row0 = 0; row0 < n; row0 += 256u, par ^= 1u) {
    if (fill + 256u > kL2MaxPerQuery) {                     // (the tail behind fill is ~0 from the last sort)
      __syncthreads();                                      // the last slice's keys are in place
      l2_block_sort(s_keys, kL2SortKeys);
      for (uint32_t i = kL2MaxPerQuery + tid; i < kL2SortKeys; i += 256u) s_keys[i] = ~0ull;
      worst = s_keys[mpq - 1u];
      fill = 0u;
      __syncthreads();
    }
    const uint32_t row = row0 + tid;
    const uint64_t key = row < n ? l2_radius_key<D>(q + (size_t)qi * D, db, row, radius) : ~0ull;
    mine += key != ~0ull ? 1u : 0u;
    const bool take = key < worst;                          // ~0 is never below worst
    const unsigned long long b = __builtin_amdgcn_ballot_w64(take);
    if (l == 0) s_wave[par][w] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) { const uint32_t c = s_wave[par][i]; before += i < w ? c : 0u; all += c; }
    if (take) s_keys[kL2MaxPerQuery + fill + before + (uint32_t)__popcll(b & ((1ull << l) - 1ull))] = key;
    fill += all;
  }
  if (mine) atomicAdd(&s_count, mine);
  __syncthreads();
  l2_block_sort(s_keys, kL2SortKeys);
  l2_radius_store(s_keys, s_count, qi, mpq, keys, counts, in_radius);
}

// LE. l2_finalize_kernel's arithmetic without its cut: the cut has been made on the keys
__global__ __launch_bounds__(256) void l2_radius_emit_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ counts, uint32_t nq,
                                                             uint32_t mpq, const uint32_t* __restrict__ obj_off, uint32_t n_objs,
                                                             const float* __restrict__ pts, todhip_dmatch* __restrict__ matches,
                                                             float* __restrict__ xyz) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= (size_t)nq * mpq) return;
  const uint32_t qi = (uint32_t)(i / mpq), j = (uint32_t)(i % mpq);
  if (j >= counts[qi]) return;                              // slots behind counts[q] are not written
  const uint64_t key = keys[i];
  l2_write_match(key, l2_key_distance(key), qi, i, obj_off, n_objs, pts, matches, xyz);
}

}  // namespace
