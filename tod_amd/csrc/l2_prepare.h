// The float matcher's bf16 images: the DB's at load time (A-fragment order, row norms, Rmax) and the queries' in every call (bf16
// scaled by -2, |q|^2, eps, zeroed shared candidate counters). Included by l2.hip. The rounding and eps are l2_bound.h's.
#pragma once
#include "l2_bound.h"

namespace {

// one wave per row: bf16 image (scaled by `scale`, a power of two) and |row|^2; rows >= n are padding
// frag != 0 (the DB image): a 32-row tile is stored in MFMA A-fragment order -- 8 segments (k-steps s) of 64 lanes x 16 bytes,
// lane (h = l >> 5, r = l & 31) of segment s holding A[row r][k = 16 s + 8 h + j], j = 0..7 -- so that one wave-load of a
// segment is 1 KB contiguous AND already the register image v_mfma_f32_32x32x16_bf16 wants: no LDS staging, no swizzle
// query side (rmax2_bits != nullptr): eps(q) from |q|^2 and Rmax^2 is written too, and the query's shared candidate counter is zeroed
// (two launches less per call)
__global__ __launch_bounds__(256) void l2_prepare_kernel(const float* __restrict__ src, uint32_t n, uint32_t n_pad, float scale,
                                                         uint16_t* __restrict__ dst, float* __restrict__ norm2,
                                                         uint32_t* __restrict__ max_norm2_bits, int frag,
                                                         const uint32_t* __restrict__ rmax2_bits = nullptr, float* __restrict__ eps = nullptr,
                                                         uint32_t* __restrict__ zero_cnt = nullptr) {
  const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6), l = threadIdx.x & 63u;
  if (row >= n_pad) return;
  float a = 0.f, b = 0.f;
  if (row < n) { a = src[(size_t)row * kDim + 2u * l]; b = src[(size_t)row * kDim + 2u * l + 1u]; }
  const uint32_t k0 = 2u * l;                               // this lane's two dimensions k0, k0 + 1
  const size_t at = frag ? ((size_t)(row >> 5) * (kTileRows * kDim) + (k0 >> 4) * 512u + (((k0 >> 3) & 1u) * 32u + (row & 31u)) * 8u + (k0 & 7u)) / 2u
                         : (size_t)row * (kDim / 2u) + l;
  reinterpret_cast<uint32_t*>(dst)[at] =
      (uint32_t)tod::l2_bf16_rne(a * scale) | ((uint32_t)tod::l2_bf16_rne(b * scale) << 16);
  float s = a * a + b * b;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (l == 0) {
    const float n2 = row < n ? s : 3.0e38f;                 // a padding row can never be a candidate
    norm2[row] = n2;
    if (row < n && max_norm2_bits) atomicMax(max_norm2_bits, __float_as_uint(s));
    if (rmax2_bits) {
      eps[row] = tod::l2_eps(n2, __uint_as_float(*rmax2_bits));
      zero_cnt[row] = 0u;
    }
  }
}

// The same for rows of kDimNarrow = 64 floats (a sibling, so that the kernel above stays what it is): one wave per row, a lane takes
// ONE dimension k = l. frag != 0: a 32-row tile is 4 segments (k-steps) of 64 lanes x 16 bytes, 4 KB, in the order stated above.
// |row|^2: lane l holds v[l]^2, then s += shfl_xor(s, 32 ... 1) -- one product and six shuffle steps, no addition before the tree
// (tests/l2_dim64_bound_host_test.cpp sums in this order).
__global__ __launch_bounds__(256) void l2_prepare_narrow_kernel(const float* __restrict__ src, uint32_t n, uint32_t n_pad, float scale,
                                                                uint16_t* __restrict__ dst, float* __restrict__ norm2,
                                                                uint32_t* __restrict__ max_norm2_bits, int frag,
                                                                const uint32_t* __restrict__ rmax2_bits = nullptr,
                                                                float* __restrict__ eps = nullptr, uint32_t* __restrict__ zero_cnt = nullptr) {
  const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6), l = threadIdx.x & 63u;
  if (row >= n_pad) return;
  const float a = row < n ? src[(size_t)row * kDimNarrow + l] : 0.f;
  const size_t at = frag ? (size_t)(row >> 5) * (kTileRows * kDimNarrow) + (l >> 4) * 512u + (((l >> 3) & 1u) * 32u + (row & 31u)) * 8u + (l & 7u)
                         : (size_t)row * kDimNarrow + l;
  dst[at] = tod::l2_bf16_rne(a * scale);
  float s = a * a;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (l == 0) {
    const float n2 = row < n ? s : 3.0e38f;                 // a padding row can never be a candidate
    norm2[row] = n2;
    if (row < n && max_norm2_bits) atomicMax(max_norm2_bits, __float_as_uint(s));
    if (rmax2_bits) {
      eps[row] = tod::l2_eps(n2, __uint_as_float(*rmax2_bits));
      zero_cnt[row] = 0u;
    }
  }
}

}  // namespace
