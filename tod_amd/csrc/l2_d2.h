// The defining distance of the float matcher (include/todhip.h): d2 = sum over i = 0..dim-1 in index order of (q[i] - r[i])^2, every
// operation in binary32, rounded once, no fused multiply-add (-ffp-contract=off). Stated once, in steps of four dimensions, for the
// two translation units that evaluate it: l2.hip (pass 3, the exact scans, the radius search) walks both rows through d2_exact,
// cross_check.hip's float kernel holds one row in registers and walks the other through d2_step4 -- the same operations in the same
// order. Device code only.
#pragma once
#include <cstdint>

namespace tod {
constexpr uint32_t kL2Dim = 128;   // floats per row (l2_plan.h's kDim)
constexpr uint32_t kL2DimNarrow = 64;   // ... of the narrower float DB (l2_plan.h's kDimNarrow): d2_exact<64>, the same loop body
}

// d2_exact's loop body for a caller that holds one of the rows in registers: four more dimensions onto a partial sum. (d2_exact does
// not call it: built from this function its additions come out with their operands swapped in l2.hip's kernels, which are to stay
// instruction for instruction what they were.)
__device__ __forceinline__ float d2_step4(float acc, const float4 a, const float4 b) {
  float t = a.x - b.x; acc = acc + t * t;
  t = a.y - b.y; acc = acc + t * t;
  t = a.z - b.z; acc = acc + t * t;
  t = a.w - b.w; acc = acc + t * t;
  return acc;
}

template <uint32_t D = tod::kL2Dim>
__device__ __forceinline__ float d2_exact(const float* __restrict__ q, const float* __restrict__ r) {
  float acc = 0.f;
  for (uint32_t i = 0; i < D; i += 4) {
    const float4 a = *reinterpret_cast<const float4*>(q + i), b = *reinterpret_cast<const float4*>(r + i);
    float t = a.x - b.x; acc = acc + t * t;
    t = a.y - b.y; acc = acc + t * t;
    t = a.z - b.z; acc = acc + t * t;
    t = a.w - b.w; acc = acc + t * t;
  }
  return acc;
}
