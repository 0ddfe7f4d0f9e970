// Two per-row device functions that more than one stage needs, free of any stage's constants. Included after ctx.h.
#pragma once

// Hamming distance of a 256-bit row, given as its two 16-byte halves, to the query words qw[8]
__device__ __forceinline__ uint32_t hamming256(const uint4& a, const uint4& b, const uint32_t (&qw)[8]) {
  return (uint32_t)(__popc(a.x ^ qw[0]) + __popc(a.y ^ qw[1]) + __popc(a.z ^ qw[2]) + __popc(a.w ^ qw[3]) +
                    __popc(b.x ^ qw[4]) + __popc(b.y ^ qw[5]) + __popc(b.z ^ qw[6]) + __popc(b.w ^ qw[7]));
}

// Hamming distance of a 512-bit row, given as its four 16-byte quarters, to the query words qw[16]
__device__ __forceinline__ uint32_t hamming512(const uint4& a, const uint4& b, const uint4& c, const uint4& d, const uint32_t (&qw)[16]) {
  return (uint32_t)(__popc(a.x ^ qw[0]) + __popc(a.y ^ qw[1]) + __popc(a.z ^ qw[2]) + __popc(a.w ^ qw[3]) +
                    __popc(b.x ^ qw[4]) + __popc(b.y ^ qw[5]) + __popc(b.z ^ qw[6]) + __popc(b.w ^ qw[7]) +
                    __popc(c.x ^ qw[8]) + __popc(c.y ^ qw[9]) + __popc(c.z ^ qw[10]) + __popc(c.w ^ qw[11]) +
                    __popc(d.x ^ qw[12]) + __popc(d.y ^ qw[13]) + __popc(d.z ^ qw[14]) + __popc(d.w ^ qw[15]));
}

// The last object whose first row is <= row (obj_off: the objects' prefix sums in DB load order, DescriptorMatcher.cpp:60-129)
__device__ __forceinline__ uint32_t object_of_row(const uint32_t* __restrict__ obj_off, uint32_t n_objs, uint32_t row) {
  uint32_t lo = 0, hi = n_objs;
  while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (obj_off[mid] <= row) lo = mid; else hi = mid; }
  return lo;
}
