// The compass pre-test of FAST-9/16 on four neighbouring positions of a row at once (host and device, plain C++, no HIP include:
// included by orb_fast.h, tested stand-alone by tests/orb_diet_host_test.cpp against the per-position statement of the same test).
//
// A 9-arc above the threshold holds two cyclically adjacent compass points (ring positions 0, 4, 8, 12) that are both brighter
// than p + 20 or both darker than p - 20, so the four adjacent-pair terms of a polarity are (b0 | b8) & (b4 | b12). The bytes of a
// window are split into the even and the odd ones, each pair in the two 16-bit fields of a word as the blur's pair sums are
// (orb_pyramid.h), and a field of ring + (0x8000 - 21) - p has bit 15 set exactly where ring - p > 20 (darker: p and ring
// swapped). No field borrows from its neighbour or carries into it: 0x8000 - 21 - 255 > 0 and 0x8000 - 21 + 255 < 2^16.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define TOD_ORB_HD __host__ __device__ __forceinline__
#else
#define TOD_ORB_HD inline
#endif

namespace tod_orb {

constexpr int kFastThr = 20;
constexpr uint32_t kCompassMask = 0x00FF00FFu, kCompassBias = (0x8000u - (uint32_t)(kFastThr + 1)) * 0x00010001u;

// The test on one position, stated on the score's own terms: the pixel at c in an image of row pitch W, the same pixels and the
// same comparisons (d > kFastThr, -d > kFastThr) as fast_score_at's. compass4 gives this for each of its four positions.
TOD_ORB_HD bool fast_compass(const uint8_t* c, int W) {
  const int p = c[0];
  const int d0 = c[3 * W] - p, d4 = c[3] - p, d8 = c[-3 * W] - p, d12 = c[-3] - p;
  const bool b0 = d0 > kFastThr, b4 = d4 > kFastThr, b8 = d8 > kFastThr, b12 = d12 > kFastThr;
  const bool k0 = -d0 > kFastThr, k4 = -d4 > kFastThr, k8 = -d8 > kFastThr, k12 = -d12 > kFastThr;
  return (b0 && b4) || (b4 && b8) || (b8 && b12) || (b12 && b0) || (k0 && k4) || (k4 && k8) || (k8 && k12) || (k12 && k0);
}

// bytes shift .. shift + 3 of the eight bytes lo, hi (shift 0..3): a four-pixel window that starts inside an aligned word
TOD_ORB_HD uint32_t window4(uint32_t lo, uint32_t hi, int shift) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * shift)); }

// the even and the odd bytes of a word, each pair as two 16-bit fields
TOD_ORB_HD uint32_t even_bytes(uint32_t x) { return x & kCompassMask; }
TOD_ORB_HD uint32_t odd_bytes(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_perm(x, x, 0x0c030c01u);                  // bytes 1, zero, 3, zero in one instruction
#else
  return (x >> 8) & kCompassMask;
#endif
}
// the larger / the smaller of each 16-bit field
TOD_ORB_HD uint32_t max_pairs(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef unsigned short pair_t __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(pair_t, a), __builtin_bit_cast(pair_t, b)));
#else
  const uint32_t lo = (a & 0xFFFFu) > (b & 0xFFFFu) ? (a & 0xFFFFu) : (b & 0xFFFFu), hi = (a >> 16) > (b >> 16) ? (a >> 16) : (b >> 16);
  return lo | (hi << 16);
#endif
}
TOD_ORB_HD uint32_t min_pairs(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef unsigned short pair_t __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(pair_t, a), __builtin_bit_cast(pair_t, b)));
#else
  const uint32_t lo = (a & 0xFFFFu) < (b & 0xFFFFu) ? (a & 0xFFFFu) : (b & 0xFFFFu), hi = (a >> 16) < (b >> 16) ? (a >> 16) : (b >> 16);
  return lo | (hi << 16);
#endif
}

// bit 15 / 31: the position in that field passes the test; p, r0 .. r12: two positions' centre and compass pixels as 16-bit fields.
// b0 | b8 is the test of the brighter of ring pixels 0 and 8 (darker: of the darker one), so each polarity is two compares.
TOD_ORB_HD uint32_t compass_pairs(uint32_t p, uint32_t r0, uint32_t r4, uint32_t r8, uint32_t r12) {
  const uint32_t up = kCompassBias - p, dn = kCompassBias + p;       // ring + up: brighter; dn - ring: darker
  const uint32_t bright = (max_pairs(r0, r8) + up) & (max_pairs(r4, r12) + up);
  const uint32_t dark = (dn - min_pairs(r0, r8)) & (dn - min_pairs(r4, r12));
  return bright | dark;
}

// Bit i: position i of the four passes the compass test. p: the four centre pixels (position i in byte i); r0, r4, r8, r12: the
// pixels three rows below, three columns right, three rows above and three columns left of each (the score's ring positions).
TOD_ORB_HD uint32_t compass4(uint32_t p, uint32_t r0, uint32_t r4, uint32_t r8, uint32_t r12) {
  const uint32_t even = compass_pairs(even_bytes(p), even_bytes(r0), even_bytes(r4), even_bytes(r8), even_bytes(r12));
  const uint32_t odd = compass_pairs(odd_bytes(p), odd_bytes(r0), odd_bytes(r4), odd_bytes(r8), odd_bytes(r12));
  const uint32_t r = ((even >> 15) & 0x00010001u) | ((odd >> 14) & 0x00020002u);   // positions 0, 1 in bits 0, 1; 2, 3 in bits 16, 17
  return (r | (r >> 14)) & 0xFu;
}

}  // namespace tod_orb
