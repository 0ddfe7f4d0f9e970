// One row of the orientation patch from four-pixel words (host and device, plain C++, no HIP include: included by orb_stages.h for
// patch_moments, tested stand-alone by tests/orb_diet_host_test.cpp against the byte loop it replaced).
//
// A row of the radius-15 disc is the pixels u = -d .. d around the keypoint. Its 32 bytes from u = -15 are eight words; byte i of
// the row has u = i - 15, so with the byte dot products sum(px) and sum(i * px) over the bytes inside +-d the row's part of m10 is
// sum(i * px) - 15 * sum(px): the same integer as the byte loop's, since every partial sum stays below 31 * 30 * 255 < 2^31.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define TOD_ORB_HD __host__ __device__ __forceinline__
#else
#define TOD_ORB_HD inline
#endif

namespace tod_orb {

constexpr int kMomentWords = 8;                 // words of a row: u = -15 .. 16, the last byte is never inside the disc

// sum over the four bytes of a * b, added to c
TOD_ORB_HD uint32_t dot4_u8(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_udot4(a, b, c, false);
#else
  for (int i = 0; i < 4; ++i) c += ((a >> (8 * i)) & 0xFFu) * ((b >> (8 * i)) & 0xFFu);
  return c;
#endif
}

// 0xFF in every byte i of word k whose row index 4 k + i lies inside the row's half-width d (bit j of `inside`: 15 - d <= j <= 15 + d)
TOD_ORB_HD uint32_t moment_inside(int d) { return ((2u << (15 + d)) - 1u) & ~((1u << (15 - d)) - 1u); }
TOD_ORB_HD uint32_t moment_byte_mask(uint32_t inside, int k) {
  const uint32_t ones = (((inside >> (4 * k)) & 0xFu) * 0x00204081u) & 0x01010101u;   // bit i of the nibble in byte i
  return (ones << 8) - ones;                                                          // (* 0xFF without a full-width multiply)
}

// row: the 32 bytes from u = -15 (any alignment; all of them are read, those beyond +-d count as zero), d <= 15.
// rs = sum of the pixels with |u| <= d, m10 = sum of u * pixel over the same
TOD_ORB_HD void row_moments(const uint8_t* row, int d, int& rs, int& m10) {
  const uint32_t inside = moment_inside(d);
  uint32_t sum = 0u, weighted = 0u;
  for (int k = 0; k < kMomentWords; ++k) {                   // (eight fixed rounds: the compiler unrolls them)
    uint32_t px;
    __builtin_memcpy(&px, row + 4 * k, 4);
    px &= moment_byte_mask(inside, k);
    sum = dot4_u8(px, 0x01010101u, sum);
    weighted = dot4_u8(px, 0x03020100u + 0x04040404u * (uint32_t)k, weighted);
  }
  rs = (int)sum;
  m10 = (int)weighted - 15 * (int)sum;
}

}  // namespace tod_orb
