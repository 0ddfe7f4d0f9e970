// Bitsets of a few 64-bit words held by ONE lane (host and device, plain C++, no HIP include: included by verify_draw.h for the
// lane-per-position draw table, tested stand-alone by tests/draw_bits_host_test.cpp against a bit-by-bit walk).
// Nothing here indexes the word array with a run-time value: every loop is unrolled over the compile-time word count and picks
// its word by compares, so the words stay in registers.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define TOD_BITS_HD __host__ __device__ __forceinline__
#define TOD_BITS_UNROLL _Pragma("unroll")
#else
#define TOD_BITS_HD inline
#define TOD_BITS_UNROLL
#endif

namespace tod_bits {

typedef unsigned long long u64;

TOD_BITS_HD uint32_t popc64(u64 w) { return (uint32_t)__builtin_popcountll(w); }

// position of the n-th set bit of w (ascending, n < popcount(w)): a binary search over the halves, six steps
TOD_BITS_HD uint32_t nth_set_bit64(u64 w, uint32_t n) {
  uint32_t pos = 0;
TOD_BITS_UNROLL
  for (uint32_t shift = 32; shift > 0; shift >>= 1) {
    const uint32_t cnt = popc64((w >> pos) & ((1ull << shift) - 1ull));
    if (n >= cnt) { n -= cnt; pos += shift; }
  }
  return pos;
}

// the same over WL words (bit 64 j + i = bit i of w[j]), n < the popcount of all of them: running popcounts pick the word -- the
// last one whose predecessors hold at most n set bits, so empty words in front of the target are passed over -- then the search
// inside it
template <int WL>
TOD_BITS_HD uint32_t nth_set_bit(const u64 (&w)[WL], uint32_t n) {
  if constexpr (WL == 2) {                                    // two words: one popcount, one branch
    const uint32_t c0 = popc64(w[0]);
    u64 word = w[0];
    uint32_t base = 0;
    if (n >= c0) { n -= c0; word = w[1]; base = 64u; }
    return base + nth_set_bit64(word, n);
  }
  u64 word = w[0];
  uint32_t base = 0, before = 0, run = 0;
TOD_BITS_UNROLL
  for (int j = 0; j + 1 < WL; ++j) {
    run += popc64(w[j]);
    if (n >= run) { word = w[j + 1]; base = 64u * (uint32_t)(j + 1); before = run; }
  }
  return base + nth_set_bit64(word, n - before);
}

template <int WL>
TOD_BITS_HD uint32_t count_bits(const u64 (&w)[WL]) {
  uint32_t c = 0;
TOD_BITS_UNROLL
  for (int j = 0; j < WL; ++j) c += popc64(w[j]);
  return c;
}

// clear bit v (v < 64 WL; a larger v clears nothing)
template <int WL>
TOD_BITS_HD void clear_bit(u64 (&w)[WL], uint32_t v) {
  if constexpr (WL == 2) {                                    // two words: the pair of registers is never an indexed array
    if (v < 64u) w[0] &= ~(1ull << v); else if (v < 128u) w[1] &= ~(1ull << (v - 64u));
    return;
  }
  // every word is rewritten, with a mask that a compare selects: a conditional store per word is what the compiler folds back
  // into one store at a run-time index (and the array into scratch)
  const u64 bit = 1ull << (v & 63u);
TOD_BITS_UNROLL
  for (int j = 0; j < WL; ++j) w[j] &= ~((v >> 6) == (uint32_t)j ? bit : 0ull);
}

}  // namespace tod_bits
