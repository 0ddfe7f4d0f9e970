// The resident fp4 copy of the 32-byte DB rows (hamming_topk_fp4rows, match_fp4rows.h): where a fragment lives and what it holds, as
// plain C++ for host and device. The copy is what expand_word (match_fp4.h) makes of the packed rows, stored once, in the order the
// DB pass reads it: fragment-major, so each of a wave's four loads per 32-row step is 1 KB contiguous at a wave-uniform base plus
// constants. No reference lines: the reference has no such search. Included by ctx.h and by tests/fp4_rows_host_test.cpp.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define TOD_FP4_HD __host__ __device__
#else
#define TOD_FP4_HD
#endif

constexpr uint32_t kFp4StepBytes = 4096;   // one 32-row step: 4 MFMA operands x 64 lanes x 16 bytes
constexpr uint32_t kFp4FragBytes = 1024;   // one MFMA operand of one step: a wave's load

// Byte offset of the 16 bytes of lane l for MFMA index m (0..3) of 32-row step s
TOD_FP4_HD inline size_t fp4_rows_offset(uint32_t s, uint32_t m, uint32_t l) { return (((size_t)s * 4u + m) * 64u + l) * 16u; }
// What they are made of: row s * 32 + (l & 31), its 32-bit word 4 (l >> 5) + m  (match_fp4.h, THE LAYOUT)
TOD_FP4_HD inline uint32_t fp4_rows_src_row(uint32_t s, uint32_t l) { return s * 32u + (l & 31u); }
TOD_FP4_HD inline uint32_t fp4_rows_src_word(uint32_t m, uint32_t l) { return 4u * (l >> 5) + m; }
// Steps and bytes of the copy of n_rows rows: whole steps (rows past the end are expanded from the slack behind the packed rows and
// masked by the pass, as they are today)
TOD_FP4_HD inline uint32_t fp4_rows_steps(uint32_t n_rows) { return (n_rows + 31u) / 32u; }
TOD_FP4_HD inline size_t fp4_rows_bytes(uint32_t n_rows) { return (size_t)fp4_rows_steps(n_rows) * kFp4StepBytes; }

// expand_word's bit assignment without its register constants: dword j (0..3) of the expansion of x. Nibble i = 0x2 | (bit (4 i + j)
// of x << 3), the E2M1 values +1.0 / -1.0. The device's expand_word stays the definition the kernels run; this is its host form, and
// tests/fp4_rows_host_test.cpp holds it to the sentence above bit by bit.
TOD_FP4_HD inline uint32_t fp4_expand_dword(uint32_t x, uint32_t j) { return ((x << (3u - j)) & 0x88888888u) | 0x22222222u; }

// Host form of expand_rows_fp4_kernel: the copy of n_rows packed rows (readable up to the end of their last whole step) into out
inline void fp4_rows_expand_host(const uint32_t* rows, uint32_t n_rows, uint32_t* out) {
  for (uint32_t s = 0; s < fp4_rows_steps(n_rows); ++s)
    for (uint32_t m = 0; m < 4u; ++m)
      for (uint32_t l = 0; l < 64u; ++l) {
        const uint32_t x = rows[(size_t)fp4_rows_src_row(s, l) * 8u + fp4_rows_src_word(m, l)];
        uint32_t* o = out + fp4_rows_offset(s, m, l) / 4u;
        for (uint32_t j = 0; j < 4u; ++j) o[j] = fp4_expand_dword(x, j);
      }
}
