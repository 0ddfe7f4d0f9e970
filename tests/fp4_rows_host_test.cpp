// The fp4 copy of the DB rows (tod_amd/csrc/fp4_rows.h) against its definition, bit by bit, on the host: bit b of row r is nibble
// (b % 32) / 4 of dword (b % 4) of the 16 bytes at fragment (step r / 32, MFMA index (b / 32) % 4, lane 32 (b / 128) + r % 32), and
// that nibble is the E2M1 value +1.0 (0x2) for a 0 bit and -1.0 (0xA) for a 1 bit. Every (row, bit) of 32, 33, 63 and 4113 rows,
// the rows of the last step past the end included (they come from the slack behind the rows). Buffers are sized exactly, so that
// the sanitizers this is built with see any access beyond a whole step. Prints the number of nibbles checked.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "fp4_rows.h"

int main() {
  unsigned long long checked = 0;
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  for (uint32_t n_rows : {32u, 33u, 63u, 4113u}) {
    const uint32_t steps = fp4_rows_steps(n_rows), padded = steps * 32u;
    if (fp4_rows_bytes(n_rows) != (size_t)steps * 4096u || steps != (n_rows + 31u) / 32u) { printf("size of %u rows\n", n_rows); return 1; }
    std::vector<uint32_t> rows((size_t)padded * 8u), out(fp4_rows_bytes(n_rows) / 4u, 0u);
    for (uint32_t& w : rows) { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; w = (uint32_t)(rng >> 16); }
    fp4_rows_expand_host(rows.data(), n_rows, out.data());
    std::vector<uint8_t> seen(out.size() * 8u, 0);                    // every nibble of the copy belongs to exactly one (row, bit)
    for (uint32_t r = 0; r < padded; ++r)
      for (uint32_t b = 0; b < 256u; ++b) {
        const uint32_t bit = (rows[(size_t)r * 8u + b / 32u] >> (b % 32u)) & 1u;
        const uint32_t s = r / 32u, m = (b / 32u) % 4u, l = 32u * (b / 128u) + r % 32u, j = b % 4u, i = (b % 32u) / 4u;
        const size_t off = fp4_rows_offset(s, m, l);
        if (off % 16u != 0 || off + 16u > out.size() * 4u) { printf("offset of step %u, index %u, lane %u\n", s, m, l); return 1; }
        if (fp4_rows_src_row(s, l) != r || fp4_rows_src_word(m, l) != b / 32u) { printf("source of step %u, index %u, lane %u\n", s, m, l); return 1; }
        const uint32_t nib = (out[off / 4u + j] >> (4u * i)) & 0xFu;
        if (nib != (0x2u | (bit << 3))) { printf("%u rows: row %u bit %u: nibble %x\n", n_rows, r, b, nib); return 1; }
        if (seen[(off / 4u + j) * 8u + i]++) { printf("%u rows: row %u bit %u: nibble used twice\n", n_rows, r, b); return 1; }
        ++checked;
      }
    for (uint8_t v : seen) if (v != 1) { printf("%u rows: a nibble of the copy belongs to no bit\n", n_rows); return 1; }
  }
  printf("%llu\n", checked);
  return 0;
}
