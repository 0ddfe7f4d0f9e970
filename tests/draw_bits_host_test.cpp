// Stand-alone host test of tod_amd/csrc/verify_draw_bits.h (built and run by tests/test_draw_bits_cpu.py with the host sanitizers):
// the n-th set bit over WL words, the bit count and the removal of a bit against a bit-by-bit walk.
// Prints "<selections checked> <removals checked>".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "verify_draw_bits.h"

using tod_bits::u64;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {                                  // xorshift64*
  g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
  return g_state * 0x2545F4914F6CDD1Dull;
}

static long g_selections = 0, g_removals = 0;

template <int WL>
static bool check(const u64 (&w)[WL], const char* what) {
  std::vector<uint32_t> bits;                                 // ascending positions of the set bits
  for (int j = 0; j < WL; ++j)
    for (uint32_t i = 0; i < 64u; ++i)
      if ((w[j] >> i) & 1ull) bits.push_back(64u * (uint32_t)j + i);
  if (tod_bits::count_bits(w) != bits.size()) { std::printf("%s: count %u, expected %zu\n", what, tod_bits::count_bits(w), bits.size()); return false; }
  for (uint32_t n = 0; n < bits.size(); ++n) {                // every n < popcount
    const uint32_t got = tod_bits::nth_set_bit(w, n);
    ++g_selections;
    if (got != bits[n]) { std::printf("%s (WL %d): bit %u is at %u, expected %u\n", what, WL, n, got, bits[n]); return false; }
  }
  // removing the bits one by one, middle outwards, keeps the others where they were (and a position beyond the words clears nothing)
  u64 v[WL];
  for (int j = 0; j < WL; ++j) v[j] = w[j];
  tod_bits::clear_bit(v, 64u * (uint32_t)WL + 3u);
  for (int j = 0; j < WL; ++j) if (v[j] != w[j]) { std::printf("%s: a position beyond the words cleared a bit\n", what); return false; }
  std::vector<uint32_t> left = bits;
  while (!left.empty()) {
    const size_t k = left.size() / 2;
    tod_bits::clear_bit(v, left[k]);
    left.erase(left.begin() + (long)k);
    ++g_removals;
    if (tod_bits::count_bits(v) != left.size()) { std::printf("%s: count after a removal\n", what); return false; }
    if (!left.empty()) {
      const uint32_t probe = (uint32_t)(left.size() / 2);
      if (tod_bits::nth_set_bit(v, probe) != left[probe]) { std::printf("%s: selection after a removal\n", what); return false; }
      if (tod_bits::nth_set_bit(v, 0) != left.front() || tod_bits::nth_set_bit(v, (uint32_t)left.size() - 1u) != left.back()) {
        std::printf("%s: first / last after a removal\n", what); return false;
      }
    }
  }
  return true;
}

template <int WL>
static bool run() {
  const u64 kinds[] = {0ull, ~0ull, 1ull, 1ull << 63, 0ull /* random */};
  u64 w[WL];
  // every word empty, full, bit 0 only, bit 63 only or random: all combinations at WL = 2, 4000 random combinations at WL = 8
  const int n_combo = WL == 2 ? 25 : 4000;
  for (int combo = 0; combo < n_combo; ++combo) {
    for (int j = 0; j < WL; ++j) {
      const int kind = WL == 2 ? (j == 0 ? combo % 5 : combo / 5) : (int)(next_u64() % 5u);
      w[j] = kind == 4 ? (next_u64() & next_u64() & (next_u64() | next_u64())) : kinds[kind];
    }
    if (!check(w, "kinds")) return false;
  }
  // the target in the first word, in the last word, and in a word whose predecessors are all empty
  for (int j = 0; j < WL; ++j) w[j] = 0ull;
  w[0] = next_u64();
  if (!check(w, "first word only")) return false;
  w[0] = 0ull; w[WL - 1] = next_u64();
  if (!check(w, "last word only")) return false;
  for (int t = 0; t < WL; ++t) {
    for (int j = 0; j < WL; ++j) w[j] = j < t ? 0ull : next_u64();
    if (!check(w, "empty predecessors")) return false;
    for (int j = 0; j < WL; ++j) w[j] = j == t ? (1ull << (7 * t)) : 0ull;
    if (!check(w, "single bit")) return false;
  }
  for (int j = 0; j < WL; ++j) w[j] = ~0ull;
  if (!check(w, "all full")) return false;
  for (int j = 0; j < WL; ++j) w[j] = (j & 1) ? ~0ull : 0ull;      // empty words between full ones
  if (!check(w, "alternating")) return false;
  for (int j = 0; j < WL; ++j) w[j] = 0ull;
  if (!check(w, "all empty")) return false;
  for (int r = 0; r < 300; ++r) {
    for (int j = 0; j < WL; ++j) w[j] = next_u64();
    if (!check(w, "random")) return false;
  }
  return true;
}

int main() {
  // the word search alone, every n of a few words
  const u64 words[] = {~0ull, 1ull, 1ull << 63, 0x8000000000000001ull, 0xAAAAAAAAAAAAAAAAull, 0x00000000FFFFFFFFull, 0xFFFFFFFF00000000ull};
  for (u64 x : words) {
    uint32_t n = 0;
    for (uint32_t i = 0; i < 64u; ++i)
      if ((x >> i) & 1ull) { if (tod_bits::nth_set_bit64(x, n) != i) { std::printf("nth_set_bit64\n"); return 1; } ++n; }
  }
  if (!run<2>() || !run<8>()) return 1;
  std::printf("%ld %ld\n", g_selections, g_removals);
  return 0;
}
