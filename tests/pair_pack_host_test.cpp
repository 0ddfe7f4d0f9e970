// The packing of two split blocks into one f32 accumulator (tod_amd/csrc/match_pair_pack.h) against its definition, on the host: for
// every cut in 1 .. 64 and every even dA, dB in [-128, 128], magic + dA + 2048 dB accumulated in `float` in the order the four MFMAs
// add (block t's two halves, then block t + 1's, each dot product split as lopsidedly as 64 positions allow) must be the exact
// integer, in [2^23, 2^24), its mantissa the integer minus 2^23; bit 9 must be set exactly when dA > thrp and bit 20 exactly when
// dB > thrp, no other bit of the mask and neither bit 10 nor bit 21 ever; unpack must return dA and dB; the magic itself ("no pending
// pair") has both flags clear. Prints the number of cases checked.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "match_pair_pack.h"

static uint32_t bits_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

int main() {
  unsigned long long checked = 0;
  for (unsigned cut = PairPack::kMinCut; cut <= PairPack::kMaxCut; ++cut) {
    const int thrp = PairPack::thrp(cut), bias = PairPack::bias(cut);
    if (thrp != 256 - 2 * (int)cut - 128 || thrp < 0 || thrp > 126) { printf("thrp of cut %u\n", cut); return 1; }
    const float magic = PairPack::magic(cut);
    if ((long long)magic != (long long)PairPack::magic_int(cut)) { printf("magic of cut %u is not an integer in f32\n", cut); return 1; }
    // "no pending pair": the magic itself has both flags clear
    if (bits_of(magic) & PairPack::kFlagMask) { printf("magic of cut %u has a flag set\n", cut); return 1; }
    for (int dA = -128; dA <= 128; dA += 2)
      for (int dB = -128; dB <= 128; dB += 2) {
        // two MFMAs per block: split each dot product into two even halves, the first as lopsided as 64 positions allow
        const int a0 = dA > 0 ? (dA > 64 ? 64 : dA) : (dA < -64 ? -64 : dA), a1 = dA - a0;
        const int b0 = dB > 0 ? (dB > 64 ? 64 : dB) : (dB < -64 ? -64 : dB), b1 = dB - b0;
        volatile float acc = magic;
        acc = acc + (float)a0; acc = acc + (float)a1;
        acc = acc + 2048.f * (float)b0; acc = acc + 2048.f * (float)b1;
        const long long want = (long long)PairPack::magic_int(cut) + dA + 2048ll * dB;
        const float got = acc;
        if ((long long)got != want || got < 8388608.f || got >= 16777216.f) { printf("cut %u dA %d dB %d: %.1f, not %lld\n", cut, dA, dB, (double)got, want); return 1; }
        const uint32_t u = bits_of(got);
        if ((u & 0x7FFFFFu) != (uint32_t)(want - 8388608ll)) { printf("cut %u dA %d dB %d: the mantissa is not the integer\n", cut, dA, dB); return 1; }
        if (((u & PairPack::kFlagA) != 0u) != (dA > thrp)) { printf("cut %u dA %d dB %d: flag A\n", cut, dA, dB); return 1; }
        if (((u & PairPack::kFlagB) != 0u) != (dB > thrp)) { printf("cut %u dA %d dB %d: flag B\n", cut, dA, dB); return 1; }
        if (((u & PairPack::kFlagMask) & ~((dA > thrp ? PairPack::kFlagA : 0u) | (dB > thrp ? PairPack::kFlagB : 0u))) != 0u) { printf("cut %u dA %d dB %d: a flag of the mask beyond the two\n", cut, dA, dB); return 1; }
        if (u & ((1u << 10) | (1u << 21))) { printf("cut %u dA %d dB %d: a field overflowed\n", cut, dA, dB); return 1; }
        if (PairPack::unpack(u, 0, bias) != dA || PairPack::unpack(u, 1, bias) != dB) { printf("cut %u dA %d dB %d: unpack\n", cut, dA, dB); return 1; }
        ++checked;
      }
  }
  if (PairPack::kScaleOne != 127 || PairPack::kScaleField != 138 || PairPack::kFlagMask != 0x00100200u) { printf("constants\n"); return 1; }
  printf("%llu\n", checked);
  return 0;
}
