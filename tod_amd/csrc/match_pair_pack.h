// Two split blocks in one f32 accumulator: the one definition of the packing that hamming_topk_fp4rows' paired step uses
// (match_fp4rows.h), in plain C++ so that host code can check it (tests/pair_pack_host_test.cpp) and tools/mfma_valu_overlap.hip
// can price it. No includes: match.hip takes it inside its anonymous namespace.
// The first two MFMAs of a block (128 bit positions, products +-1) give an even integer d in [-128, 128]. Blocks t and t + 1 of a row
// step run their four MFMAs into ONE accumulator: those of block t + 1 in the block-scaled form of the instruction with an E8M0 scale
// of 2^kFieldBits on the rows, and the first MFMA takes the launch's magic as srcC:
//   acc = magic + dA + 2^kFieldBits dB,   magic = 1.5 * 2^23 + bias * (2^kFieldBits + 1),   bias = kFieldZero - (thrp + 1)
// with thrp = thr_of_limit(cut) - 128 = 128 - 2 cut, the part threshold of the launch's radius (0 <= thrp <= 126 wherever split 2 is
// allowed: 1 <= cut <= 64). Every partial sum is an integer in [2^23, 2^24), where an f32's unit in the last place is 1: the sum is
// exact and the mantissa bits ARE the integer minus 2^23. So field A = dA + bias sits at bit 0 and field B = dB + bias at bit
// kFieldBits, both in [257, 639]: neither borrows from nor carries into its neighbour, bit 9 of a field is set exactly when
// d + bias >= 512, that is d > thrp, and bit 10 never. "Does any row pair of either block reach the launch's threshold" is an OR over
// the 16 registers and one mask.
#pragma once

struct PairPack {
  static constexpr int kFieldBits = 11, kFieldZero = 512;
  static constexpr unsigned kFieldMask = (1u << kFieldBits) - 1u;
  static constexpr unsigned kFlagA = 1u << 9, kFlagB = kFlagA << kFieldBits, kFlagMask = kFlagA | kFlagB;   // 0x00100200
  static constexpr int kScaleOne = 127, kScaleField = 127 + kFieldBits;   // E8M0 bytes: 2^0 and 2^kFieldBits
  static constexpr unsigned kMinCut = 1u, kMaxCut = 64u;                  // where split 2 is allowed
  static constexpr int kMaxDot = 128;                                     // |d| <= 128: two MFMAs of 64 positions
  static constexpr float kMagicBase = 12582912.f;                         // 1.5 * 2^23
  static constexpr int thrp(unsigned cut) { return 128 - 2 * (int)cut; }
  static constexpr int bias(unsigned cut) { return kFieldZero - (thrp(cut) + 1); }
  static constexpr int magic_int(unsigned cut) { return 12582912 + bias(cut) * ((1 << kFieldBits) + 1); }
  static constexpr float magic(unsigned cut) { return kMagicBase + (float)(bias(cut) * ((1 << kFieldBits) + 1)); }
  // the dot product of field F (0: block t, 1: block t + 1) of a packed accumulator's bits
  static constexpr int unpack(unsigned bits, int field, int bias_of_cut) { return (int)((bits >> (field * kFieldBits)) & kFieldMask) - bias_of_cut; }
};
static_assert(PairPack::kFlagMask == 0x00100200u, "bit 9 of either field");
static_assert(PairPack::thrp(PairPack::kMaxCut) == 0 && PairPack::thrp(PairPack::kMinCut) == 126, "0 <= thrp <= 126");
static_assert(PairPack::bias(PairPack::kMinCut) - PairPack::kMaxDot >= 256 && PairPack::bias(PairPack::kMaxCut) + PairPack::kMaxDot < 640,
              "a field stays in [256, 640): bit 9 is the flag, bit 10 and the neighbour are never touched");
static_assert(PairPack::magic_int(PairPack::kMaxCut) + PairPack::kMaxDot * ((1 << PairPack::kFieldBits) + 1) < (1 << 24) &&
              PairPack::magic_int(PairPack::kMinCut) - PairPack::kMaxDot * ((1 << PairPack::kFieldBits) + 1) >= (1 << 23),
              "every partial sum is an integer in [2^23, 2^24): exact in f32");
