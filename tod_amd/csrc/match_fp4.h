// The matrix-core block primitives of the exact 256-bit Hamming searches, and no kernel: what hamming_topk_mfma, hamming_topk_mfma_q32
// (match_mfma.h) and radius_collect_mfma (match_radius.hip) share; at the end, their 512-bit forms for hamming_topk_wide (match_wide.hip).
// Included inside the anonymous namespace after match_keys.h.
// With every descriptor bit b written as the MX-fp4 (E2M1) value 1 - 2b, the dot product of two descriptors is 256 - 2 * hamming:
// products are +-1, the f32 accumulator holds integers <= 256, so the result is EXACT. v_mfma_f32_32x32x64_f8f6f4 (fp4 x fp4, unit
// scales) takes 64 bit positions of 32 DB rows x 32 queries per issue: 4 MFMAs = 1024 complete distances in 128 matrix-pipe cycles
// (8 pairs per clock and SIMD; K4's VALU form peaks at 1, or ~2 when its elimination fires) and the rate does not depend on the data.
// One WAVE = (DB tile, 32 QT queries). The query fragments stay in registers (16 VGPRs per 32 queries); every lane loads 16 packed
// bytes of one DB row per 32-row step (a wave load = 32 rows = 1 KB contiguous, served by L2: all query waves of a tile read the
// same lines), expands them to fp4 with 7 VALU ops per 32 bits, no LDS, no barrier. A and B use the same (lane, register, nibble)
// -> bit assignment, so the sum runs over matching bit positions whatever the hardware's internal k order is.
// THE LAYOUT (dtype independent): lane l loads the 16 bytes at word 4 (l >> 5) of row / query (l & 31) of its step / block; in the
// accumulator, lane = query column (l & 31) and register i = the step's row (i & 3) + 8 (i >> 2) + 4 (l >> 5)  (block_row,
// lane_row_base). A block is tested for "some lane's best of 16 reaches its threshold" (block_reaches), in the shadow of the next
// block's MFMAs, and only a block with a hit walks its registers.
typedef int mfma_i32x8 __attribute__((ext_vector_type(8)));
typedef float mfma_f32x16 __attribute__((ext_vector_type(16)));
// 32 descriptor bits -> 32 fp4 values (4 dwords): nibble i of out[j] = 0x2 | (bit (4 i + j) << 3)  (+1.0 / -1.0 in E2M1).
// The two constants live in registers (gfx9 VOP3 takes no literal), so each dword is one shift + one v_and_or_b32.
struct Fp4Consts { uint32_t sign, one; };
__device__ __forceinline__ Fp4Consts fp4_consts() {
  Fp4Consts k;
  asm volatile("s_mov_b32 %0, 0x88888888" : "=s"(k.sign));
  asm volatile("v_mov_b32 %0, 0x22222222" : "=v"(k.one));
  return k;
}
__device__ __forceinline__ mfma_i32x8 expand_word(uint32_t x, const Fp4Consts& k) {
  const int a = (int)(((x << 3) & k.sign) | k.one), b = (int)(((x << 2) & k.sign) | k.one),
            c = (int)(((x << 1) & k.sign) | k.one), d = (int)((x & k.sign) | k.one);
  return mfma_i32x8{a, b, c, d, 0, 0, 0, 0};
}
struct Fp4Row { mfma_i32x8 s[4]; };   // the lane's 128 bits of one row: 4 MFMA steps x 4 dwords (upper halves unused by fp4)
__device__ __forceinline__ void expand_row(const uint4& p, Fp4Row& f, const Fp4Consts& k) {
  f.s[0] = expand_word(p.x, k); f.s[1] = expand_word(p.y, k); f.s[2] = expand_word(p.z, k); f.s[3] = expand_word(p.w, k);
}
__device__ __forceinline__ float thr_of_limit(uint32_t limit) { return 256.f - 2.f * (float)limit; }   // dot > thr <=> d < limit

// The first SPLIT (2 or 3) of the block's 4 MFMAs, the rest waiting behind a test (mfma_block_test_part); and all 4: 256 bit
// positions of 32 DB rows (A) x 32 queries (B), in the layout above
template <int SPLIT>
__device__ __forceinline__ mfma_f32x16 dot_part0(const Fp4Row& a, const Fp4Row& b) {
  mfma_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < SPLIT; ++s) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a.s[s], b.s[s], acc, 4, 4, 0, 0, 0, 0);
  return acc;
}
__device__ __forceinline__ mfma_f32x16 dot_block(const Fp4Row& a, const Fp4Row& b) { return dot_part0<4>(a, b); }
// What fills the accumulator that stands for "no pending block yet": below every threshold (256 - 2 * 1023 at the least in the
// top-k kernels, -256 in the radius pass)
constexpr float kNoBlock = -4096.f;
// The step's row of register i (bits 0, 1 and 3), and the tile-local row base of this lane (h = lane >> 5) in a step: 32 step + 4 h
// leaves bits 0, 1, 3 and 4 free, so base | block_row(i) == base + block_row(i). The base is a macro: as a function it changes the
// top-k kernels' generated code (the register allocation of the masked steps), and the kernels are tuned to the code they have.
__device__ __forceinline__ constexpr uint32_t block_row(int i) { return (uint32_t)((i & 3) + 8 * (i >> 2)); }
#define lane_row_base(step, h) (32u * (step) + 4u * (h))

// Does this lane's best of the block's 16 dot products reach thr -- beat it (the top-k lists: d < limit), or, INCL, equal it as well
// (the radius pass: d <= radius)? IMAX: thr is >= 0 (radius < 128; the top-k thresholds only rise), so the 16-way maximum may be
// taken on the raw bits as integers -- among non-negative floats the order is the same, and a negative dot product can never reach
// a non-negative threshold -- which spares the float maximum's NaN-quieting moves.
// The integer maximum is a tree (5 independent max3, then 2 + 1): in this form the split-block kernel is bound by vector issue, not by
// the matrix pipe (tools/mfma_valu_overlap.hip: 2 MFMAs + chain + expansion 113 cycles per block and SIMD, + tree 103), and the
// tree's independent operations fill the issue slots a chain leaves to its own latency.
template <bool IMAX, bool INCL>
__device__ __forceinline__ bool block_reaches(const mfma_f32x16& acc, float thr) {
  if (IMAX) {
    int g[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) g[j] = max(max(__float_as_int(acc[3 * j]), __float_as_int(acc[3 * j + 1])), __float_as_int(acc[3 * j + 2]));
    const int m = max(max(max(g[0], g[1]), g[2]), max(max(g[3], g[4]), __float_as_int(acc[15])));
    return INCL ? m >= __float_as_int(thr) : m > __float_as_int(thr);
  }
  float m = fmaxf(fmaxf(acc[0], acc[1]), acc[2]);
#pragma unroll
  for (int i = 3; i < 15; i += 2) m = fmaxf(fmaxf(m, acc[i]), acc[i + 1]);
  m = fmaxf(m, acc[15]);
  return INCL ? m >= thr : m > thr;
}

// One resident query fragment: this lane's 16 bytes of query qi = the block's first + (lane & 31). Queries at or beyond nq repeat
// the last one (padding: never stored). A block at a time: K4x sets up a block's list between two loads, and its code follows that.
__device__ __forceinline__ void load_query_block(const uint32_t* __restrict__ q, uint32_t qi, uint32_t nq, uint32_t h, Fp4Row& qb,
                                                 const Fp4Consts& kc) {
  const uint4 p = *reinterpret_cast<const uint4*>(q + (size_t)(qi < nq ? qi : nq - 1u) * kWords + 4u * h);
  expand_row(p, qb, kc);
}

// This lane's 16 packed bytes of row (row0 + 32 step + (lane & 31)), steps beyond the tile's last repeating the last. No per-lane
// clamp: the DB's last step may reach up to 31 rows past its end -- into the slack todhip_db_load leaves behind the descriptors
// (kDbSlackBytes, also behind a view), rows that the walks mask, never use -- and the address stays a wave-uniform base plus a
// constant lane offset (no vector instruction per load: the kernels are bound by those)
struct StepLoader {
  const uint32_t* db;
  uint32_t row0, n_steps, lane_off;                          // lane_off: bytes from the step's first row
  __device__ __forceinline__ StepLoader(const uint32_t* d, uint32_t r0, uint32_t n, uint32_t c, uint32_t h)
      : db(d), row0(r0), n_steps(n), lane_off((c * kWords + 4u * h) * 4u) {}
  __device__ __forceinline__ uint32_t first_row(uint32_t step) const { return row0 + 32u * min(step, n_steps - 1u); }   // wave-uniform
  __device__ __forceinline__ uint4 operator()(uint32_t step) const {
    const char* base = reinterpret_cast<const char*>(db) + (size_t)first_row(step) * (kWords * 4u);
    return *reinterpret_cast<const uint4*>(base + lane_off);
  }
};

// ---- 512-bit rows (match_wide.hip: BRISK, FREAK, 64-byte descriptors). A row is two 256-bit halves in the layout above: lane l
// loads the 16 bytes at word 4 (l >> 5) of the row and the 16 bytes at word 8 + 4 (l >> 5). 8 MFMAs per 32 x 32 block give
// dot = 512 - 2 d, still exact in f32; the accumulator layout, block_row / lane_row_base, block_reaches and kNoBlock are unchanged
// (the least threshold of a 10-bit limit is 512 - 2 * 1023).
constexpr int kWordsWide = 16;
struct Fp4Row2 { Fp4Row lo, hi; };
__device__ __forceinline__ float thr_of_limit_wide(uint32_t limit) { return 512.f - 2.f * (float)limit; }   // dot > thr <=> d < limit
// dot_block on top of what acc already holds
__device__ __forceinline__ mfma_f32x16 dot_block_acc(mfma_f32x16 acc, const Fp4Row& a, const Fp4Row& b) {
#pragma unroll
  for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a.s[s], b.s[s], acc, 4, 4, 0, 0, 0, 0);
  return acc;
}
__device__ __forceinline__ mfma_f32x16 dot_block_wide(const Fp4Row2& a, const Fp4Row2& b) { return dot_block_acc(dot_block(a.lo, b.lo), a.hi, b.hi); }
__device__ __forceinline__ void load_query_block_wide(const uint32_t* __restrict__ q, uint32_t qi, uint32_t nq, uint32_t h, Fp4Row2& qb,
                                                      const Fp4Consts& kc) {
  const uint32_t* row = q + (size_t)(qi < nq ? qi : nq - 1u) * kWordsWide + 4u * h;
  expand_row(*reinterpret_cast<const uint4*>(row), qb.lo, kc);
  expand_row(*reinterpret_cast<const uint4*>(row + 8), qb.hi, kc);
}
// StepLoader for 64-byte rows: the same wave-uniform base plus constant lane offset, the same reliance on the slack behind the rows
// (31 rows of 64 bytes: ctx.h holds kDbSlackBytes to that)
struct StepLoaderWide {
  const uint32_t* db;
  uint32_t row0, n_steps, lane_off;
  __device__ __forceinline__ StepLoaderWide(const uint32_t* d, uint32_t r0, uint32_t n, uint32_t c, uint32_t h)
      : db(d), row0(r0), n_steps(n), lane_off((c * kWordsWide + 4u * h) * 4u) {}
  __device__ __forceinline__ void operator()(uint32_t step, uint4& lo, uint4& hi) const {
    const char* base = reinterpret_cast<const char*>(db) + (size_t)(row0 + 32u * min(step, n_steps - 1u)) * (kWordsWide * 4u) + lane_off;
    lo = *reinterpret_cast<const uint4*>(base);
    hi = *reinterpret_cast<const uint4*>(base + 32);
  }
};
