// The matrix-core block primitives of the exact Hamming searches, and no kernel: what hamming_topk_mfma, hamming_topk_mfma_q32
// (match_mfma.h), hamming_topk_fp4rows (match_fp4rows.h), radius_collect_mfma (match_radius.hip) and hamming_topk_wide
// (match_wide.hip) share; the top-k passes' list helpers (exchange_bounds, store_tile_lists); at the end, the row widths (RowBits:
// 256 and 512 bits) and the step loop of R1 and W1 (block_step_loop).
// Included by match.hip, match_radius.hip and match_wide.hip inside their anonymous namespaces, after match_keys.h.
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

// One resident query fragment: this lane's 16 bytes of query qi = the block's first + (lane & 31), rows of ROW_WORDS words. Queries at
// or beyond nq repeat the last one (padding: never stored). A block at a time: K4x sets up a block's list between two loads, and its
// code follows that.
template <int ROW_WORDS = kWords>
__device__ __forceinline__ void load_query_block(const uint32_t* __restrict__ q, uint32_t qi, uint32_t nq, uint32_t h, Fp4Row& qb,
                                                 const Fp4Consts& kc) {
  const uint4 p = *reinterpret_cast<const uint4*>(q + (size_t)(qi < nq ? qi : nq - 1u) * ROW_WORDS + 4u * h);
  expand_row(p, qb, kc);
}

// This lane's 16 packed bytes of row (row0 + 32 step + (lane & 31)), `behind` bytes further on for the later 256-bit parts of a wider
// row; steps beyond the tile's last repeat the last. No per-lane clamp: the DB's last step may reach up to 31
// rows past its end -- into the slack todhip_db_load leaves behind the descriptors (kDbSlackBytes, also behind a view; ctx.h holds
// it to 31 rows of the widest row), rows that the walks mask, never use -- and the address stays a wave-uniform base plus a
// constant lane offset (no vector instruction per load: the kernels are bound by those)
template <int ROW_WORDS>
struct StepLoaderT {
  const uint32_t* db;
  uint32_t row0, n_steps, lane_off;                          // lane_off: bytes from the step's first row
  __device__ __forceinline__ StepLoaderT(const uint32_t* d, uint32_t r0, uint32_t n, uint32_t c, uint32_t h)
      : db(d), row0(r0), n_steps(n), lane_off((c * ROW_WORDS + 4u * h) * 4u) {}
  __device__ __forceinline__ uint32_t first_row(uint32_t step) const { return row0 + 32u * min(step, n_steps - 1u); }   // wave-uniform
  __device__ __forceinline__ uint4 operator()(uint32_t step, uint32_t behind = 0u) const {
    const char* base = reinterpret_cast<const char*>(db) + (size_t)first_row(step) * (ROW_WORDS * 4u);
    return *reinterpret_cast<const uint4*>(base + lane_off + behind);
  }
};
using StepLoader = StepLoaderT<kWords>;

// ---- What the top-k DB passes do to their lists around the step loop: hamming_topk_fp4rows (match_fp4rows.h) and hamming_topk_wide
// (match_wide.hip) call these two. hamming_topk_mfma and hamming_topk_mfma_q32 (match_mfma.h) keep inline copies, the only ones left:
// with the functions hipcc allocates hamming_topk_mfma's registers anew -- measured when they were written (the QT = 6 forms) and again
// when W1 joined: QT = 6 gains 2 VGPRs and 3 SGPRs (<2, 6, 2>: 221 -> 223 of the 224 tests/test_build_checks.py allows), QT = 2 gains
// 15 instructions, QT = 4 and 8 do not move -- and that kernel is tuned to the code it has. The callers' code is the same either way.
// The exchange of distance bounds between tiles, once per share period: take the bounds loaded one period ago (a published bound stays
// valid: bounds only fall), publish a full list's bound if it improves on what was seen, start the loads of the next period.
// q0 + c: this lane's query of block 0; thr_of_limit: the row width's (dot > thr <=> d < limit); tightened(t): behind a threshold that
// took a foreign bound (the split blocks' part thresholds follow it there). Both come as lambdas, as block_step_loop's hooks do: handed
// thr_of_limit by its name, a pointer, hamming_topk_fp4rows' split forms came out with other registers (the call is resolved after
// the inlining, not with it)
template <int K, int QT, typename ThrOfLimit, typename Tightened>
__device__ __forceinline__ void exchange_bounds(uint32_t* bound, uint32_t q0, uint32_t c, uint32_t nq, const uint32_t (&best)[QT][K],
                                                uint32_t (&seen)[QT], float (&thr)[QT], ThrOfLimit thr_of_limit, Tightened tightened) {
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    const uint32_t qi = q0 + 32u * t + c;
    uint32_t* my_bound = bound + (qi < nq ? qi : nq - 1u);
    const uint32_t worst_d = best[t][K - 1] >> kLocalBits;
    if (worst_d < kNoLimit && worst_d < seen[t]) atomicMin(my_bound, worst_d);
    // a foreign bound is applied with <=: a smaller row index elsewhere may still win a tie
    if (seen[t] != 0xFFFFFFFFu) { thr[t] = fmaxf(thr[t], thr_of_limit(seen[t] + 1u)); tightened(t); }
    seen[t] = __hip_atomic_load(my_bound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
// The epilogue: lanes l and l + 32 hold the two halves of a query's rows: merge the partner's list, then K4's output format
// (partial keys + one flag byte per (tile, 64 queries); two query blocks share a flag, so both are stored when either kept something)
template <int K, int QT>
__device__ __forceinline__ void store_tile_lists(uint32_t (&best)[QT][K], uint32_t tile, uint32_t q0, uint32_t nq, uint32_t nq_pad,
                                                 uint32_t n_qw64, uint32_t lane, uint32_t c, uint32_t h, uint32_t* __restrict__ part,
                                                 uint8_t* __restrict__ stored) {
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    uint32_t other[K];
#pragma unroll
    for (int j = 0; j < K; ++j) other[j] = __shfl_xor(best[t][j], 32);
#pragma unroll
    for (int j = 0; j < K; ++j) topk_insert<K>(best[t], other[j]);
  }
#pragma unroll
  for (int u = 0; u < QT / 2; ++u) {
    const uint32_t qa = q0 + 64u * u + c, qb2 = qa + 32u;
    const bool any_a = qa < nq && best[2 * u][0] != 0xFFFFFFFFu, any_b = qb2 < nq && best[2 * u + 1][0] != 0xFFFFFFFFu;
    if (__builtin_amdgcn_ballot_w64(any_a || any_b) != 0ull) {  // some query below nq: the flag's index is below n_qw64
      if (h == 0u) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
          if (qa < nq) part[((size_t)tile * K + j) * nq_pad + qa] = best[2 * u][j];
          if (qb2 < nq) part[((size_t)tile * K + j) * nq_pad + qb2] = best[2 * u + 1][j];
        }
      }
      if (lane == 0) stored[(size_t)tile * n_qw64 + (q0 >> 6) + u] = 0;
    }
  }
}

// ---- Rows of BITS = 256 or 512 bits (ORB; BRISK, FREAK and the other 64-byte descriptors) for the passes that take the width as
// a parameter. A wider row is 256-bit parts in the layout above: lane l holds the 16 bytes at word 8 part + 4 (l >> 5). A 32 x 32
// block is 4 MFMAs per part, dot = BITS - 2 d, still exact in f32; the accumulator layout, block_row / lane_row_base, block_reaches
// and kNoBlock do not depend on the width (the least threshold of a 10-bit limit is 512 - 2 * 1023).
template <int BITS>
struct RowBits {
  static constexpr int kParts = BITS / 256, kRowWords = BITS / 32;
  struct Frag { Fp4Row part[kParts]; };                      // a lane's expanded share of one row or query
  struct Packed { uint4 part[kParts]; };                     // the same as loaded
  using Loader = StepLoaderT<kRowWords>;
  static __device__ __forceinline__ float thr_of_limit(uint32_t limit) { return (float)BITS - 2.f * (float)limit; }   // dot > thr <=> d < limit
  static __device__ __forceinline__ Packed load_step(const Loader& rows, uint32_t step) {
    Packed p;
#pragma unroll
    for (int i = 0; i < kParts; ++i) p.part[i] = rows(step, 32u * i);
    return p;
  }
  static __device__ __forceinline__ void expand(const Packed& p, Frag& f, const Fp4Consts& kc) {
#pragma unroll
    for (int i = 0; i < kParts; ++i) expand_row(p.part[i], f.part[i], kc);
  }
  static __device__ __forceinline__ void load_query_block(const uint32_t* __restrict__ q, uint32_t qi, uint32_t nq, uint32_t h, Frag& qb,
                                                          const Fp4Consts& kc) {
#pragma unroll
    for (int i = 0; i < kParts; ++i) ::load_query_block<kRowWords>(q + 8 * i, qi, nq, h, qb.part[i], kc);
  }
  static __device__ __forceinline__ mfma_f32x16 dot(const Frag& a, const Frag& b) {
    mfma_f32x16 acc = dot_block(a.part[0], b.part[0]);
#pragma unroll
    for (int i = 1; i < kParts; ++i)
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a.part[i].s[s], b.part[i].s[s], acc, 4, 4, 0, 0, 0, 0);
    return acc;
  }
};

// The DB pass of one wave over its tile (rows row0 .. row0 + n_local of db) against QT resident query blocks: what R1
// (match_radius.hip) and W1 (match_wide.hip) are around their tests. The packed rows of step s + 1 are loaded before step s is
// expanded and multiplied; the test of block t - 1 sits behind the MFMAs of block t; the step's last block waits in acc_odd for
// block 0 of the next step (QT is even) and the last step's is drained at the end.
//   test(acc, t, r_lane)   the accumulator of query block t (a constant once unrolled) over the rows r_lane | block_row(i), tile-local
//   after_step(step)       behind each step's blocks (W1: the exchange of bounds between tiles)
template <typename W, int QT, typename Test, typename AfterStep>
__device__ __forceinline__ void block_step_loop(const uint32_t* __restrict__ db, uint32_t row0, uint32_t n_local, uint32_t c, uint32_t h,
                                                const typename W::Frag (&qb)[QT], const Fp4Consts& kc, Test test, AfterStep after_step) {
  static_assert(QT % 2 == 0 && QT >= 2, "the pending block alternates between two accumulators");
  const uint32_t n_steps = (n_local + 31u) / 32u;
  const typename W::Loader rows(db, row0, n_steps, c, h);
  typename W::Packed p = W::load_step(rows, 0);
  mfma_f32x16 acc_even, acc_odd;                            // acc_odd: the previous step's last block -- none yet
#pragma unroll
  for (int i = 0; i < 16; ++i) acc_odd[i] = kNoBlock;
  for (uint32_t step = 0; step < n_steps; ++step) {
    typename W::Frag a;
    W::expand(p, a, kc);
    p = W::load_step(rows, step + 1u);
    const uint32_t r_lane = lane_row_base(step, h);
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      if (t & 1) acc_odd = W::dot(a, qb[t]); else acc_even = W::dot(a, qb[t]);
      if (t == 0) test(acc_odd, QT - 1, r_lane - 32u);      // the previous step's last block
      else test((t & 1) ? acc_even : acc_odd, t - 1, r_lane);
    }
    after_step(step);
  }
  test(acc_odd, QT - 1, lane_row_base(n_steps - 1u, h));    // drain
}
