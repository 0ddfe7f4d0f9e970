// K4x over the resident fp4 copy of the rows (layout: fp4_rows.h): expand_rows_fp4_kernel, which builds the copy, the loader of its
// fragments, the split-block tests and steps of this pass and hamming_topk_fp4rows -- the default DB pass of every launch of 4 or 6
// query blocks per wave (match_launch.h). Included by match.hip inside its anonymous namespace, after match_fp4.h (arithmetic, layout,
// block primitives, exchange_bounds, store_tile_lists), match_mfma.h (mfma_block_test) and match_pair_pack.h (PairPack).
// hamming_topk_mfma expands every packed row to fp4 again in every launch and in every query wave of its tile: 28 of the 82 vector
// instructions of a 32-row step of six split blocks, in a loop that is bound by vector issue. The DB is loaded once and searched for
// many frames, so the expansion is done once instead (expand_rows_fp4_kernel) and this pass loads the fragments as they stand: four
// 1 KB wave loads per step instead of one, nothing between them and the MFMAs. Same tiles, same tests, same lists, same output.

// The copy: one thread per 16-byte fragment (step, MFMA index, lane), n_steps whole steps of the rows at db -- the last one may reach
// up to 31 rows into the slack behind them (kDbSlackBytes), rows the pass masks. expand_word is the one definition of the bit assignment.
__global__ __launch_bounds__(kBlock) void expand_rows_fp4_kernel(const uint32_t* __restrict__ db, uint32_t n_steps, uint4* __restrict__ out) {
  const uint32_t s = blockIdx.x, m = threadIdx.x >> 6, l = threadIdx.x & 63u;   // kBlock = 4 x 64: a workgroup writes one step
  if (s >= n_steps) return;
  const Fp4Consts kc = fp4_consts();
  const mfma_i32x8 e = expand_word(db[(size_t)fp4_rows_src_row(s, l) * kWords + fp4_rows_src_word(m, l)], kc);
  *reinterpret_cast<uint4*>(reinterpret_cast<char*>(out) + fp4_rows_offset(s, m, l)) =
      uint4{(uint32_t)e[0], (uint32_t)e[1], (uint32_t)e[2], (uint32_t)e[3]};
}
static_assert(kBlock == 256, "expand_rows_fp4_kernel: one workgroup = the 4 x 64 fragments of a step");

// This lane's fragment m of step (step0 + step) of the copy; steps beyond the tile's last repeat the last. Buffer loads: the copy is the
// buffer (under 4 GiB: fp4_rows_ready), the lane offset the vector operand, the step a scalar offset -- no address arithmetic on the
// vector ALU and no address registers (a 64-bit vector address per load took the split-2 form to 229), and a load beyond the copy
// would return zeros instead of faulting. The m KB of the fragment go into the scalar offset (M_SCALAR) or onto the lane offset: both
// are free, but hipcc's register allocation differs -- with six query blocks and k = 2 the split forms take 228 registers the first
// way and 220 the second, the whole-block forms 222 and 225, and 224 is the budget (tests/test_build_checks.py).
typedef uint32_t fp4_u32x4 __attribute__((ext_vector_type(4)));
struct Fp4StepLoader {
  __amdgpu_buffer_rsrc_t copy;
  uint32_t step0, n_steps, lane_off;
  __device__ __forceinline__ Fp4StepLoader(const uint4* p, uint32_t copy_bytes, uint32_t s0, uint32_t n, uint32_t lane)
      : copy(__builtin_amdgcn_make_buffer_rsrc(const_cast<uint4*>(p), 0, (int)copy_bytes, 0x00020000)), step0(s0), n_steps(n),
        lane_off((uint32_t)fp4_rows_offset(0, 0, lane)) {}
  template <bool M_SCALAR>
  __device__ __forceinline__ mfma_i32x8 load(uint32_t step, uint32_t m) const {
    const uint32_t step_off = (uint32_t)fp4_rows_offset(step0 + min(step, n_steps - 1u), M_SCALAR ? m : 0u, 0);   // wave-uniform
    const fp4_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(copy, (int)(lane_off + (M_SCALAR ? 0u : m * kFp4FragBytes)), (int)step_off, 0);
    return mfma_i32x8{(int)v.x, (int)v.y, (int)v.z, (int)v.w, 0, 0, 0, 0};
  }
};

// mfma_block_test_part for this pass: the same test and the same completion, written for the path that all but one block in 2200 take
// on independent bits. The block that goes on is the unlikely side, so hipcc lays the completion (the other MFMAs, the second test, the
// walk) out behind the loop and the hot loop falls through from block to block instead of jumping over 1.2 KB per block; and the count
// of such blocks (half_stats) is bumped here, where it happens, as one wave-uniform counter -- a 0/1 flag per block, summed per trip,
// cost the fast path a join block and an s_add each (tools/mfma_valu_overlap.hip prices both; profiles/match_fastpath.json).
template <int K, int SPLIT>
__device__ __forceinline__ void fp4rows_block_test_part(mfma_f32x16& acc, const Fp4Row& rows, const Fp4Row& q, float& thr, float& thrp,
                                                        uint32_t r_lane, uint32_t n_lim, uint32_t (&best)[K], uint32_t& n_pass) {
  if (__builtin_expect(__builtin_amdgcn_ballot_w64(block_reaches<true, false>(acc, thrp)) == 0ull, 1)) return;
  ++n_pass;
#pragma unroll
  for (int s = SPLIT; s < 4; ++s) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(rows.s[s], q.s[s], acc, 4, 4, 0, 0, 0, 0);
  mfma_block_test<K, false, true>(acc, thr, r_lane, n_lim, best);
  thrp = thr - 64.f * (float)(4 - SPLIT);
}

// The same for the form whose fast path carries only what it uses (split 2: see the kernel): fragments 0 .. SPLIT-1 of the rows and of
// the queries (Fp4Frags<SPLIT>), nothing of the tails -- in the form above half of the loop's vector loads and 64 of its registers are
// there for one block in 2200. The block that goes on fetches its tails where it goes on: fragments SPLIT .. 3 of its OWN step (own_step, wave-uniform: the current step, or the one
// before for the block carried across a step) from the copy, and the lane's 16 packed bytes of its query qi, expanded by expand_word.
template <int N>
struct Fp4Frags { mfma_i32x8 s[N]; };
template <int N>
__device__ __forceinline__ mfma_f32x16 dot_frags(const Fp4Frags<N>& a, const Fp4Frags<N>& b) {
  mfma_f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < N; ++s) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a.s[s], b.s[s], acc, 4, 4, 0, 0, 0, 0);
  return acc;
}
// This lane's 16 packed bytes of query qi, as load_query_block reads them (queries at or beyond nq repeat the last one)
__device__ __forceinline__ uint4 load_query_packed(const uint32_t* __restrict__ q, uint32_t qi, uint32_t nq, uint32_t h) {
  return *reinterpret_cast<const uint4*>(q + (size_t)(qi < nq ? qi : nq - 1u) * kWords + 4u * h);
}
__device__ __forceinline__ uint32_t packed_word(const uint4& p, int m) { return m == 0 ? p.x : m == 1 ? p.y : m == 2 ? p.z : p.w; }

template <int K, int SPLIT>
__device__ __forceinline__ void fp4rows_block_test_part(mfma_f32x16& acc, const Fp4StepLoader& rows, uint32_t own_step,
                                                        const uint32_t* __restrict__ q, uint32_t qi, uint32_t nq, uint32_t h,
                                                        const Fp4Consts& kc, float& thr, float& thrp, uint32_t r_lane, uint32_t n_lim,
                                                        uint32_t (&best)[K], uint32_t& n_pass) {
  if (__builtin_expect(__builtin_amdgcn_ballot_w64(block_reaches<true, false>(acc, thrp)) == 0ull, 1)) return;
  ++n_pass;
  // everything the tails need is worked out HERE: hoisted in front of the loop, a query address per block and a lane offset per
  // fragment would sit in registers across the fast path for one block in two thousand (hence the fragment's KB in the scalar offset,
  // and qi made opaque)
  asm volatile("" : "+v"(qi));
  mfma_i32x8 tail[4 - SPLIT];
#pragma unroll
  for (int s = SPLIT; s < 4; ++s) tail[s - SPLIT] = rows.template load<true>(own_step, s);
  const uint4 p = load_query_packed(q, qi, nq, h);
#pragma unroll
  for (int s = SPLIT; s < 4; ++s)
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(tail[s - SPLIT], expand_word(packed_word(p, s), kc), acc, 4, 4, 0, 0, 0, 0);
  mfma_block_test<K, false, true>(acc, thr, r_lane, n_lim, best);
  // the new threshold as a register of its own: without this hipcc keeps the QT thresholds as pairs that it moves between register
  // pairs on the FAST side of every block (three v_mov_b64 per block in the split-2 form, 16 instructions per block instead of 13)
  asm("" : "+v"(thr));
  thrp = thr - 64.f * (float)(4 - SPLIT);
}

// mfma_step on the copy: the fragments of step next_step go straight into a_next, which holds the rows of the step BEFORE this one
// until then. Those are dead but for the block carried in from that step, which completes at t == 0 with its s[SPLIT .. 3]: the
// fragments below SPLIT are loaded at once (all four with whole blocks), the others behind that test. Nothing else differs.
template <int K, int QT, bool MASK, bool IMAX, int SPLIT = 0>
__device__ __forceinline__ void fp4rows_step(const Fp4Row& a, Fp4Row& a_next, const Fp4StepLoader& rows, uint32_t next_step,
                                             const Fp4Row (&qb)[QT], float (&thr)[QT], float (&thrp)[QT], uint32_t (&best)[QT][K],
                                             mfma_f32x16& acc_even, mfma_f32x16& acc_odd, uint32_t r_lane, uint32_t n_lim, uint32_t& n_pass) {
  constexpr bool HALF = SPLIT != 0;
  constexpr int kEarly = HALF ? SPLIT : 4;
  static_assert(!(HALF && MASK) && !(HALF && !IMAX) && QT >= 4, "split blocks: unmasked steps, integer maximum; >= 4 query blocks");
  static_assert(SPLIT == 0 || SPLIT == 2 || SPLIT == 3, "2 or 3 of the 4 MFMAs first");
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    if (HALF) { if (t & 1) acc_odd = dot_part0<HALF ? SPLIT : 2>(a, qb[t]); else acc_even = dot_part0<HALF ? SPLIT : 2>(a, qb[t]); }
    else { if (t & 1) acc_odd = dot_block(a, qb[t]); else acc_even = dot_block(a, qb[t]); }
    if (t == 0) {
#pragma unroll
      for (int m = 0; m < kEarly; ++m) a_next.s[m] = rows.template load<!HALF>(next_step, m);
    }
    if (t == 1) {
#pragma unroll
      for (int m = kEarly; m < 4; ++m) a_next.s[m] = rows.template load<!HALF>(next_step, m);
    }
    if (HALF) {
      if (t == 0) fp4rows_block_test_part<K, HALF ? SPLIT : 2>(acc_odd, a_next, qb[QT - 1], thr[QT - 1], thrp[QT - 1], r_lane - 32u, n_lim, best[QT - 1], n_pass);   // previous step's last block, its rows
      else fp4rows_block_test_part<K, HALF ? SPLIT : 2>((t & 1) ? acc_even : acc_odd, a, qb[t - 1], thr[t - 1], thrp[t - 1], r_lane, n_lim, best[t - 1], n_pass);
    } else {
      if (t == 0) mfma_block_test<K, MASK, IMAX>(acc_odd, thr[QT - 1], r_lane - 32u, n_lim, best[QT - 1]);   // previous step's last block
      else mfma_block_test<K, MASK, IMAX>((t & 1) ? acc_even : acc_odd, thr[t - 1], r_lane, n_lim, best[t - 1]);
    }
  }
}

// A step of the form that loads its tails on demand (written for SPLIT 2 / 3, used for 2: see the kernel; unmasked steps, integer maximum): every block starts with its first SPLIT MFMAs and only
// completes behind fp4rows_block_test_part, out of line, with tails it loads there. So a step loads fragments 0 .. SPLIT-1 of step
// `step + 1` and nothing else, and a_next's old rows are dead at once: the block carried in from the step before (t == 0) names that
// step, not registers. q0c: this lane's query of block 0.
template <int K, int QT, int SPLIT>
__device__ __forceinline__ void fp4rows_split_step(const Fp4Frags<SPLIT>& a, Fp4Frags<SPLIT>& a_next, const Fp4StepLoader& rows, uint32_t step,
                                                   const Fp4Frags<SPLIT> (&qh)[QT], const uint32_t* __restrict__ q, uint32_t q0c, uint32_t nq,
                                                   uint32_t h, const Fp4Consts& kc, float (&thr)[QT], float (&thrp)[QT],
                                                   uint32_t (&best)[QT][K], mfma_f32x16& acc_even, mfma_f32x16& acc_odd, uint32_t r_lane,
                                                   uint32_t n_lim, uint32_t& n_pass) {
  static_assert(SPLIT == 2 || SPLIT == 3, "2 or 3 of the 4 MFMAs first");
  static_assert(QT >= 4 && QT % 2 == 0, "the pending block alternates between two accumulators");
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    if (t & 1) acc_odd = dot_frags(a, qh[t]); else acc_even = dot_frags(a, qh[t]);
    if (t == 0) {
#pragma unroll
      for (int m = 0; m < SPLIT; ++m) a_next.s[m] = rows.template load<false>(step + 1u, m);
    }
    if (t == 0) fp4rows_block_test_part<K, SPLIT>(acc_odd, rows, step - 1u, q, q0c + 32u * (QT - 1), nq, h, kc, thr[QT - 1], thrp[QT - 1], r_lane - 32u, n_lim, best[QT - 1], n_pass);   // previous step's last block, its rows
    else fp4rows_block_test_part<K, SPLIT>((t & 1) ? acc_even : acc_odd, rows, step, q, q0c + 32u * (t - 1), nq, h, kc, thr[t - 1], thrp[t - 1], r_lane, n_lim, best[t - 1], n_pass);
  }
}

// ---- Two split blocks per accumulator (match_pair_pack.h has the packing; profiles/match_pairs.json the measurements). The block
// test above is at its operation count for 16 registers per block -- 8 v_max3 + a compare, in a loop bound by vector issue -- so the
// paired step tests 16 registers per TWO blocks: query blocks t and t + 1 of a row step share an accumulator, block t + 1's MFMAs
// scaled by 2^11, and 7 v_or3 + v_bitop3 + a compare answer for both. The bias is one per launch, so the fast path tests against
// the launch's radius, not against each query's tightened threshold: exact, since a threshold only rises (a block skipped at the
// radius is skipped at any tighter threshold), and the block that goes on applies its query's own thr as before.
struct PairConsts {
  mfma_f32x16 magic;          // srcC of a pair's first MFMA; also "no pending pair" (both flags clear)
  int scale_one, scale_field; // the E8M0 scales, in vector registers: from scalar ones hipcc copies both in front of every pair
  int bias;                   // field = dot + bias (wave-uniform)
};
__device__ __forceinline__ PairConsts pair_consts(uint32_t cut) {
  PairConsts pk;
  const float m = PairPack::magic(cut);
#pragma unroll
  for (int i = 0; i < 16; ++i) pk.magic[i] = m;
  asm volatile("v_mov_b32 %0, %1" : "=v"(pk.scale_one) : "n"(PairPack::kScaleOne));
  asm volatile("v_mov_b32 %0, %1" : "=v"(pk.scale_field) : "n"(PairPack::kScaleField));
  pk.bias = PairPack::bias(cut);
  return pk;
}
// The first block in the unscaled form of the instruction, the second with 2^11 on the rows: tools/mfma_valu_overlap.hip measured all
// four scaled at 79.7 cycles per block and this at 76.5 (today's block: 87.3). The empty asm keeps the MFMAs where they stand: hipcc
// otherwise sinks them behind the NEXT test, straight in front of their own, with s_nop 11 and one accumulator.
__device__ __forceinline__ void dot_pair(mfma_f32x16& acc, const Fp4Frags<2>& a, const Fp4Frags<2>& qa, const Fp4Frags<2>& qb, const PairConsts& pk) {
  acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a.s[0], qa.s[0], pk.magic, 4, 4, 0, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a.s[1], qa.s[1], acc, 4, 4, 0, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a.s[0], qb.s[0], acc, 4, 4, 0, pk.scale_field, 0, pk.scale_one);
  acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a.s[1], qb.s[1], acc, 4, 4, 0, pk.scale_field, 0, pk.scale_one);
  asm volatile("" : "+v"(acc));
}
// The OR of a packed accumulator's 16 registers, as a tree like block_reaches' maximum (hipcc reassociates plain ORs into one chain)
__device__ __forceinline__ uint32_t pair_or(const mfma_f32x16& acc) {
  uint32_t g[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    g[j] = (uint32_t)__float_as_int(acc[3 * j]) | (uint32_t)__float_as_int(acc[3 * j + 1]) | (uint32_t)__float_as_int(acc[3 * j + 2]);
    asm("" : "+v"(g[j]));
  }
  return (g[0] | g[1] | g[2]) | (g[3] | g[4] | (uint32_t)__float_as_int(acc[15]));
}
// Block FIELD of a pair goes on: its part is unpacked from its field (exact: the dot products of its first two MFMAs) and completes as
// fp4rows_block_test_part's block does -- the tails of its own step from the copy, its query's tail words, the test against the
// query's own thr, the walk. Unpacking keeps nothing for this path in registers across the fast path.
// The exchange of distance bounds between tiles happens here too, and only here: the paired fast path tests at the launch's radius
// and never reads thr, and a list changes nowhere else, so a periodic exchange_bounds in the loop bought the fast path nothing -- about
// 60 vector instructions, six sc1 loads the next trip waited for, and ten v_mov_b32 at every back edge for the seen[] it kept across
// the loop. The query's bound is loaded with the tails (one latency), applied in front of the test as exchange_bounds applies it (<=:
// a smaller row index elsewhere may still win a tie) and the list's own bound published behind it: never later than a periodic
// exchange would, and what is read is never staler. The tile-local row of the block (lane_row_base of its own step) is built here as
// well, from the wave-uniform step and an h made opaque as qi is: the loop carries neither.
template <int K, int FIELD>
__device__ __forceinline__ void fp4rows_pair_complete(const mfma_f32x16& packed, int bias, const Fp4StepLoader& rows, uint32_t own_step,
                                                      const uint32_t* __restrict__ q, uint32_t qi, uint32_t nq, uint32_t h, const Fp4Consts& kc,
                                                      float& thr, uint32_t n_lim, uint32_t (&best)[K], uint32_t& n_pass, uint32_t* bound) {
  ++n_pass;
  asm volatile("" : "+v"(qi));
  asm volatile("" : "+v"(h));
  const uint32_t r_lane = lane_row_base(own_step, h);
  uint32_t* my_bound = bound + (qi < nq ? qi : nq - 1u);
  const uint32_t seen = __hip_atomic_load(my_bound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  mfma_f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = (float)PairPack::unpack((uint32_t)__float_as_int(packed[i]), FIELD, bias);
  mfma_i32x8 tail[2];
#pragma unroll
  for (int s = 2; s < 4; ++s) tail[s - 2] = rows.template load<true>(own_step, s);
  const uint4 p = load_query_packed(q, qi, nq, h);
#pragma unroll
  for (int s = 2; s < 4; ++s)
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(tail[s - 2], expand_word(packed_word(p, s), kc), acc, 4, 4, 0, 0, 0, 0);
  if (seen != 0xFFFFFFFFu) thr = fmaxf(thr, thr_of_limit(seen + 1u));
  mfma_block_test<K, false, true>(acc, thr, r_lane, n_lim, best);
  const uint32_t worst_d = best[K - 1] >> kLocalBits;
  if (worst_d < kNoLimit && worst_d < seen) atomicMin(my_bound, worst_d);
  asm("" : "+v"(thr));        // (a register of its own: see fp4rows_block_test_part)
}
// The test of a pair (blocks ta and ta + 1 of own_step; qi: this lane's query of block ta). n_pass counts each block that goes on, by
// its own flag: a block whose partner alone went on is not counted.
template <int K>
__device__ __forceinline__ void fp4rows_pair_test(const mfma_f32x16& acc, const PairConsts& pk, const Fp4StepLoader& rows, uint32_t own_step,
                                                  const uint32_t* __restrict__ q, uint32_t qi, uint32_t nq, uint32_t h, const Fp4Consts& kc,
                                                  float& thr_a, float& thr_b, uint32_t n_lim, uint32_t (&best_a)[K],
                                                  uint32_t (&best_b)[K], uint32_t& n_pass, uint32_t* bound) {
  const uint32_t o = pair_or(acc);
  if (__builtin_expect(__builtin_amdgcn_ballot_w64((o & PairPack::kFlagMask) != 0u) == 0ull, 1)) return;
  if (__builtin_amdgcn_ballot_w64((o & PairPack::kFlagA) != 0u) != 0ull)
    fp4rows_pair_complete<K, 0>(acc, pk.bias, rows, own_step, q, qi, nq, h, kc, thr_a, n_lim, best_a, n_pass, bound);
  if (__builtin_amdgcn_ballot_w64((o & PairPack::kFlagB) != 0u) != 0ull)
    fp4rows_pair_complete<K, 1>(acc, pk.bias, rows, own_step, q, qi + 32u, nq, h, kc, thr_b, n_lim, best_b, n_pass, bound);
}
// fp4rows_split_step in pairs: QT / 2 pairs per step into two alternating accumulators, the test of a pair behind the MFMAs of the
// next (three accumulators, the test trailing further, measured no better), the step's last pair carried into the next step. With
// three pairs per step the pending pair's accumulator alternates per step: PH is the step's place in the loop's trip of two. Either
// way a trip starts and ends with its pending pair in acc_odd.
template <int K, int QT, int PH>
__device__ __forceinline__ void fp4rows_pair_step(const Fp4Frags<2>& a, Fp4Frags<2>& a_next, const Fp4StepLoader& rows, uint32_t step,
                                                  const Fp4Frags<2> (&qh)[QT], const uint32_t* __restrict__ q, uint32_t q0c, uint32_t nq,
                                                  uint32_t h, const Fp4Consts& kc, const PairConsts& pk, float (&thr)[QT],
                                                  uint32_t (&best)[QT][K], mfma_f32x16& acc_even, mfma_f32x16& acc_odd,
                                                  uint32_t n_lim, uint32_t& n_pass, uint32_t* bound) {
  static_assert(QT >= 4 && QT % 2 == 0, "whole pairs; the pending pair alternates between two accumulators");
  constexpr int NP = QT / 2;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const bool odd = ((NP * PH + j) & 1) != 0;
    dot_pair(odd ? acc_odd : acc_even, a, qh[2 * j], qh[2 * j + 1], pk);
    if (j == 0) {
#pragma unroll
      for (int m = 0; m < 2; ++m) a_next.s[m] = rows.template load<false>(step + 1u, m);
    }
    constexpr int kLast = NP - 1;
    if (j == 0) fp4rows_pair_test<K>(odd ? acc_even : acc_odd, pk, rows, step - 1u, q, q0c + 64u * kLast, nq, h, kc, thr[2 * kLast], thr[2 * kLast + 1], n_lim, best[2 * kLast], best[2 * kLast + 1], n_pass, bound);   // previous step's last pair, its rows
    else fp4rows_pair_test<K>(odd ? acc_even : acc_odd, pk, rows, step, q, q0c + 64u * (j - 1), nq, h, kc, thr[2 * j - 2], thr[2 * j - 1], n_lim, best[2 * j - 2], best[2 * j - 1], n_pass, bound);
  }
}

// A masked whole-block step (and the one before it when the loop leaves an odd step) in a split form: at most two per tile. The rows
// come complete (a); of the queries only the packed tail words are kept for these steps (qtail, loaded once per wave), and one block's
// tail is expanded at a time.
template <int K, int QT, int SPLIT>
__device__ __forceinline__ void fp4rows_split_masked_step(const Fp4Row& a, const Fp4Frags<SPLIT> (&qh)[QT], const uint32_t (&qtail)[QT][4 - SPLIT],
                                                          const Fp4Consts& kc, float (&thr)[QT], uint32_t (&best)[QT][K],
                                                          mfma_f32x16& acc_even, mfma_f32x16& acc_odd, uint32_t r_lane, uint32_t n_lim) {
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    Fp4Frags<SPLIT> ah;
#pragma unroll
    for (int s = 0; s < SPLIT; ++s) ah.s[s] = a.s[s];
    mfma_f32x16 acc = dot_frags(ah, qh[t]);
#pragma unroll
    for (int s = SPLIT; s < 4; ++s) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a.s[s], expand_word(qtail[t][s - SPLIT], kc), acc, 4, 4, 0, 0, 0, 0);
    if (t & 1) acc_odd = acc; else acc_even = acc;
    if (t == 0) mfma_block_test<K, true, true>(acc_odd, thr[QT - 1], r_lane - 32u, n_lim, best[QT - 1]);   // previous step's last block
    else mfma_block_test<K, true, true>((t & 1) ? acc_even : acc_odd, thr[t - 1], r_lane, n_lim, best[t - 1]);
  }
}

// hamming_topk_mfma with the rows read from their fp4 copy (rows_fp4: fp4_rows.h's layout of the rows the packed pass would read;
// rows_per_tile is a multiple of 32, so a tile starts on a step of the copy). MODE, the work items, the lists and the output as there,
// and one more: MODE 4 is split 2 in single blocks (fp4rows_split_step), the step MODE 2 had before it paired its blocks
// (fp4rows_pair_step) -- kept for A/B and diagnostics (TODHIP_K4X_PAIRS=0).
#ifndef TOD_K4X_STATIC_PRIO
#define TOD_K4X_STATIC_PRIO 1
#endif
template <int K, int QT, int MODE>
__global__ __launch_bounds__(kBlock, 2) void hamming_topk_fp4rows(const uint4* __restrict__ rows_fp4,
                                                                  const uint32_t* __restrict__ q, uint32_t n_rows,
                                                                  uint32_t nq, uint32_t nq_pad, uint32_t rows_per_tile,
                                                                  uint32_t n_tiles, uint32_t n_qw, uint32_t n_qw64,
                                                                  uint32_t blocks_per_xcd, uint32_t tiles_per_xcd, uint32_t cut,
                                                                  uint32_t share_period,
                                                                  uint32_t* __restrict__ part, uint32_t* bound,
                                                                  uint8_t* __restrict__ stored, uint32_t* half_stats) {
  static_assert(QT == 4 || QT == 6, "four or six query blocks per wave: with eight the fragments of two steps do not fit beside them");
  constexpr bool IMAX = MODE >= 1;
  constexpr int HALF = MODE == 4 ? 2 : (MODE >= 2 ? MODE : 0);        // the split (0: whole blocks)
  constexpr float kPartOff = HALF ? 64.f * (float)(4 - HALF) : 0.f;   // what the positions behind the split can still add to a dot product
  const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3;
  uint32_t tile, qw;
  if (tiles_per_xcd) {
    const uint32_t local = __builtin_amdgcn_readfirstlane(slot * kWavesPerBlock + (threadIdx.x >> 6));
    if (local >= tiles_per_xcd * n_qw) return;
    tile = xcd * tiles_per_xcd + local / n_qw; qw = local % n_qw;
  } else {
    const uint32_t vblock = xcd * blocks_per_xcd + slot;
    const uint32_t item = __builtin_amdgcn_readfirstlane(vblock * kWavesPerBlock + (threadIdx.x >> 6));
    tile = item / n_qw; qw = item % n_qw;
  }
  if (tile >= n_tiles) return;
  const uint32_t lane = threadIdx.x & 63u, c = lane & 31u, h = lane >> 5;
  const uint32_t q0 = qw * (32u * QT);

  const Fp4Consts kc = fp4_consts();                                  // (the queries are still expanded here, once per wave)
  // TAILS: the loop keeps only the fragments in front of the split, and a block that goes on loads its tails (fp4rows_split_step).
  // Split 2 alone: on data where split 2 pays, one block in 2200 goes on. Split 3 is what the adaptive launch probes on data where
  // every second block goes on (match_split.h); there each such block would wait for its loads, and at 32 000 x 1M split 3 gained
  // nothing from it (profiles/match_tails.json). Split 3 and whole blocks keep all four fragments resident, as before.
  constexpr bool TAILS = HALF == 2;
  constexpr bool PAIRS = MODE == 2;                                   // two blocks per accumulator, tested at the launch's radius
  constexpr int NF = TAILS ? HALF : 4;                                // the fragments the loop keeps
  using Frags = typename std::conditional<TAILS, Fp4Frags<NF>, Fp4Row>::type;
  Frags qb[QT];
  uint32_t best[QT][K];
  float thr[QT], thrp[QT];                                            // (thrp: not in the paired form)
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    if constexpr (TAILS) {
      const uint4 p = load_query_packed(q, q0 + 32u * t + c, nq, h);
#pragma unroll
      for (int m = 0; m < NF; ++m) qb[t].s[m] = expand_word(packed_word(p, m), kc);
    } else {
      load_query_block(q, q0 + 32u * t + c, nq, h, qb[t], kc);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) best[t][j] = 0xFFFFFFFFu;
    thr[t] = thr_of_limit(cut);
    if constexpr (!PAIRS) thrp[t] = thr[t] - kPartOff;
  }

  const uint32_t row0 = tile * rows_per_tile;
  const uint32_t n_local = min(n_rows, row0 + rows_per_tile) - row0;  // > 0: tile < n_tiles
  const uint32_t n_full = n_local / 32u, n_steps = (n_local + 31u) / 32u;   // the DB's last step may be partial
  const Fp4StepLoader rows(rows_fp4, (uint32_t)fp4_rows_bytes(n_rows), row0 / 32u, n_steps, lane);
  Frags a0, a1;
#pragma unroll
  for (int m = 0; m < NF; ++m) a0.s[m] = rows.template load<false>(0, m);
  a1 = a0;                                                            // "the step before the first": its pending block is none
  mfma_f32x16 acc_even, acc_odd;
  PairConsts pk;
  if constexpr (PAIRS) { pk = pair_consts(cut); acc_odd = pk.magic; }   // "no pending pair"
  else {
#pragma unroll
    for (int i = 0; i < 16; ++i) acc_odd[i] = kNoBlock;
  }
  // The periodic exchange of bounds and its state, in every form but the paired one, which exchanges where a block goes on
  // (fp4rows_pair_complete) and so ignores share_period
  [[maybe_unused]] uint32_t seen[QT], next_share = 2u;
  if constexpr (!PAIRS) {
#pragma unroll
    for (int t = 0; t < QT; ++t) seen[t] = 0xFFFFFFFFu;              // "nothing published"
  }
  uint32_t step = 0, n_pass = 0;
  // Static priority for half of the workgroups, set once in front of the loop: the two waves of a SIMD run the same program, and at
  // equal priority the older one wins every arbitration. Workgroups are dealt out over the 8 XCDs and then over an XCD's 32 CUs, so
  // bit 5 of the slot tells a CU's first workgroup from its second in the first round and splits the later ones evenly. Measured at
  // 32 000 x 1M, split 2, alternating: 1.378 -> 1.353 ms (profiles/match_fastpath.json); it changes no result. Only in the form it
  // was measured to pay in, split 2 with six query blocks: raised everywhere it also outranked ORB's and the verifier's kernels in
  // the chained pipeline, whose DB runs whole blocks or split 3 (one run: 10 428 -> 9 522 frames/s), and whole blocks gained 0.7 %.
  // TOD_K4X_STATIC_PRIO=0: a build without it, for the A/B (tools/match_pairs.sh prio).
  if (TOD_K4X_STATIC_PRIO && HALF == 2 && QT == 6 && ((slot >> 5) & 1u)) __builtin_amdgcn_s_setprio(1);
  for (; step + 2u <= n_full; step += 2u) {                           // two steps per trip: the fragments ping-pong between a0 and a1
    if constexpr (PAIRS) {
      fp4rows_pair_step<K, QT, 0>(a0, a1, rows, step, qb, q, q0 + c, nq, h, kc, pk, thr, best, acc_even, acc_odd, n_local, n_pass, bound);
      fp4rows_pair_step<K, QT, 1>(a1, a0, rows, step + 1u, qb, q, q0 + c, nq, h, kc, pk, thr, best, acc_even, acc_odd, n_local, n_pass, bound);
    } else if constexpr (TAILS) {
      fp4rows_split_step<K, QT, NF>(a0, a1, rows, step, qb, q, q0 + c, nq, h, kc, thr, thrp, best, acc_even, acc_odd, lane_row_base(step, h), n_local, n_pass);
      fp4rows_split_step<K, QT, NF>(a1, a0, rows, step + 1u, qb, q, q0 + c, nq, h, kc, thr, thrp, best, acc_even, acc_odd, lane_row_base(step, h) + 32u, n_local, n_pass);
    } else {
      fp4rows_step<K, QT, false, IMAX, HALF>(a0, a1, rows, step + 1u, qb, thr, thrp, best, acc_even, acc_odd, lane_row_base(step, h), n_local, n_pass);
      fp4rows_step<K, QT, false, IMAX, HALF>(a1, a0, rows, step + 2u, qb, thr, thrp, best, acc_even, acc_odd, lane_row_base(step, h) + 32u, n_local, n_pass);
    }
    if constexpr (!PAIRS) {
      if (step + 2u >= next_share) {                                  // wave-uniform
        next_share += share_period;
        exchange_bounds<K, QT>(bound, q0, c, nq, best, seen, thr, [](uint32_t limit) { return thr_of_limit(limit); },
                               [&](int t) { thrp[t] = thr[t] - kPartOff; });
      }
    }
  }
  if constexpr (TAILS) {
    // the last unmasked step's last block is still a part: it completes here, in the same form, with the tails of step - 1
    if (step > 0u) {
      if constexpr (PAIRS)                                            // (the last pair, likewise)
        fp4rows_pair_test<K>(acc_odd, pk, rows, step - 1u, q, q0 + c + 32u * (QT - 2), nq, h, kc, thr[QT - 2], thr[QT - 1], n_local, best[QT - 2], best[QT - 1], n_pass, bound);
      else
        fp4rows_block_test_part<K, NF>(acc_odd, rows, step - 1u, q, q0 + c + 32u * (QT - 1), nq, h, kc, thr[QT - 1], thrp[QT - 1], lane_row_base(step - 1u, h), n_local, best[QT - 1], n_pass);
#pragma unroll
      for (int i = 0; i < 16; ++i) acc_odd[i] = kNoBlock;
      if (lane == 0 && half_stats) { atomicAdd(half_stats, n_pass); atomicAdd(half_stats + 1, step * (uint32_t)QT); }
    }
    // at most one full and one partial step: masked, whole blocks. They need complete rows and queries: a0 holds the first fragments of
    // `step`, the others and the queries' packed tail words are loaded here, once per wave
    if (step < n_steps) {                                             // wave-uniform
      uint32_t qtail[QT][4 - NF];
#pragma unroll
      for (int t = 0; t < QT; ++t) {
        const uint4 p = load_query_packed(q, q0 + 32u * t + c, nq, h);
#pragma unroll
        for (int m = NF; m < 4; ++m) qtail[t][m - NF] = packed_word(p, m);
      }
      Fp4Row a, a_next;
#pragma unroll
      for (int m = 0; m < NF; ++m) a.s[m] = a0.s[m];
#pragma unroll
      for (int m = NF; m < 4; ++m) a.s[m] = rows.template load<false>(step, m);
      for (; step < n_steps; ++step) {
#pragma unroll
        for (int m = 0; m < 4; ++m) a_next.s[m] = rows.template load<false>(step + 1u, m);
        fp4rows_split_masked_step<K, QT, NF>(a, qb, qtail, kc, thr, best, acc_even, acc_odd, lane_row_base(step, h), n_local);
        a = a_next;
      }
    }
  } else {
    // the last unmasked step's last block is still a part: it completes here, with that step's rows (a1)
    if (HALF && step > 0u) {
      fp4rows_block_test_part<K, HALF ? HALF : 2>(acc_odd, a1, qb[QT - 1], thr[QT - 1], thrp[QT - 1], lane_row_base(step - 1u, h), n_local, best[QT - 1], n_pass);
#pragma unroll
      for (int i = 0; i < 16; ++i) acc_odd[i] = kNoBlock;
      if (lane == 0 && half_stats) { atomicAdd(half_stats, n_pass); atomicAdd(half_stats + 1, step * (uint32_t)QT); }
    }
    for (; step < n_steps; ++step) {                                  // at most one full and one partial step: masked, whole blocks
      fp4rows_step<K, QT, true, IMAX>(a0, a1, rows, step + 1u, qb, thr, thrp, best, acc_even, acc_odd, lane_row_base(step, h), n_local, n_pass);
      a0 = a1;
    }
  }
  mfma_block_test<K, true, IMAX>(acc_odd, thr[QT - 1], lane_row_base(n_steps - 1u, h), n_local, best[QT - 1]);   // drain
  store_tile_lists<K, QT>(best, tile, q0, nq, nq_pad, n_qw64, lane, c, h, part, stored);
}
