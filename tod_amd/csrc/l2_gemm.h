// The float matcher's DB pass, L2G (passes 0, 1 and 2 of l2.hip's head comment): one bf16 GEMM on the matrix cores whose epilogue
// keeps per-lane minima, per-lane top lists or the candidates below a threshold. Included by l2.hip.
#pragma once

namespace {

typedef __attribute__((ext_vector_type(8))) short bf16x8;  // 8 bf16 = 4 VGPRs: one MFMA A/B fragment
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// diagnostics builds (tools/l2_ablate.sh; results are garbage): -DTOD_L2_ABLATE=1 no DMA of the next tiles, 2 no LDS reads of the next
// tile's fragments, 3 neither
#ifdef TOD_L2_ABLATE
constexpr bool kAblateDma = TOD_L2_ABLATE == 1 || TOD_L2_ABLATE == 3, kAblateLdsReads = TOD_L2_ABLATE >= 2;
#else
constexpr bool kAblateDma = false, kAblateLdsReads = false;
#endif

// Where pass 2 puts a lane's candidates. A lane is the only writer for (query, chunk, lane half): its first kSlot rows go to a
// private slot with plain stores and a count in a register -- nothing to wait for. (An atomic append to one list per query, the
// round-1 form, costs a round trip to L2 per candidate with every outstanding load drained first, and with some hundreds
// of candidates per query at the eps band of bf16 that was most of the pass.) Rows beyond kSlot go to the shared list.
struct CandSink {
  uint32_t* __restrict__ slots;        // [nq_pad][n_parts][kSlot]
  uint32_t* __restrict__ shared;       // [nq_pad][kCandCap]
  uint32_t* __restrict__ shared_cnt;   // [nq_pad]
  uint32_t n_parts, part;              // this lane's partition = 2 chunk + h
};

// What becomes of the 16 scores a lane holds for query q (register i <-> DB row row0 + (i & 3) + 8 (i >> 2), row0 including the
// lane half's 4 h).
//   pass 1, KT > 1: the KT smallest below `limit` in `best` (ascending), and the limit follows best[KT - 1]
//   pass 1, KT = 1: the minimum only -- one instruction behind the min tree, no branch (the seed pass: the k-th smallest of
//                   the partitions' minima is the score of k distinct rows, hence an upper bound of A_k like the exact k-th)
//   pass 2: rows with score <= limit are appended to the lane's slot (`cnt` rows so far)
template <int PASS, uint32_t KT>
__device__ __forceinline__ void l2_epilogue(const f32x16& sc, float& limit, float (&best)[KT], uint32_t& cnt, uint32_t q, uint32_t row0,
                                            const CandSink& sink) {
  if (PASS == 2) {
    // two levels, so that a tile with one candidate among its 64 x 16 scores (the usual case when there is any) pays four
    // group tests and four leaf tests rather than sixteen: minima of the four register groups (= row groups 8 g + 4 h ..+3)
    float gm[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) gm[g] = fminf(fminf(fminf(sc[4 * g], sc[4 * g + 1]), sc[4 * g + 2]), sc[4 * g + 3]);
    const float m = fminf(fminf(fminf(gm[0], gm[1]), gm[2]), gm[3]);
    if (__builtin_amdgcn_ballot_w64(m <= limit) != 0ull) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        if (__builtin_amdgcn_ballot_w64(gm[g] <= limit) != 0ull) {   // wave-uniform
          asm volatile("");                                           // a scalar branch of its own, not folded into the lanes' tests below
#pragma unroll
          for (int i = 4 * g; i < 4 * g + 4; ++i) {
            if (sc[i] <= limit) {
              uint32_t base = row0;
              asm volatile("" : "+v"(base));                    // keeps the 16 row numbers from being hoisted into 16 registers of the main path
              const uint32_t row = base + (uint32_t)(i & 3) + 8u * (uint32_t)(i >> 2);
              if (cnt < kSlot) {
                sink.slots[((size_t)q * sink.n_parts + sink.part) * kSlot + cnt] = row;
              } else {
                const uint32_t at = atomicAdd(&sink.shared_cnt[q], 1u);
                if (at < kCandCap) sink.shared[(size_t)q * kCandCap + at] = row;
              }
              ++cnt;
            }
          }
        }
      }
    }
    return;
  }
  float m = fminf(fminf(sc[0], sc[1]), sc[2]);
#pragma unroll
  for (int i = 3; i < 15; i += 2) m = fminf(fminf(m, sc[i]), sc[i + 1]);
  m = fminf(m, sc[15]);
  if (KT == 1) {
    best[0] = fminf(best[0], m);
  } else {
    if (__builtin_amdgcn_ballot_w64(m < limit) != 0ull) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (__builtin_amdgcn_ballot_w64(sc[i] < limit) != 0ull) {    // wave-uniform: usually one value of the 16
          float v = sc[i] < limit ? sc[i] : FLT_MAX;                  // FLT_MAX falls through the list unchanged
#pragma unroll
          for (uint32_t j = 0; j < KT; ++j) { const float lo = fminf(best[j], v); v = fmaxf(best[j], v); best[j] = lo; }
        }
      }
      limit = fminf(limit, best[KT - 1]);
    }
  }
}

// L2G. One WAVE = (DB chunk, 128 queries): 4 query tiles of 32 as B fragments in registers (128 VGPRs); the DB streams through
// in tiles of 32 rows that are stored in A-fragment order (l2_prepare_kernel), so a tile is 8 contiguous 1 KB wave-loads whose
// lane l part is exactly what lane l feeds the MFMA -- LDS is only a FIFO between the load and the register, never a
// transpose. No barrier, no dependence between the waves of a block (they load the same tiles at about the same time, so
// three of four loads hit the CU's L1). The row norms enter as the C operand of a tile's first MFMA, so the accumulator IS
// the score; the epilogue of query tile t sits behind the MFMAs of tile t + 1 (two accumulators).
// KT: per-lane list length of pass 1 (1: minimum only, the seed pass; 4 when k <= 4: 16 VGPRs less), unused in pass 2
// D: floats per row, kDim or kDimNarrow. The comments below give kDim's numbers; what depends on the width is taken from l2_plan.h's
// l2_k_steps (8 or 4 segments, loads and MFMAs per tile), l2_tile_loads (9 or 5: what the vmcnt waits count in) and
// l2_ring_slot_bytes. At 64 the query fragments are 64 VGPRs and a tile is 4 KB; the geometry, the sink and the epilogues are the same.
template <int PASS, uint32_t KT, uint32_t D = kDim>
__global__ __launch_bounds__(256, 2) void l2_gemm_kernel(const uint16_t* __restrict__ db, const float* __restrict__ dbn,
                                                         uint32_t n_tiles, uint32_t tiles_per_chunk, uint32_t tile_stride,
                                                         const uint16_t* __restrict__ qh, uint32_t nq_pad,
                                                         float* __restrict__ part, const float* __restrict__ thr,
                                                         uint32_t* __restrict__ slots, uint32_t* __restrict__ slot_cnt,
                                                         uint32_t* __restrict__ cand, uint32_t* __restrict__ cand_cnt) {
  // tile_stride: tile t of the launch is DB tile t * tile_stride (the seed pass samples the DB evenly; 1 otherwise)
  // thr: PASS 1 -- optional per-query seed (only scores below it can matter), PASS 2 -- the candidate threshold
  const uint32_t tid = threadIdx.x, wave = tid >> 6, l = tid & 63u, r = l & 31u, h = l >> 5;
  const uint32_t chunk = blockIdx.x;
  const uint32_t q_base = blockIdx.y * kBlockQueries + wave * (kQTilesPerWave * 32u);
  const uint32_t t_begin = chunk * tiles_per_chunk, t_end = min(n_tiles, t_begin + tiles_per_chunk);
  if (t_begin >= t_end) return;
  const uint64_t t_start = (PASS == 2 && part) ? __builtin_amdgcn_s_memrealtime() : 0ull;

  // this wave's query fragments: B[k = 16 s + 8 h + j][col r] = q^[q_base + 32 t + r][16 s + 8 h + j]
  constexpr uint32_t kSteps = l2_k_steps(D), kNormOff = kTileRows * D * 2u, kSlotBytes = l2_ring_slot_bytes(D);
  bf16x8 bq[kQTilesPerWave][kSteps];
#pragma unroll
  for (uint32_t t = 0; t < kQTilesPerWave; ++t) {
    const uint16_t* qp = qh + (size_t)(q_base + 32u * t + r) * D + 8u * h;
#pragma unroll
    for (uint32_t s = 0; s < kSteps; ++s) bq[t][s] = *reinterpret_cast<const bf16x8*>(qp + 16u * s);
  }
  float best[kQTilesPerWave][KT];
  float limit[kQTilesPerWave];
  uint32_t n_cand[kQTilesPerWave];                          // pass 2: rows this lane has appended per query
#pragma unroll
  for (uint32_t t = 0; t < kQTilesPerWave; ++t) {
#pragma unroll
    for (uint32_t j = 0; j < KT; ++j) best[t][j] = FLT_MAX;
    limit[t] = (PASS == 1 && !thr) ? FLT_MAX : thr[q_base + 32u * t + r];
    n_cand[t] = 0u;
  }
  const CandSink sink{slots, cand, cand_cnt, 2u * gridDim.x, 2u * chunk + h};
  // everything loaded so far is waited for HERE: the compiler does not see the ring's loads below, and a wait of its own for one
  // of these, placed lazily inside the loop, would be counted without them and drain the ring
#pragma unroll
  for (uint32_t t = 0; t < kQTilesPerWave; ++t) {
#pragma unroll
    for (uint32_t s = 0; s < kSteps; ++s) asm volatile("" :: "v"(bq[t][s]));
    asm volatile("" :: "v"(limit[t]));
  }
  // The wave's private ring in LDS: two slots of one DB tile (8 KB of fragments, already in register order) + its 32 row norms
  // (twice: the 64 lanes of the load bring them as lanes l & 31). A slot is filled by 9 loads that write LDS directly
  // (global_load_lds: no destination registers, so their depth costs nothing) and read back with ds_read_b128 -- lane l
  // gets exactly the 16 bytes lane l loaded. Written as asm, with the vmcnt waits counted by hand: loads retire in order, each
  // tile is exactly 9 of them, and "at most 9 outstanding" therefore means the older of the two tiles in flight has landed
  // (the compiler would wait for everything before any LDS read, which is the depth this ring exists for).
  __shared__ __attribute__((aligned(16))) uint8_t ring[kWaves][2][kSlotBytes];
  typedef __attribute__((address_space(3))) void* lptr_t;
  const uint32_t ring_lds = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(size_t)(lptr_t)(&ring[wave][0][0]));
  const uint32_t frag_off = l * 16u, norm_off = r * 4u;
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
#define L2_DMA(width_, voff_, gaddr_, lds_)                                                                     \
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_" width_ " %0, %1" :: "v"(voff_), "s"(gaddr_), "s"(lds_) : "memory", "m0")
  auto issue = [&](uint32_t tile, uint32_t slot) {
    tile = min(tile, t_end - 1u);                           // past the chunk: a harmless reload, the count per tile stays 9
    // (the addresses are wave-uniform; readfirstlane says so in a way the "s" constraints below can rely on)
    auto uniform64 = [](uint64_t v) {
      return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32) |
             (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    };
    const uint64_t g = uniform64((uint64_t)(db + (size_t)tile * tile_stride * (kTileRows * D)));
    const uint64_t gn = uniform64((uint64_t)(dbn + (size_t)tile * tile_stride * kTileRows));
    const uint32_t lds = ring_lds + slot * kSlotBytes;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the slot's previous tile has been read out
#pragma unroll
    for (uint32_t s = 0; s < kSteps; ++s) L2_DMA("dwordx4", frag_off, g + s * 1024u, lds + s * 1024u);
    L2_DMA("dword", norm_off, gn, lds + kNormOff);
  };
  // "at most one tile's loads outstanding": the older of the two tiles in flight has landed
#define L2_WAIT_OLDER_TILE() asm volatile("s_waitcnt vmcnt(%0)" :: "n"(l2_tile_loads(D)) : "memory")
  // One DB tile against the wave's 4 query tiles. The tile's fragments live in ONE register set: the last query tile's
  // MFMA of k-step s is the last reader of a[s], and the next tile's a[s] is read from the ring right behind it (a second
  // set would not fit beside the 128 query registers at two waves per SIMD; LDS latency is what that distance covers).
  bf16x8 a[kSteps];
  // |row|^2 of the rows this lane's accumulators belong to (register 4 g + i <-> row 8 g + 4 h + i): the C operand of a query
  // tile's first MFMA. Like a[], ONE register set, reloaded behind its last reader.
  f32x16 nrm;
  auto read_frag = [&](uint32_t slot, uint32_t s) { return *reinterpret_cast<const bf16x8*>(&ring[wave][slot][s * 1024u + frag_off]); };
  auto read_norms = [&](uint32_t slot) {
    const float* np = reinterpret_cast<const float*>(&ring[wave][slot][kNormOff]) + 4u * h;
#pragma unroll
    for (uint32_t gg = 0; gg < 4; ++gg) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(np + 8u * gg);
      nrm[4 * gg + 0] = v[0]; nrm[4 * gg + 1] = v[1]; nrm[4 * gg + 2] = v[2]; nrm[4 * gg + 3] = v[3];
    }
  };
  issue(t_begin, 0u);
  issue(t_begin + 1u, 1u);
  L2_WAIT_OLDER_TILE();
#pragma unroll
  for (uint32_t s = 0; s < kSteps; ++s) a[s] = read_frag(0u, s);
  read_norms(0u);
  uint32_t cur = 0;
  for (uint32_t tile = t_begin; tile < t_end; ++tile, cur ^= 1u) {
    if (!kAblateDma) issue(tile + 2u, cur);                 // in flight now: tile + 1 (the other slot) and tile + 2
    f32x16 acc[2];
    auto mfma_tile = [&](uint32_t t) {
      if (!kAblateDma && t + 1 == kQTilesPerWave) L2_WAIT_OLDER_TILE();                                // tile + 1 has landed
      f32x16 c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], bq[t][0], nrm, 0, 0, 0);
      if (!kAblateLdsReads && t + 1 == kQTilesPerWave) { a[0] = read_frag(cur ^ 1u, 0u); read_norms(cur ^ 1u); }
#pragma unroll
      for (uint32_t s = 1; s < kSteps; ++s) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s], bq[t][s], c, 0, 0, 0);
        if (!kAblateLdsReads && t + 1 == kQTilesPerWave) a[s] = read_frag(cur ^ 1u, s);
      }
      return c;
    };
    acc[0] = mfma_tile(0);
#pragma unroll
    for (uint32_t t = 0; t < kQTilesPerWave; ++t) {
      if (t + 1 < kQTilesPerWave) acc[(t + 1) & 1u] = mfma_tile(t + 1);
      l2_epilogue<PASS, KT>(acc[t & 1u], limit[t], best[t], n_cand[t], q_base + 32u * t + r, tile * tile_stride * kTileRows + 4u * h, sink);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // nothing may still be on its way into this block's LDS when it is handed on
#undef L2_WAIT_OLDER_TILE
#undef L2_DMA
#pragma clang diagnostic pop
  if (PASS == 2) {
#pragma unroll
    for (uint32_t t = 0; t < kQTilesPerWave; ++t) slot_cnt[(size_t)(q_base + 32u * t + r) * sink.n_parts + sink.part] = n_cand[t];
    if (part && l == 0) {                                   // diagnostics (TODHIP_L2_TRACE): when each wave started and ended, 100 MHz ticks
      uint64_t* tr = reinterpret_cast<uint64_t*>(part) + 2u * (((size_t)blockIdx.y * gridDim.x + chunk) * kWaves + wave);
      tr[0] = t_start; tr[1] = __builtin_amdgcn_s_memrealtime();
    }
  }
  if (PASS == 1) {
    // partition (chunk, lane half): kTop ascending scores per query
#pragma unroll
    for (uint32_t t = 0; t < kQTilesPerWave; ++t) {
      float* dst = part + ((size_t)(chunk * 2u + h) * nq_pad + (q_base + 32u * t + r)) * kTop;
#pragma unroll
      for (uint32_t j = 0; j < kTop; ++j) dst[j] = j < KT ? best[t][j] : FLT_MAX;
    }
  }
}

}  // namespace
