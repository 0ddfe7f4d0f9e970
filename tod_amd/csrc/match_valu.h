// K4, the exact search on the vector ALU (overview: match.hip): the accumulating popcount, the hand-issued scalar loads of the DB
// rows, the partial-distance elimination schedules and hamming_topk_tiles. The radius bound restates DescriptorMatcher.cpp:212-220.
// Included by match.hip inside its anonymous namespace, after match_keys.h.

// popcount with accumulate: v_bcnt_u32_b32 D = countbits(S0) + S1. Written as asm because the compiler
// otherwise re-associates the chain into bcnt(x, 0) + v_add3 trees (3 extra VALU ops per row).
__device__ __forceinline__ uint32_t bcnt_acc(uint32_t x, uint32_t acc) {
  uint32_t d;
  asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(d) : "v"(x), "v"(acc));
  return d;
}

typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));

// One SGPR group = kGroupRows (4) DB rows = two s_load_dwordx16. The loads are issued and waited for by
// hand (asm): hipcc otherwise sinks a prefetch below its consumer. Scalar loads return out of order, so the
// only usable wait is lgkmcnt(0); the ping-pong below always has exactly one group in flight when it waits.
struct RowGroup { u32x16 lo, hi; };

__device__ __forceinline__ void issue_rows(RowGroup& g, const uint32_t* p) {
  asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx16 %1, %2, 0x40"
               : "=&s"(g.lo), "=&s"(g.hi) : "s"(p) : "memory");
  __builtin_amdgcn_sched_barrier(0);   // keep the prefetch ahead of the compute it overlaps with
}
__device__ __forceinline__ void wait_rows(RowGroup& g) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(g.lo), "+s"(g.hi));
}

// bits [32 W0, 32 W0 + 128) of row HALF of a 2-row SGPR block, accumulated onto acc
template <int HALF, int W0>
__device__ __forceinline__ uint32_t hamming128(const uint32_t (&q)[kWords], const u32x16& rows, uint32_t acc) {
#pragma unroll
  for (int w = W0; w < W0 + 4; ++w) acc = bcnt_acc(q[w] ^ rows[HALF * kWords + w], acc);
  return acc;
}

__device__ __forceinline__ uint32_t hamming256_mem(const uint32_t (&q)[kWords], const uint32_t* row) {
  uint32_t d = 0;
#pragma unroll
  for (int w = 0; w < kWords; ++w) d = bcnt_acc(q[w] ^ row[w], d);
  return d;
}

// `limit` = min(own k-th best distance, 1 + the smallest k-th best distance any tile has published for this
// query): a row at or above it cannot be among the k nearest of the whole DB (ties with a foreign bound are kept
// because a smaller row index could still win them), so skipping it keeps the merged result exact.
// MODE picks the elimination schedule by how tight the initial bound (radius + 1) is; every schedule is exact.
//   2: test after 96 bits per row, then after 128, after 192, then the rest   (pays for cut <= 38: a row passes the first test
//      in some lane with probability ~0.3 on independent bits at cut 36, ~0.9 at cut 40)
//   1: test after 128 bits per 4 rows, then the rest                  (38 < cut <= 48)
//   3: test after 192 bits per 4 rows, then the rest                  (48 < cut <= 80, e.g. radius 55 of conf/detection.ros.ork:60)
//   0: full distances, one test per 4 rows                            (larger radii: no lower bound prunes anything)
template <int K, int MODE>
__device__ __forceinline__ void consume_group(const uint32_t (&qd)[kWords], const RowGroup& g, uint32_t r,
                                              uint32_t (&best)[K], uint32_t& worst_d, uint32_t& limit, uint32_t foreign) {
  if (MODE != 2) {
    // the four rows' accumulate chains are interleaved word by word: no instruction depends on its predecessor
    constexpr int kFirst = MODE == 1 ? 4 : (MODE == 3 ? 6 : kWords);   // words before the group test
    uint32_t d0 = 0u, d1 = 0u, d2 = 0u, d3 = 0u;
#pragma unroll
    for (int w = 0; w < kFirst; ++w) {
      const uint32_t x0 = qd[w] ^ g.lo[w], x1 = qd[w] ^ g.lo[kWords + w], x2 = qd[w] ^ g.hi[w], x3 = qd[w] ^ g.hi[kWords + w];
      d0 = bcnt_acc(x0, d0); d1 = bcnt_acc(x1, d1); d2 = bcnt_acc(x2, d2); d3 = bcnt_acc(x3, d3);
    }
    uint32_t dmin = min(min(d0, d1), min(d2, d3));
    if (kFirst < kWords) {
      if (__builtin_amdgcn_ballot_w64(dmin < limit) == 0ull) return;    // lower bounds already out: skip the rest
#pragma unroll
      for (int w = kFirst; w < kWords; ++w) {
        const uint32_t x0 = qd[w] ^ g.lo[w], x1 = qd[w] ^ g.lo[kWords + w], x2 = qd[w] ^ g.hi[w], x3 = qd[w] ^ g.hi[kWords + w];
        d0 = bcnt_acc(x0, d0); d1 = bcnt_acc(x1, d1); d2 = bcnt_acc(x2, d2); d3 = bcnt_acc(x3, d3);
      }
      dmin = min(min(d0, d1), min(d2, d3));
    }
    if (__builtin_amdgcn_ballot_w64(dmin < limit) != 0ull) {
      // rows are visited in ascending order, so a later row never displaces an equal distance:
      // "key < best[K-1]" is exactly "d < worst_d" and insertion order inside the group is free.
      topk_insert<K>(best, (d0 << kLocalBits) | r);
      topk_insert<K>(best, (d1 << kLocalBits) | (r + 1));
      topk_insert<K>(best, (d2 << kLocalBits) | (r + 2));
      topk_insert<K>(best, (d3 << kLocalBits) | (r + 3));
      worst_d = best[K - 1] >> kLocalBits;
      limit = min(worst_d, foreign);
    }
    return;
  }
  // Three-stage partial-distance elimination. Stage A: 96 bits of each of the four rows (chains interleaved word by
  // word: no instruction depends on its predecessor) and one ballot per row; a row whose lower bound reaches the limit
  // in all 64 queries is finished. Stage B, per surviving row (~29 % of the rows on independent bits at radius 35):
  // the 4th word, test again; stage C (rare on independent bits, common on correlated ones): words 5-6, test; stage D: the
  // last 64 bits, test, insert.
  uint32_t d0 = 0u, d1 = 0u, d2 = 0u, d3 = 0u;
#pragma unroll
  for (int w = 0; w < 3; ++w) {
    const uint32_t x0 = qd[w] ^ g.lo[w], x1 = qd[w] ^ g.lo[kWords + w], x2 = qd[w] ^ g.hi[w], x3 = qd[w] ^ g.hi[kWords + w];
    d0 = bcnt_acc(x0, d0); d1 = bcnt_acc(x1, d1); d2 = bcnt_acc(x2, d2); d3 = bcnt_acc(x3, d3);
  }
  const unsigned long long b0 = __builtin_amdgcn_ballot_w64(d0 < limit), b1 = __builtin_amdgcn_ballot_w64(d1 < limit),
                           b2 = __builtin_amdgcn_ballot_w64(d2 < limit), b3 = __builtin_amdgcn_ballot_w64(d3 < limit);
  if ((b0 | b1 | b2 | b3) == 0ull) return;
  // rows are visited in ascending order, so a later row never displaces an equal distance:
  // "key < best[K-1]" is exactly "d < worst_d"
#define TOD_ROW_STAGES(bal_, d_, rows_, half_, idx_)                                                               \
  if ((bal_) != 0ull) {                                                                                            \
    d_ = bcnt_acc(qd[3] ^ rows_[half_ * kWords + 3], d_);                                                         \
    if (__builtin_amdgcn_ballot_w64(d_ < limit) != 0ull) {                                                         \
      d_ = bcnt_acc(qd[4] ^ rows_[half_ * kWords + 4], d_);                                                       \
      d_ = bcnt_acc(qd[5] ^ rows_[half_ * kWords + 5], d_);                                                       \
      if (__builtin_amdgcn_ballot_w64(d_ < limit) != 0ull) {                                                       \
        d_ = bcnt_acc(qd[6] ^ rows_[half_ * kWords + 6], d_);                                                     \
        d_ = bcnt_acc(qd[7] ^ rows_[half_ * kWords + 7], d_);                                                     \
        if (__builtin_amdgcn_ballot_w64(d_ < limit) != 0ull) {                                                     \
          topk_insert<K>(best, (d_ << kLocalBits) | (r + idx_));                                                  \
          worst_d = best[K - 1] >> kLocalBits;                                                                    \
          limit = min(worst_d, foreign);                                                                          \
        }                                                                                                         \
      }                                                                                                           \
    }                                                                                                             \
  }
  TOD_ROW_STAGES(b0, d0, g.lo, 0, 0u)
  TOD_ROW_STAGES(b1, d1, g.lo, 1, 1u)
  TOD_ROW_STAGES(b2, d2, g.hi, 0, 2u)
  TOD_ROW_STAGES(b3, d3, g.hi, 1, 3u)
#undef TOD_ROW_STAGES
}

// One WAVE = one work item (DB tile, group of 64 queries). Work items are numbered tile-major so the waves
// of a block share a tile (scalar-cache / L2 locality); blocks b and b+8 share an XCD, and the decode below
// gives each XCD a contiguous run of tiles.
template <int K, int MODE>
__global__ __launch_bounds__(kBlock) void hamming_topk_tiles(const uint32_t* __restrict__ db,
                                                             const uint32_t* __restrict__ q, uint32_t n_rows,
                                                             uint32_t nq, uint32_t nq_pad, uint32_t rows_per_tile,
                                                             uint32_t n_tiles, uint32_t n_qw,
                                                             uint32_t blocks_per_xcd, uint32_t tiles_per_xcd, uint32_t cut,
                                                             uint32_t* __restrict__ part, uint32_t* bound,
                                                             uint8_t* __restrict__ stored) {
  const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3;
  uint32_t tile, qw;
  if (tiles_per_xcd) {
    // every XCD owns whole DB tiles (its L2 then holds one contiguous slice of the DB, read by all its query waves)
    const uint32_t local = __builtin_amdgcn_readfirstlane(slot * kWavesPerBlock + (threadIdx.x >> 6));
    if (local >= tiles_per_xcd * n_qw) return;
    tile = xcd * tiles_per_xcd + local / n_qw; qw = local % n_qw;
  } else {
    const uint32_t vblock = xcd * blocks_per_xcd + slot;               // XCD-contiguous virtual block id
    const uint32_t item = __builtin_amdgcn_readfirstlane(vblock * kWavesPerBlock + (threadIdx.x >> 6));
    tile = item / n_qw; qw = item % n_qw;
  }
  if (tile >= n_tiles) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t qi = qw * 64u + lane;
  const uint32_t qi_ld = qi < nq ? qi : (nq - 1);

  uint32_t qd[kWords];
  {
    const uint4* qp = reinterpret_cast<const uint4*>(q + (size_t)qi_ld * kWords);
    uint4 a = qp[0], b = qp[1];
    qd[0] = a.x; qd[1] = a.y; qd[2] = a.z; qd[3] = a.w;
    qd[4] = b.x; qd[5] = b.y; qd[6] = b.z; qd[7] = b.w;
  }
  uint32_t best[K];
#pragma unroll
  for (int j = 0; j < K; ++j) best[j] = 0xFFFFFFFFu;
  uint32_t worst_d = 0xFFFFFFFFu >> kLocalBits;

  const uint32_t row0 = tile * rows_per_tile;
  const uint32_t row_end = min(n_rows, row0 + rows_per_tile);
  const uint32_t n_local = row_end > row0 ? row_end - row0 : 0u;
  const uint32_t* __restrict__ base = db + (size_t)row0 * kWords;

  // ping-pong SGPR groups: the load of group g+1 is in flight while group g is consumed
  const uint32_t n_groups = n_local / kGroupRows;
  uint32_t r = 0;
  // foreign = min(1 + smallest published k-th best distance, cut); cut = radius + 1: a row at distance > radius is
  // dropped by the radius truncation whatever its rank, so the search may drop it as well
  uint32_t foreign = cut, limit = min(worst_d, foreign);
  uint32_t* my_bound = bound + (qi < nq ? qi : nq - 1);
  if (n_groups > 0) {
    constexpr uint32_t kStride = kGroupRows * kWords;
    RowGroup ga, gb;
    issue_rows(ga, base);
    wait_rows(ga);
    uint32_t g = 0, next_share = 16;                        // first exchange early: the tile's own list is full by then
    for (; g + 2 <= n_groups; g += 2) {
      issue_rows(gb, base + (size_t)(g + 1) * kStride);
      consume_group<K, MODE>(qd, ga, r, best, worst_d, limit, foreign);
      wait_rows(gb);
      const uint32_t gn = (g + 2 < n_groups) ? g + 2 : g;      // the last pair re-reads an in-bounds group
      issue_rows(ga, base + (size_t)gn * kStride);
      consume_group<K, MODE>(qd, gb, r + kGroupRows, best, worst_d, limit, foreign);
      wait_rows(ga);
      r += 2 * kGroupRows;
      if (g >= next_share) {                                // wave-uniform
        next_share += kSharePeriod;
        // publish this tile's bound (only once its list is full), pick up the smallest bound published so far
        uint32_t seen = __hip_atomic_load(my_bound, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (worst_d < seen) { atomicMin(my_bound, worst_d); seen = worst_d; }   // publish only a real improvement
        foreign = seen == 0xFFFFFFFFu ? cut : min(cut, seen + 1u);
        limit = min(worst_d, foreign);
      }
    }
    if (g < n_groups) {                                         // odd group count: ga holds group g
      consume_group<K, MODE>(qd, ga, r, best, worst_d, limit, foreign);
      r += kGroupRows;
    }
  }
  for (; r < n_local; ++r) {
    uint32_t d = hamming256_mem(qd, base + (size_t)r * kWords);
    if (d < cut) topk_insert<K>(best, (d << kLocalBits) | r);
  }
  // A (tile, 64 queries) pair that found nothing below the limit -- the rule once a radius is set: 96 % of them on the
  // benchmark's data -- stores nothing; the merge skips it by its flag byte (0xFF from the launch's memset = nothing stored)
  if (__builtin_amdgcn_ballot_w64(qi < nq && best[0] != 0xFFFFFFFFu) != 0ull) {
    if (qi < nq) {
#pragma unroll
      for (int j = 0; j < K; ++j) part[((size_t)tile * K + j) * nq_pad + qi] = best[j];
    }
    if (lane == 0) stored[(size_t)tile * n_qw + qw] = 0;
  }
}
