// The float matcher's launch plan (host, plain C++, no HIP include; included by l2.hip; tested stand-alone by
// tests/l2_plan_host_test.cpp): the constants the kernels and the host share, the tuning and diagnostics knobs, and L2Plan -- the
// geometry of the DB pass, what the seed pass does and the size of every workspace buffer, from a call's numbers alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

constexpr uint32_t kDim = 128;                            // floats per row of the wider of the two float DBs (desc_bytes 512)
constexpr uint32_t kDimNarrow = 64;                       // ... and of the narrower (desc_bytes 256: SURF, KAZE); DESIGN 6p
constexpr uint32_t kTileRows = 32;                        // DB rows of one MFMA A tile (8 KB of bf16)
// what of the DB pass depends on the width, each stated once: k-steps of 16 dimensions per tile (one 1 KB wave-load and one MFMA per
// query tile each), loads per tile (the k-steps' and the norms': what a hand-counted vmcnt counts in), a wave's ring slot in LDS (one
// tile's fragments + its 32 norms, twice)
constexpr uint32_t l2_k_steps(uint32_t dim) { return dim / 16u; }
constexpr uint32_t l2_tile_loads(uint32_t dim) { return l2_k_steps(dim) + 1u; }
constexpr uint32_t l2_ring_slot_bytes(uint32_t dim) { return kTileRows * dim * 2u + 256u; }
constexpr uint32_t kRingSlotBytes = l2_ring_slot_bytes(kDim);
// floats per row of a DB of desc_bytes bytes a row; 0: not a float DB
constexpr uint32_t l2_dim_of(uint32_t desc_bytes) { return desc_bytes == kDim * 4u ? kDim : desc_bytes == kDimNarrow * 4u ? kDimNarrow : 0u; }
constexpr uint32_t kQTilesPerWave = 4;
constexpr uint32_t kWaves = 4;
constexpr uint32_t kBlockQueries = kWaves * kQTilesPerWave * 32u;   // 512
constexpr uint32_t kTop = 8;                              // per-lane list length of pass 1 (k <= 8)
constexpr uint32_t kSlot = 8;                             // candidate rows a (query, chunk, lane half) keeps in its private slot
constexpr uint32_t kCandCap = 1024;                       // shared list per query for what the slots cannot hold; beyond it the exact scan
constexpr uint32_t kListCap = 2048;                       // candidates per query all told (pass 3's list in LDS); beyond it the exact scan
constexpr uint32_t kL2MaxPerQuery = 1024;                 // the radius search's max_per_query; the lower half of LS's buffer
constexpr uint32_t kL2SortKeys = 2u * kL2MaxPerQuery;     // keys LR and LS sort in LDS (16 KB); LR holds at most kListCap candidates

// The environment's tuning knobs (0: unset) and diagnostics switches (tools/README.md), read once by l2.hip
struct L2Knobs {
  uint32_t chunk_rounds = 0;       // TODHIP_L2_CHUNK_ROUNDS: rounds of blocks in the DB pass instead of one
  uint32_t sample_tiles = 0;       // TODHIP_L2_SAMPLE_TILES: tiles of the one-GEMM path's sample
  uint32_t seed_chunks = 0;        // TODHIP_L2_SEED_CHUNKS: chunks of the one-GEMM path's seed pass
  bool no_candidates = false;      // TODHIP_L2_NO_CANDIDATES: a threshold below every score, so that pass 2 runs its GEMM and finds nothing
  bool trace = false;              // TODHIP_L2_TRACE: pass 2 leaves (start, end) of every wave in the partition buffer (l2_trace.h)
  bool exact_scan = false;         // TODHIP_L2_EXACT_SCAN: skip the GEMM filter
};

inline uint32_t l2_pad_rows(uint32_t n_rows) { return ((n_rows + kTileRows - 1u) / kTileRows) * kTileRows; }

struct L2Plan {
  // the DB pass: grid (n_chunks, q_blocks), a block = 512 queries x tiles_per_chunk DB tiles, two partitions (lane halves) per chunk
  uint32_t nq_pad, q_blocks, n_tiles, n_chunks, tiles_per_chunk, n_parts;
  // pass 0: the k-th smallest score over a sample of the DB bounds A_k from above.
  //  * one-GEMM path (fast: DBs of >= 64k rows): the sample is every (n_tiles / sample)-th tile, a quarter of the DB at most
  //    2048 tiles, so it is representative whatever the object order; seed + 2 eps IS the candidate threshold of pass 2 --
  //    a superset of what the exact A_k would admit (rows of rank <= ~k N / n_sample plus the eps band) -- and the pass
  //    that computes A_k over the whole DB is skipped. Its seed needs no exact k-th smallest of the sample: the k-th smallest of
  //    the partitions' minima bounds A_k just as well and costs the GEMM's epilogue one instruction (kt0 = 1; needs k partitions
  //    with a real row: 2 s_used >= 512 here)
  //  * classic path (smaller DBs): the sample is the first rows and the seed only limits what enters pass 1's lists.
  bool seed_pass, fast;
  uint32_t sample_tiles, sample_stride, s_chunks, s_tpc, s_used;   // the last three: 0 without a seed pass
  uint32_t kt0, kt1, k_eff;        // l2_gemm_kernel's KT in pass 0 and pass 1; k, or the row count of a smaller DB
  float margin;                    // candidates = scores <= A_k + margin * eps
  bool one_gemm() const { return seed_pass && fast; }
  // bytes of the workspace buffers (L2Ws, l2.hip)
  size_t keys_bytes, cand_cnt_bytes, flags_bytes, q_bf16_bytes, q_eps_bytes, q_norm_bytes, thr_bytes, seed_bytes, scan_marks_bytes,
      cand_bytes, slots_bytes, slot_cnt_bytes, part_bytes;
};

// k: the list length per query (the radius search passes max_per_query; it uses the DB pass's geometry and the sizes, not the seed pass)
// dim: floats per row, kDim or kDimNarrow. The geometry does not depend on it (a wave is 4 query tiles at either width); the queries'
// bf16 image does
inline L2Plan l2_plan(uint32_t n_rows, uint32_t nq, uint32_t k, uint32_t n_cu, const L2Knobs& knobs, uint32_t dim = kDim) {
  L2Plan P{};
  P.nq_pad = ((nq + kBlockQueries - 1u) / kBlockQueries) * kBlockQueries;
  P.q_blocks = P.nq_pad / kBlockQueries;
  P.n_tiles = l2_pad_rows(n_rows) / kTileRows;
  // 2 blocks per CU in flight; the DB is cut into as many chunks as that allows for this many query blocks
  P.n_chunks = std::max(1u, (std::max(knobs.chunk_rounds, 1u) * 2u * n_cu) / P.q_blocks);
  P.n_chunks = std::min(P.n_chunks, std::max(1u, P.n_tiles));
  P.tiles_per_chunk = (P.n_tiles + P.n_chunks - 1u) / P.n_chunks;
  P.n_chunks = (P.n_tiles + P.tiles_per_chunk - 1u) / P.tiles_per_chunk;
  P.n_parts = 2u * P.n_chunks;
  P.k_eff = std::min(k, std::max(1u, n_rows));
  P.kt1 = P.k_eff <= 4u ? 4u : 8u;
  P.fast = P.n_tiles >= 2048u;
  P.sample_tiles = P.fast ? std::min(knobs.sample_tiles ? knobs.sample_tiles : 2048u, P.n_tiles / 4u) : std::min(P.n_tiles, 256u);
  P.sample_stride = P.fast ? P.n_tiles / P.sample_tiles : 1u;
  P.margin = knobs.no_candidates ? -1e30f : 2.f;
  P.seed_pass = (P.fast || P.n_tiles >= 8u * P.sample_tiles) && P.sample_tiles * kTileRows >= P.k_eff;
  P.kt0 = P.fast ? 1u : P.kt1;
  if (P.seed_pass) {
    P.s_chunks = std::min(P.sample_tiles, P.fast ? (knobs.seed_chunks ? std::min(knobs.seed_chunks, P.n_chunks) : P.n_chunks) : 32u);
    P.s_tpc = (P.sample_tiles + P.s_chunks - 1u) / P.s_chunks;
    P.s_used = (P.sample_tiles + P.s_tpc - 1u) / P.s_tpc;
  }
  P.keys_bytes = (size_t)nq * k * 8;
  // a word per padded query; the counters among them: l2_prepare_kernel zeroes one for every row < nq_pad
  P.cand_cnt_bytes = P.flags_bytes = P.q_eps_bytes = P.q_norm_bytes = P.thr_bytes = P.seed_bytes = P.scan_marks_bytes = (size_t)P.nq_pad * 4;
  P.q_bf16_bytes = (size_t)P.nq_pad * dim * 2;
  P.cand_bytes = (size_t)P.nq_pad * kCandCap * 4;
  P.slots_bytes = (size_t)P.nq_pad * P.n_parts * kSlot * 4;        // 2 x 512 partitions x 8 rows x 4 B x 512 queries per query block: 16 MB whatever nq
  P.slot_cnt_bytes = (size_t)P.nq_pad * P.n_parts * 4;
  P.part_bytes = (size_t)std::max(P.n_parts, 64u) * P.nq_pad * kTop * 4;   // the seed pass writes up to 2 x 32 partitions
  return P;
}
