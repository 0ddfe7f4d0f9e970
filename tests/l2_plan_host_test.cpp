// l2_plan (tod_amd/csrc/l2_plan.h) against the expressions it replaced, restated here as they stood in tod_l2_db_prepare (n_pad),
// l2_pass_begin (the DB pass's geometry, seven reserves) and l2_keys (the seed pass, the part reserve, the keys reserve): every field,
// the byte sizes included, over DB sizes that cross the 32-row tile, the 256-tile sample, the 8 x sample condition and the 2048-tile
// switch, query counts around the 512-query block, k = 1..8, four CU counts, the knobs unset and each tuning knob alone.
// Where one old buffer became two, the two sizes are held against the old one: eps and norms were q_eps, threshold and seed (the
// radius search: its marks) were thr, counters and flags were cand_cnt, which was sized from nq and is now sized from nq_pad -- the
// counters must cover the nq_pad words l2_prepare_kernel zeroes, and the two together may not need more than before.
// Invariants of every plan: the chunks cover the tiles and none is empty, the sample lies inside the DB, the seed pass's chunks cover
// the sample and none is empty. Prints the number of cases; exits 1 at the first difference.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "l2_plan.h"

struct Old {
  uint32_t nq_pad, q_blocks, n_tiles, n_chunks, tiles_per_chunk, n_parts;
  bool seed_pass, fast;
  uint32_t sample_tiles, sample_stride, s_chunks, s_tpc, s_used, kt0, kt1, k_eff;
  float margin;
  size_t cand_cnt, q_bf16, q_eps, thr, cand, slots, slot_cnt, part, keys;
};

static Old old_plan(uint32_t n, uint32_t nq, uint32_t k, uint32_t ctx_n_cu, uint32_t env_cm, uint32_t env_st, uint32_t env_sc,
                    bool no_candidates) {
  Old o{};
  // tod_l2_db_prepare
  const uint32_t ws_n_pad = ((n + kTileRows - 1u) / kTileRows) * kTileRows;
  // l2_pass_begin
  const uint32_t nq_pad = ((nq + kBlockQueries - 1u) / kBlockQueries) * kBlockQueries;
  const uint32_t q_blocks = nq_pad / kBlockQueries;
  const uint32_t n_tiles = ws_n_pad / kTileRows;
  uint32_t n_chunks = std::max(1u, (std::max(env_cm, 1u) * 2u * (uint32_t)ctx_n_cu) / q_blocks);
  n_chunks = std::min(n_chunks, std::max(1u, n_tiles));
  const uint32_t tiles_per_chunk = (n_tiles + n_chunks - 1u) / n_chunks;
  n_chunks = (n_tiles + tiles_per_chunk - 1u) / tiles_per_chunk;
  const uint32_t n_parts = 2u * n_chunks;
  o.cand_cnt = ((size_t)nq + kBlockQueries) * 4 * 2;
  o.q_bf16 = (size_t)nq_pad * kDim * 2;
  o.q_eps = (size_t)nq_pad * 4 * 2;
  o.thr = (size_t)nq_pad * 4 * 2;
  o.cand = (size_t)nq_pad * kCandCap * 4;
  o.slots = (size_t)nq_pad * n_parts * kSlot * 4;
  o.slot_cnt = (size_t)nq_pad * n_parts * 4;
  // l2_keys
  o.keys = (size_t)nq * k * 8;
  o.part = (size_t)std::max(n_parts, 64u) * nq_pad * kTop * 4;
  const uint32_t k_eff = std::min(k, std::max(1u, n));
  o.kt1 = k_eff <= 4u ? 4u : 8u;                            // auto gemm1 = k_eff <= 4u ? l2_gemm_kernel<1, 4> : l2_gemm_kernel<1, 8>;
  const bool fast = n_tiles >= 2048u;
  const uint32_t sample_tiles = fast ? std::min(env_st ? env_st : 2048u, n_tiles / 4u) : std::min(n_tiles, 256u);
  const uint32_t sample_stride = fast ? n_tiles / sample_tiles : 1u;
  const float margin = no_candidates ? -1e30f : 2.f;
  if ((fast || n_tiles >= 8u * sample_tiles) && sample_tiles * kTileRows >= k_eff) {
    const uint32_t s_chunks = std::min(sample_tiles, fast ? (env_sc ? std::min(env_sc, n_chunks) : n_chunks) : 32u), s_tpc = (sample_tiles + s_chunks - 1u) / s_chunks;
    const uint32_t s_used = (sample_tiles + s_tpc - 1u) / s_tpc;
    o.seed_pass = true; o.s_chunks = s_chunks; o.s_tpc = s_tpc; o.s_used = s_used;
  }
  o.kt0 = fast ? 1u : o.kt1;                                // auto gemm0 = fast ? l2_gemm_kernel<1, 1> : gemm1;
  o.nq_pad = nq_pad; o.q_blocks = q_blocks; o.n_tiles = n_tiles; o.n_chunks = n_chunks; o.tiles_per_chunk = tiles_per_chunk; o.n_parts = n_parts;
  o.fast = fast; o.sample_tiles = sample_tiles; o.sample_stride = sample_stride; o.k_eff = k_eff; o.margin = margin;
  return o;
}

#define CHECK(cond)                                                                                                             \
  do {                                                                                                                          \
    if (!(cond)) {                                                                                                              \
      std::fprintf(stderr, "n_rows %u nq %u k %u n_cu %u knobs %u/%u/%u/%d: %s\n", n, nq, k, n_cu, kn.chunk_rounds, kn.sample_tiles, \
                   kn.seed_chunks, (int)kn.no_candidates, #cond);                                                               \
      return 1;                                                                                                                 \
    }                                                                                                                           \
  } while (0)

int main() {
  const uint32_t tile_sample = 256u * 32u;
  const uint32_t rows[] = {1, 2, 31, 32, 33, 255u * 32u, tile_sample, tile_sample + 1u, 8u * tile_sample - 1u, 8u * tile_sample, 65504, 65505,
                           65535, 65536, 65537, 70000, 500000, 1u << 24};
  const uint32_t nqs[] = {1, 511, 512, 513, 1000, 16000};
  const uint32_t cus[] = {1, 64, 256, 304};
  L2Knobs knob_sets[6];
  knob_sets[1].chunk_rounds = 3; knob_sets[2].sample_tiles = 512; knob_sets[3].seed_chunks = 7; knob_sets[4].seed_chunks = 1000000;
  knob_sets[5].no_candidates = true;
  unsigned long cases = 0;
  for (uint32_t n : rows) for (uint32_t nq : nqs) for (uint32_t k = 1; k <= 8; ++k) for (uint32_t n_cu : cus) for (const L2Knobs& kn : knob_sets) {
    const L2Plan P = l2_plan(n, nq, k, n_cu, kn);
    const Old o = old_plan(n, nq, k, n_cu, kn.chunk_rounds, kn.sample_tiles, kn.seed_chunks, kn.no_candidates);
    CHECK(P.nq_pad == o.nq_pad && P.q_blocks == o.q_blocks && P.n_tiles == o.n_tiles && P.n_chunks == o.n_chunks);
    CHECK(P.tiles_per_chunk == o.tiles_per_chunk && P.n_parts == o.n_parts);
    CHECK(P.seed_pass == o.seed_pass && P.fast == o.fast && P.one_gemm() == (o.seed_pass && o.fast));
    CHECK(P.sample_tiles == o.sample_tiles && P.sample_stride == o.sample_stride);
    CHECK(P.s_chunks == o.s_chunks && P.s_tpc == o.s_tpc && P.s_used == o.s_used);
    CHECK(P.kt0 == o.kt0 && P.kt1 == o.kt1 && P.k_eff == o.k_eff && P.margin == o.margin);
    CHECK(P.keys_bytes == o.keys && P.q_bf16_bytes == o.q_bf16 && P.cand_bytes == o.cand && P.slots_bytes == o.slots);
    CHECK(P.slot_cnt_bytes == o.slot_cnt && P.part_bytes == o.part);
    CHECK(P.q_eps_bytes + P.q_norm_bytes == o.q_eps && P.q_eps_bytes == P.q_norm_bytes);
    CHECK(P.thr_bytes + P.seed_bytes == o.thr && P.thr_bytes == P.seed_bytes && P.scan_marks_bytes == P.seed_bytes);
    CHECK(P.cand_cnt_bytes >= (size_t)P.nq_pad * 4 && P.flags_bytes >= (size_t)nq * 4 && P.cand_cnt_bytes + P.flags_bytes <= o.cand_cnt);
    CHECK(P.nq_pad >= nq && P.nq_pad % kBlockQueries == 0 && (size_t)P.n_tiles * kTileRows >= n);
    CHECK((uint64_t)P.n_chunks * P.tiles_per_chunk >= P.n_tiles);
    CHECK(P.n_chunks >= 1 && (uint64_t)(P.n_chunks - 1u) * P.tiles_per_chunk < P.n_tiles);          // the last chunk is not empty
    if (P.seed_pass) {
      CHECK(P.sample_tiles >= 1 && P.sample_stride >= 1 && (uint64_t)P.sample_stride * P.sample_tiles <= P.n_tiles);
      CHECK(P.s_used >= 1 && P.s_used <= P.s_chunks && (uint64_t)P.s_used * P.s_tpc >= P.sample_tiles);
      CHECK((uint64_t)(P.s_used - 1u) * P.s_tpc < P.sample_tiles);
      CHECK((size_t)2u * P.s_used * P.nq_pad * kTop * 4 <= P.part_bytes);                          // the seed pass's partitions fit
    }
    ++cases;
  }
  std::printf("%lu\n", cases);
  return 0;
}
