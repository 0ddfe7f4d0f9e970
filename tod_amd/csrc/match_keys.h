// What both matcher engines and the merges share: the launch constants, the per-lane sorted list of partial keys (distance << 22 |
// tile-local row; the merges widen them to distance << 32 | global row, the order (distance asc, global row asc) of decision D1) and
// the pick over ascending lists of global keys, and the store of one kept match (object lookup, row_ops.h, and 3D gather,
// DescriptorMatcher.cpp:231-244). Included by match.hip, match_radius.hip and match_wide.hip inside their anonymous namespaces, after ctx.h and row_ops.h.

constexpr int kWords = 8;          // 256-bit descriptors (ORB / rBRIEF), 32 bytes per row
constexpr int kGroupRows = 4;      // DB rows per SGPR group (two s_load_dwordx16)
constexpr int kLocalBits = 22;     // tile-local row index bits in a partial key (tile <= 4M rows)
constexpr uint32_t kLocalMask = (1u << kLocalBits) - 1u;
constexpr uint32_t kNoLimit = 0xFFFFFFFFu >> kLocalBits;   // 1023: the distance field of the empty key, above every distance
constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / 64;
constexpr int kWavesPerCU = 24;    // waves a CU holds at once: 6 blocks of 4 waves (<= 112 SGPRs); the grid is ~3x that
constexpr uint32_t kSharePeriod = 128;   // groups between two exchanges of the per-query distance bound
constexpr int kMergeGroups = 16;   // stage-1 merge fan-in

template <int K>
__device__ __forceinline__ void topk_insert(uint32_t (&best)[K], uint32_t key) {
  // branch-free sorted insertion: key falls through the list, each slot keeps the smaller one
#pragma unroll
  for (int j = 0; j < K; ++j) {
    uint32_t lo = min(best[j], key);
    key = max(best[j], key);
    best[j] = lo;
  }
}

// The work-item decode (xcd, slot) -> (tile, query wave) stands inline, three times the same, at the head of hamming_topk_tiles,
// hamming_topk_mfma and hamming_topk_fp4rows (the commented copy is hamming_topk_tiles'). As a __forceinline__ function returning
// "this wave has an item" it changed the generated code of every form of all three (the early return becomes a flag that hipcc
// branches on: another block layout in front of the loops, other register numbers behind it; K4's forms differ by two swapped scalar
// moves only) -- in four spellings of the function, with and without branch hints -- and these kernels are tuned to the code they have.

// The smallest key of query qi over n_lists ascending lists (layout [list][nq][k]) that is greater than the last one taken (any,
// while !have_last); ~0 when nothing is left. Keys are unique (the row is part of the key), so each list's candidate is its first
// key greater than `last`.
__device__ __forceinline__ uint64_t next_key_over_lists(const uint64_t* __restrict__ lists, uint32_t n_lists, uint32_t nq, uint32_t qi,
                                                        uint32_t k, uint64_t last, bool have_last) {
  uint64_t nxt = ~0ull;
  for (uint32_t s = 0; s < n_lists; ++s) {
    const uint64_t* lst = lists + ((size_t)s * nq + qi) * k;
    for (uint32_t i = 0; i < k; ++i) {
      uint64_t v = lst[i];
      if (have_last && v <= last) continue;
      if (v < nxt) nxt = v;
      break;
    }
  }
  return nxt;
}

// One kept match into output slot `slot`: the global row becomes (imgIdx, trainIdx) through the object prefix sums (object_of_row)
// and brings its model point (DescriptorMatcher.cpp:231-244). What K4f and the radius search's finalize both end in.
__device__ __forceinline__ void store_match(uint32_t qi, uint32_t d, uint32_t row, size_t slot, const uint32_t* __restrict__ obj_off,
                                            uint32_t n_objs, const float* __restrict__ pts, todhip_dmatch* __restrict__ matches,
                                            float* __restrict__ xyz) {
  const uint32_t lo = object_of_row(obj_off, n_objs, row);
  todhip_dmatch m;
  m.queryIdx = (int32_t)qi;
  m.trainIdx = (int32_t)(row - obj_off[lo]);
  m.imgIdx = (int32_t)lo;
  m.distance = (float)d;
  matches[slot] = m;
  float* o = xyz + slot * 3;
  o[0] = pts[(size_t)row * 3 + 0];
  o[1] = pts[(size_t)row * 3 + 1];
  o[2] = pts[(size_t)row * 3 + 2];
}
