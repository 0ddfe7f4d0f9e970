// The cross-check filter (todhip_cross_check_device, include/todhip.h): THE statement of its predicate -- which frame a query belongs
// to, which of a frame's query rows compete, and when one (distance, query) pair beats another. cross_check.hip's kernels evaluate
// these functions on the device; tests/cross_check_host_test.cpp includes this header into a host program. Plain C++, integers only.
//
// nq query rows are cut into frames of Q rows (the last frame may be short). Frame f owns rows f Q ... min((f + 1) Q, nq) - 1, and its
// valid queries are the first min(frame_nq[f], rows of f) of them (all of them without a frame_nq). A kept match of query q that names
// DB row g survives iff q is valid and no valid query q' of the same frame has (d(q', g), q') < (d(q, g), q) lexicographically: q is the
// nearest valid query of its frame to g, ties to the lower query index.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define TOD_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TOD_HD inline
#endif

namespace tod {

// frames of Q >= 1 rows that nq rows make (the last one may be short)
TOD_HD uint32_t cross_check_n_frames(uint32_t nq, uint32_t Q) { return nq / Q + (nq % Q ? 1u : 0u); }

// the frame of query row q
TOD_HD uint32_t cross_check_frame(uint32_t q, uint32_t Q) { return q / Q; }

// [lo, hi): the valid query rows of frame f < cross_check_n_frames(nq, Q). limited: the frame has a frame_nq entry, frame_nq_f; without
// one every row of the frame is valid. A frame_nq_f above the frame's rows counts as all of them, 0 leaves the range empty.
struct CrossCheckRange { uint32_t lo, hi; };
TOD_HD CrossCheckRange cross_check_valid(uint32_t f, uint32_t nq, uint32_t Q, bool limited, uint32_t frame_nq_f) {
  const uint64_t first = (uint64_t)f * Q;                               // < nq for a frame that exists
  if (first >= nq) return CrossCheckRange{nq, nq};
  const uint32_t lo = (uint32_t)first;
  uint32_t rows = nq - lo;
  if (rows > Q) rows = Q;
  const uint32_t valid = limited && frame_nq_f < rows ? frame_nq_f : rows;
  return CrossCheckRange{lo, lo + valid};
}

// does query q2 at distance d2 from a DB row take that row from query q at distance d? (never for q2 == q: the distances are equal)
TOD_HD bool cross_check_beats(uint32_t d2, uint32_t q2, uint32_t d, uint32_t q) { return d2 < d || (d2 == d && q2 < q); }

}  // namespace tod
