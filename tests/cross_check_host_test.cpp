// Stand-alone host program over tod_amd/csrc/cross_check.h (built with -fsanitize=address,undefined by tests/test_cross_check_cpu.py):
// the frame of a query, a frame's valid range under frame_nq and the short last frame, and the lexicographic tie rule. Prints one line
// per check group and "ok"; any failed check prints what failed and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cross_check.h"

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

// the ranges of every frame of (nq, Q, frame_nq) against the definition written out with loops over the rows
static void check_ranges(uint32_t nq, uint32_t Q, const std::vector<uint32_t>* frame_nq) {
  const uint32_t n_frames = tod::cross_check_n_frames(nq, Q);
  CHECK(n_frames == (nq + Q - 1) / Q);
  CHECK(!frame_nq || frame_nq->size() == n_frames);
  std::vector<int> valid(nq, 0);
  for (uint32_t f = 0; f < n_frames; ++f) {
    const tod::CrossCheckRange r = tod::cross_check_valid(f, nq, Q, frame_nq != nullptr, frame_nq ? (*frame_nq)[f] : 0u);
    CHECK(r.lo == f * Q && r.lo <= r.hi && r.hi <= nq && r.hi - r.lo <= Q);
    for (uint32_t q = r.lo; q < r.hi; ++q) valid[q] += 1;
  }
  for (uint32_t q = 0; q < nq; ++q) {
    const uint32_t f = tod::cross_check_frame(q, Q);
    CHECK(f == q / Q && f < n_frames);
    const uint32_t in_frame = q - f * Q;                                // the row's position in its frame
    const bool want = !frame_nq || in_frame < (*frame_nq)[f];
    CHECK(valid[q] == (want ? 1 : 0));
  }
  std::printf("ranges nq=%u Q=%u frame_nq=%s\n", nq, Q, frame_nq ? "given" : "null");
}

int main() {
  // Q = 1, nq < Q, nq = Q, nq = Q + 1, several frames with a short last one; frame_nq NULL
  const uint32_t shapes[][2] = {{1, 1}, {5, 1}, {3, 7}, {7, 7}, {8, 7}, {70, 33}, {99, 33}, {64, 64}, {65, 64}};
  for (const auto& s : shapes) check_ranges(s[0], s[1], nullptr);
  // frame_nq of 0, larger than the frame, larger than the short last frame, exact
  { std::vector<uint32_t> n = {33, 0, 7};        check_ranges(99, 33, &n); }
  { std::vector<uint32_t> n = {40, 33, 100};     check_ranges(70, 33, &n); }
  { std::vector<uint32_t> n = {0xFFFFFFFFu, 0, 5}; check_ranges(70, 33, &n); }
  { std::vector<uint32_t> n = {0};               check_ranges(7, 7, &n); }
  { std::vector<uint32_t> n = {9};               check_ranges(3, 7, &n); }
  { std::vector<uint32_t> n = {1, 0, 1, 0, 2};   check_ranges(5, 1, &n); }
  // the largest sizes: no 32-bit wrap in f * Q
  {
    const uint32_t nq = 0xFFFFFFF0u, Q = 0x80000000u;
    CHECK(tod::cross_check_n_frames(nq, Q) == 2u);
    const tod::CrossCheckRange a = tod::cross_check_valid(0, nq, Q, false, 0), b = tod::cross_check_valid(1, nq, Q, true, 0xFFFFFFFFu);
    CHECK(a.lo == 0u && a.hi == Q && b.lo == Q && b.hi == nq);
    const tod::CrossCheckRange c = tod::cross_check_valid(2, nq, Q, false, 0);       // a frame that does not exist: empty
    CHECK(c.lo == c.hi);
  }
  // the tie rule: (d2, q2) < (d, q) lexicographically, never a query against itself
  for (uint32_t d2 = 0; d2 < 4; ++d2)
    for (uint32_t q2 = 0; q2 < 4; ++q2)
      for (uint32_t d = 0; d < 4; ++d)
        for (uint32_t q = 0; q < 4; ++q) {
          const bool want = d2 < d || (d2 == d && q2 < q);
          CHECK(tod::cross_check_beats(d2, q2, d, q) == want);
          CHECK(!(tod::cross_check_beats(d2, q2, d, q) && tod::cross_check_beats(d, q, d2, q2)));                     // antisymmetric
          if (d2 != d || q2 != q) CHECK(tod::cross_check_beats(d2, q2, d, q) || tod::cross_check_beats(d, q, d2, q2)); // total
        }
  CHECK(!tod::cross_check_beats(5, 9, 5, 9));
  CHECK(tod::cross_check_beats(5, 8, 5, 9) && !tod::cross_check_beats(5, 9, 5, 8));
  CHECK(tod::cross_check_beats(512, 0, 0xFFFFFFFFu, 0) && !tod::cross_check_beats(6, 0, 5, 0xFFFFFFFFu));
  std::printf("ties\n");
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
