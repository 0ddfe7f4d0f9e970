// The plain C++ of fast_nms_kernel's pass 2 and of its survivor list (tod_amd/csrc/orb_arc.h) against their definitions (host, no GPU):
//   fast_score_pairs, the score from one sliding minimum and one sliding maximum over 16-bit pairs (ring elements i and i + 8 in one
//     word), against the score's definition arc by arc: for each of the 16 arcs of 9 contiguous ring pixels the minimum of
//     ring - p and the minimum of p - ring, the largest of the 32, 0 unless above the threshold. Rings: every centre 0..255 with
//     ring pixels around both thresholds and at 0 and 255 (arcs of exactly 8, 9 and 16 pixels among them), all-equal rings, the
//     extremes (p = 0 with ring 255 and the reverse: differences of +-255), and 10^6 seeded random rings, half of them near p;
//   nms_entry / nms_entry_px / nms_entry_py on every scored position of a 66 x 18 tile: the round trip, the entries of a group of
//     four as the first one's + i (how pass 1 appends them), all entries different and inside 16 bits.
// Prints "<rings compared> <entries compared>"; exits 1 at the first difference.
#include <cstdint>
#include <cstdio>
#include <set>

#include "orb_arc.h"

using namespace tod_orb;

static uint32_t rng_state = 0x2545F491u;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

static long n_rings = 0, n_entries = 0;

// the definition
static int score_by_arcs(int p, const int (&ring)[16]) {
  int best = 0;
  for (int a = 0; a < 16; ++a) {
    int lo = 1 << 30, lo_neg = 1 << 30;
    for (int k = 0; k < 9; ++k) {
      const int d = ring[(a + k) & 15] - p;
      if (d < lo) lo = d;
      if (-d < lo_neg) lo_neg = -d;
    }
    if (lo > best) best = lo;
    if (lo_neg > best) best = lo_neg;
  }
  return best > kFastThr ? best : 0;
}

static bool check_ring(int p, const int (&ring)[16]) {
  pair16 d[8];
  const uint32_t pp = (uint32_t)p * 0x00010001u;
  for (int i = 0; i < 8; ++i) d[i] = pk_diff((uint32_t)ring[i], (uint32_t)ring[i + 8], pp);
  const int got = fast_score_pairs(d), want = score_by_arcs(p, ring);
  ++n_rings;
  if (got != want) {
    std::printf("fast_score_pairs: p %d ring", p);
    for (int i = 0; i < 16; ++i) std::printf(" %d", ring[i]);
    std::printf(": %d, by arcs %d\n", got, want);
    return false;
  }
  return true;
}

static int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

static bool check_scores() {
  int ring[16];
  for (int p = 0; p < 256; ++p) {
    // arcs of n bright (then dark) pixels at p +- t starting at every ring position, the rest at p; t around the threshold
    for (int n = 7; n <= 16; ++n)
      for (int start = 0; start < 16; ++start)
        for (int t : {19, 20, 21, 22, 60, 255})
          for (int sign : {1, -1}) {
            for (int i = 0; i < 16; ++i) ring[i] = p;
            for (int k = 0; k < n; ++k) ring[(start + k) & 15] = clamp255(p + sign * (t + (int)(rnd() % 3u)));
            if (!check_ring(p, ring)) return false;
          }
    for (int v : {0, p, 255}) {
      for (int i = 0; i < 16; ++i) ring[i] = v;
      if (!check_ring(p, ring)) return false;
    }
  }
  for (int n = 0; n < 1000000; ++n) {
    const int p = (int)(rnd() & 255u);
    for (int i = 0; i < 16; ++i) ring[i] = (n & 1) ? clamp255(p + (int)(rnd() % 81u) - 40) : (int)(rnd() & 255u);
    if (!check_ring(p, ring)) return false;
  }
  return true;
}

static bool check_entries() {
  constexpr int kScoreW = 66, kScoreH = 18, kGroups = 17;
  std::set<uint32_t> seen;
  for (int py = 0; py < kScoreH; ++py)
    for (int g = 0; g < kGroups; ++g) {
      const uint32_t first = nms_entry(4 * g, py);
      for (int i = 0; i < 4 && 4 * g + i < kScoreW; ++i, ++n_entries) {
        const uint32_t e = first + (uint32_t)i;
        if (e != nms_entry(4 * g + i, py) || nms_entry_px(e) != 4 * g + i || nms_entry_py(e) != py || e > 0xFFFFu || !seen.insert(e).second) {
          std::printf("nms_entry: row %d group %d position %d: entry %u -> (%d, %d)\n", py, g, i, e, nms_entry_px(e), nms_entry_py(e));
          return false;
        }
      }
    }
  return true;
}

int main() {
  if (!check_scores() || !check_entries()) return 1;
  std::printf("%ld %ld\n", n_rings, n_entries);
  return 0;
}
