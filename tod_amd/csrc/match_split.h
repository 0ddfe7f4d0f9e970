// K4x's block-split controller (host, plain C++): which split -- after 2 or 3 of a block's 4 MFMAs, or 4 = whole blocks -- the next
// launch of hamming_topk_mfma uses (mfma_block_test_part, match_mfma.h). No reference lines: the reference has no such search.
// Included by ctx.h after include/todhip.h; todhip_ctx owns one K4xSplit beside the two buffers the reports travel through.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>

// Which split pays is a property of the DATA (independent bits: 2; this library's ORB descriptors of rendered views: 3, since nearly
// every block survives 128 positions there and the 2-split then costs +30 %), so the launch adapts: a split launch counts the blocks
// that went on to their second part, the merge kernel behind it leaves the totals in pinned memory, and the controller moves one
// level up (2 -> 3 -> whole blocks) when more than a quarter of the blocks went on, and probes one level down every hold_len
// launches (32, doubling to 256 while the probes keep failing). `force` (todhip_set_matcher_block_split), else the process's
// default (TODHIP_K4X_HALF): < 0 adaptive, 0 never, 2 / 3 always that split (1 = 2).
// "Went on" at split 2 over the fp4 copy is judged at the LAUNCH's radius, not at each query's tightened threshold: the paired step
// (fp4rows_pair_step, match_fp4rows.h) tests two blocks at once against one bias per launch. The count can only be higher than the
// single-block step's, and it is what that step pays for: every such block runs the slow path.
struct K4xSplit {
  int force = -1;
  uint32_t seq_sent = 0, seq_seen = 0;   // split launches sent; the last report looked at
  uint32_t split = 2, hold = 0, hold_len = 32;   // level in use; launches left before the next probe; the hold after that probe
  uint32_t last[4] = {0, 0, 0, 0};       // the cumulative counts already accounted for

  // the data the launches see has changed (todhip_db_select_objects): start over at the lowest level. The report counters stay: the
  // device's totals are cumulative.
  void restart() { split = 2; hold = 0; hold_len = 32; }

  int mode(int process_default) const { return force >= 0 ? force : process_default; }
  // false: whole blocks, and neither method below is needed. min_split: the lowest split the thresholds allow (4: none)
  bool may_split(uint32_t min_split, int process_default) const { return mode(process_default) != 0 && min_split != 4u; }

  // hs: [0..1] split 2: blocks that went on, blocks; [2..3] split 3; [4] launches reported -- written by the merge kernel
  void take_report(const volatile uint32_t* hs, todhip_counters& counters, uint32_t min_split, int process_default, bool debug) {
    if (split < min_split) split = min_split;
    const uint32_t seq_now = hs[4];
    if (seq_now == seq_seen) return;                       // no split launch has reported since the last look
    seq_seen = seq_now;
    for (uint32_t m = 2; m <= 3; ++m) {
      const uint32_t pass = hs[2 * (m - 2)] - last[2 * (m - 2)], blocks = hs[2 * (m - 2) + 1] - last[2 * (m - 2) + 1];
      if (!blocks) continue;
      last[2 * (m - 2)] += pass; last[2 * (m - 2) + 1] += blocks;
      counters.k4x_half_blocks += blocks; counters.k4x_half_blocks_completed += pass;
      const bool pays = (uint64_t)pass * 4u <= blocks;     // (measured on the rendered-view DB: 48 % going on at split 3 = 2.71 ms, whole blocks 2.60)
      if (debug) fprintf(stderr, "[todhip] K4x blocks split after %u MFMAs: %u of %u went on (%.3f)%s, split in use %u\n", m, pass, blocks,
                         (double)pass / blocks, pays ? "" : ": does not pay", split);
      if (mode(process_default) >= 0) continue;            // a forced split only reports
      if (m == split && !pays) {                           // the level in use stopped paying: one level up
        split = m + 1; hold = hold_len = 32;
      } else if (m + 1 == split) {                         // a probe's report
        if (pays) { split = m; hold_len = 32; }
        else hold_len = std::min(256u, hold_len * 2u);
      }
    }
  }

  // the split of this launch; an adaptive level above min_split counts its hold down and then probes one level down once
  uint32_t next(uint32_t min_split, int process_default) {
    const int md = mode(process_default);
    if (!may_split(min_split, process_default)) return 4u;
    if (md >= 0) return std::max<uint32_t>(min_split, md == 1 ? 2u : (uint32_t)std::min(md, 3));
    if (split > min_split) {
      if (hold == 0) { hold = hold_len ? hold_len : 32; return split - 1u; }
      --hold;
    }
    return split;
  }
};
