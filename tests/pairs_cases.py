"""Constructed DBs and queries for the paired split-2 step of hamming_topk_fp4rows (tests/test_match_pairs_gpu.py and its child
tests/pairs_child.py). No GPU here. Tilings, the positions of the first part and the CPU's count of blocks: tests/fastpath_cases.py.

Query blocks 2p and 2p + 1 of a wave share an accumulator: register i of lane c + 32 h holds row (i & 3) + 8 (i >> 2) + 4 h of the step
against query c of block 2p (field A) and against query c of block 2p + 1 (field B). A plant is a row whose distance to its query over
the first part (the positions of the first two MFMAs) is exactly `radius` (the block must go on) or exactly `radius + 1` (it must
not), in the first block of a pair, in the second, or in both; the query with the same c in the partner block is then rewritten so that
the row's first part equals it (dot +128) or is its complement (dot -128): a carry or a borrow between the fields would flip the
plant's flag."""
import numpy as np

import fastpath_cases as FC

FIRST = FC.PART_WORDS[2]
REST = tuple(w for w in range(8) if w not in FIRST)
RADII = (1, 35, 63)                                            # the API rejects radius 0 (TODHIP_EINVAL); 63: cut 64, thrp = 0, the edge


def nq_of(qt):
    return 32 * qt * (4 if qt == 6 else 5) + 5                 # four / five whole query waves and a ragged one


def flip_first_part(words, n, rng):
    """n of the 128 first-part bit positions of a row (8 uint32 words) flipped"""
    for b in rng.choice(128, n, replace=False):
        words[FIRST[b >> 5]] ^= np.uint32(1 << (b & 31))


def make(n_rows, qt, radius, seed, within):
    """Independent random bits plus plants. within: the plants at distance `radius` equal their query on the rest of the row as well
    (they are answers, at exactly the radius; those at radius + 1 are exactly one bit too far); otherwise every plant differs from its
    query on all of the rest, so that NO row lies within the radius and the counters are the construction's. Plants sit in the first,
    a middle and the last tile; in the first step, the second (its last pair is carried across the trip boundary), the last step of
    the two-step loop (its last pair completes behind the loop), the masked step behind the loop and the last step; in every pair of
    the step, the last pair in all six (which block, distance) variants, rows alternating between the lane halves.
    Returns desc, pts, off, q, plants = [(row, query, which, dist, partner_dot)]."""
    rng = np.random.Generator(np.random.PCG64(seed))
    nq = nq_of(qt)
    desc = rng.integers(0, 256, (n_rows, 32), dtype=np.uint8)
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    d32, q32 = desc.view(np.uint32), q.view(np.uint32)
    rpt, tiles = FC.tiling(n_rows)
    n_full_waves, n_pairs = nq // (32 * qt), qt // 2
    free = {p: [(w, c) for w in range(n_full_waves) for c in range(32)] for p in range(n_pairs)}
    for p in free:
        rng.shuffle(free[p])
    row_order = [8 * (i // 8) + (i % 8) // 2 + 4 * (i % 2) for i in range(32)]      # lane halves alternate: 0, 4, 1, 5, ...
    plants, n = [], 0
    for ti in sorted({0, len(tiles) // 2, len(tiles) - 1}):
        n_local, ls = tiles[ti], FC.loop_steps(tiles[ti])
        for s in sorted({0, 1, max(ls - 1, 0), ls, (n_local - 1) // 32}):
            used = 0
            for p in range(n_pairs):
                variants = [(w, d) for w in ("first", "second", "both") for d in (radius, radius + 1)]
                if p != n_pairs - 1:
                    variants = [variants[(n + i) % 6] for i in (0, 3)]
                for which, dist in variants:
                    row = ti * rpt + 32 * s + row_order[used]
                    if row >= n_rows or not free[p]:
                        continue
                    used += 1
                    w, c = free[p].pop()
                    qa = w * 32 * qt + 64 * p + c                                      # query c of the pair's first block; qa + 32: of its second
                    own = {"first": (qa,), "second": (qa + 32,), "both": (qa, qa + 32)}[which]
                    if which == "both":
                        q32[qa + 32, list(FIRST)] = q32[qa, list(FIRST)]               # one row at the same first-part distance to both
                    base = q32[own[0]].copy()
                    flip_first_part(base, dist, rng)
                    if not within:
                        base[list(REST)] ^= np.uint32(0xFFFFFFFF)                      # 128 further away: not an answer at any radius here
                    d32[row] = base
                    partner_dot = 0
                    if which != "both":
                        partner = qa + 32 if which == "first" else qa
                        partner_dot = 128 if int(rng.integers(0, 2)) else -128
                        q32[partner, list(FIRST)] = base[list(FIRST)] ^ np.uint32(0 if partner_dot > 0 else 0xFFFFFFFF)
                        q32[partner, list(REST)] = base[list(REST)] ^ np.uint32(0xFFFFFFFF)   # 128 away on the rest: never an answer
                    plants.append((row, own[0], which, dist, partner_dot))
                    n += 1
    pts = rng.random((n_rows, 3), dtype=np.float32)
    off = np.array([0, n_rows // 3, 2 * n_rows // 3, n_rows], np.uint32)
    return np.ascontiguousarray(desc), pts, off, np.ascontiguousarray(q), plants
