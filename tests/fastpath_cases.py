"""Constructed DBs and queries for the split-block fast path of hamming_topk_fp4rows (tests/test_match_fastpath_gpu.py and its child
tests/fastpath_child.py), with what the CPU can say about them: the tiling the launcher will choose, the rows that must come out, and
the number of blocks that go on to their second part. No GPU here.

A block is 32 rows of a step x 32 queries; a wave holds QT blocks of queries (positions 0 .. QT-1). MFMA s of a block covers the
32-bit words s and 4 + s of the 8-word rows, so "the positions of the first 2 (3) MFMAs" are words {0, 1, 4, 5} ({0, 1, 2, 4, 5, 6})."""
import numpy as np

PART_WORDS = {2: (0, 1, 4, 5), 3: (0, 1, 2, 4, 5, 6)}
# rows: 8 tiles of 288 rows (9 steps: the two-step loop leaves one to the masked tail) whose last tile holds 1 step + 1 row (fewer than
# two full steps: no loop at all), 3 steps, 3 steps + 1 row, 4 steps + 31 rows, 5 steps; 2048 and 4096: 8 and 16 tiles of 8 steps (even,
# nothing left to the tail); the same last tiles behind 15 tiles of 288 (16 tiles: whole tiles per XCD, as with 8); 4065: 15 tiles, the
# linear work-item decode
ROWS = (2048, 2049, 2112, 2113, 2175, 2176, 4096, 4353, 4416, 4417, 4479, 4480, 4065)


def tiling(n_rows, want_tiles=1 << 20):
    """mfma_tile_rows(n_rows, want, 256, true) and tile_plan (tod_amd/csrc/match_tiles.h) for a launch that is not short of waves:
    rows per tile, and the rows of every tile"""
    n_tiles = min(max(1, want_tiles), max(1, n_rows // 256), 8192)
    if n_tiles >= 16:
        n_tiles &= ~7
    rpt = ((n_rows + n_tiles - 1) // n_tiles + 31) & ~31
    n_tiles = (n_rows + rpt - 1) // rpt
    return rpt, [min(n_rows, (t + 1) * rpt) - t * rpt for t in range(n_tiles)]


def loop_steps(n_local):
    """the steps of a tile that the two-step loop runs on split blocks (the rest is masked, whole blocks)"""
    return 2 * ((n_local // 32) // 2)


def make(n_rows, nq, qt, seed, only_part2=False):
    """Independent random bits, plus planted rows for chosen queries: 'full' rows equal their query; 'part2' / 'part3' rows equal it
    on the positions of the first 2 / 3 MFMAs and differ on 120 of the other 128 / on all of the other 64 (they pass the part test and
    fail the whole one at radius 35). Plants sit in the first, a middle and the last tile, in their first step, their second (its
    position QT-1 is carried across the trip boundary), the last step of the two-step loop (position QT-1 completes behind the loop),
    the masked steps behind it and the partial last step; in each such step one plant per block position, two for position QT-1: one in
    a row held by lanes 0-31 ((row >> 2) & 1 == 0) and one in a row held by lanes 32-63. The last query (which pads the ragged
    last query wave) gets a plant as well. Returns desc, pts, off, q, plants = [(row, query, kind)]."""
    rng = np.random.Generator(np.random.PCG64(seed))
    desc = rng.integers(0, 256, (n_rows, 32), dtype=np.uint8)
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    rpt, tiles = tiling(n_rows)
    n_qw = (nq + 32 * qt - 1) // (32 * qt)
    plants, used_q, used_r = [], set(), set()
    kinds = ("part2",) if only_part2 else ("full", "part2", "part3")

    def plant(row, qi, kind):
        if row >= n_rows or row in used_r or qi in used_q:
            return
        used_r.add(row); used_q.add(qi)
        d = q[qi].copy().view(np.uint32)
        if kind != "full":
            rest = [w for w in range(8) if w not in PART_WORDS[int(kind[-1])]]
            d[rest] ^= 0xFFFFFFFF
            if kind == "part2":                                 # "few of the rest": 8 of the 128 other positions agree again
                bits = d.view(np.uint8)
                for b in rng.choice(128, 8, replace=False):
                    w = rest[b >> 5]
                    bits[4 * w + ((b & 31) >> 3)] ^= np.uint8(1 << (b & 7))
        desc[row] = d.view(np.uint8)
        plants.append((row, qi, kind))

    n = 0
    for ti in sorted({0, len(tiles) // 2, len(tiles) - 1}):
        n_local, ls = tiles[ti], loop_steps(tiles[ti])
        steps = sorted({0, 1, max(ls - 1, 0), ls, (n_local - 1) // 32})
        for s in steps:
            for t in range(qt):
                for r in ((3 + 5 * t) % 32,) + (((28 + t) % 32,) if t == qt - 1 else ()):
                    # a query of block position t that has no plant yet, the query waves taken in turn (the ragged last wave has
                    # queries in its first position only)
                    free = [qi for w in range(n_qw) for qi in range(((n + w) % n_qw) * 32 * qt + 32 * t, min(nq, ((n + w) % n_qw) * 32 * qt + 32 * t + 32))
                            if qi not in used_q and qi != nq - 1]
                    if free:
                        plant(ti * rpt + 32 * s + r, free[int(rng.integers(0, min(4, len(free))))], kinds[n % len(kinds)])
                    n += 1
    plant(rpt + 32 + 9, nq - 1, "part2")                        # tile 1, step 1: every padded block of the last wave goes on
    pts = rng.random((n_rows, 3), dtype=np.float32)
    off = np.array([0, n_rows // 3, 2 * n_rows // 3, n_rows], np.uint32)
    return np.ascontiguousarray(desc), pts, off, np.ascontiguousarray(q), plants


def part_distances(desc, q, split):
    """Hamming distances over the positions of the first `split` MFMAs, rows x queries"""
    cols = np.concatenate([np.arange(4 * w, 4 * w + 4) for w in PART_WORDS[split]])
    a = np.unpackbits(desc[:, cols], axis=1).astype(np.float32)
    b = np.unpackbits(q[:, cols], axis=1).astype(np.float32)
    return (a.sum(1)[:, None] + b.sum(1)[None, :] - 2.0 * (a @ b.T)).astype(np.int32)


def split_counts(desc, q, qt, radius, split=2):
    """(blocks tested, blocks that go on) of one launch with the split forced, provided NO row lies within the radius of any query: the
    lists then stay empty, no threshold ever moves, and a block goes on exactly when some pair of it is closer than radius + 1 on
    the first part. Queries beyond the last repeat the last (load_query_block)."""
    nq = len(q)
    n_qw = (nq + 32 * qt - 1) // (32 * qt)
    rpt, tiles = tiling(len(desc))
    close = part_distances(desc, q, split) <= radius
    tested = passed = 0
    for ti, n_local in enumerate(tiles):
        ls = loop_steps(n_local)
        tested += ls * qt * n_qw
        for s in range(ls):
            rows = close[ti * rpt + 32 * s: ti * rpt + 32 * s + 32]
            for qw in range(n_qw):
                for t in range(qt):
                    qi = np.minimum(qw * 32 * qt + 32 * t + np.arange(32), nq - 1)
                    passed += int(rows[:, qi].any())
    return tested, passed
