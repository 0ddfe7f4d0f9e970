"""Constructed DBs and queries for the exchange of distance bounds in the paired split-2 step of hamming_topk_fp4rows
(tests/test_match_ondemand_bounds_gpu.py and its child tests/ondemand_bounds_child.py). No GPU here. The tiling the launcher will
choose and the CPU's count of blocks that go on: tests/fastpath_cases.py.

The paired step exchanges bounds between the tiles of a query only where a block goes on (fp4rows_pair_complete): it loads the
query's published bound there, applies it with <=, and publishes its own list's bound once the list is full. What can go wrong is a
bound that prunes a row the answer needs (a tie a smaller row index elsewhere should win, a row at exactly the bound), a bound that
is published from a list that is not full, or a completion that names the wrong rows. So every third query gets plants of one of
four kinds, in turn:

  falling  k + 1 rows within the radius in each of three tiles, the distances falling from tile to tile: the answer is the last
           tile's, whatever the earlier tiles published
  rising   the same with the distances rising: the later tiles' rows lose against the first tile's bound
  tie      k - 1 near rows and a row at distance TIE_D in one tile (a full list: it publishes TIE_D) and a second row at TIE_D in another
           tile; the smaller row index wins the last place, so the other tile must keep a row AT the published bound. The full
           list is in the earlier tile for one such query and in the later one for the next
  edge     a row at exactly the radius and one at radius + 1, in two tiles: the first is the answer, the second is none

Plants go to queries of every block position, so also to the blocks of a step's last pair, whose test is carried into the next step;
in a DB whose last tile ends in a partial step, the edge queries' row at the radius stands in that step for some of them."""
import numpy as np

import fastpath_cases as FC

RADIUS = 35
TIE_D = 12
ROWS = (16384, 16403)                                          # 64 tiles of 8 steps; 56 tiles of 9 steps and one of 8 steps + 19 rows
KINDS = ("falling", "rising", "tie", "edge")
N_OBJECTS = 9


def nq_of(qt):
    return 380 if qt == 6 else 250                             # two query waves each, the last block of the second one padded


def at_distance(query_row, d, rng):
    """a copy of the 32-byte row with d of its 256 bits flipped"""
    bits = np.unpackbits(query_row)
    bits[rng.choice(256, d, replace=False)] ^= 1
    return np.packbits(bits)


def make(n_rows, qt, k, seed):
    """Returns desc, pts, off, q, plants = [(row, query, kind, distance)]"""
    rng = np.random.Generator(np.random.PCG64(seed))
    nq = nq_of(qt)
    desc = rng.integers(0, 256, (n_rows, 32), dtype=np.uint8)
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    rpt, tiles = FC.tiling(n_rows)
    n_tiles = len(tiles)
    used, plants = set(), []

    def free_row(tile, lo=0, hi=None):
        hi = tiles[tile] if hi is None else hi
        while True:
            row = tile * rpt + int(rng.integers(lo, hi))
            if row not in used:
                used.add(row)
                return row

    def plant(qi, kind, tile, d, lo=0, hi=None):
        row = free_row(tile, lo, hi)
        desc[row] = at_distance(q[qi], d, rng)
        plants.append((row, qi, kind, d))

    partial = tiles[-1] % 32 != 0                              # the DB's last tile ends in a partial step
    for n, qi in enumerate(range(0, nq, 3)):
        kind = KINDS[n % 4]
        t3 = sorted(int(t) for t in rng.choice(n_tiles, 3, replace=False))
        if kind in ("falling", "rising"):
            base = (3 * (k + 1), 2 * (k + 1), k + 1) if kind == "falling" else (k + 1, 2 * (k + 1), 3 * (k + 1))
            for tile, b in zip(t3, base):                      # distances b - k .. b, all distinct, all <= 18 < RADIUS
                for j in range(k + 1):
                    plant(qi, kind, tile, b - j)
        elif kind == "tie":
            full, other = (t3[0], t3[2]) if (n // 4) % 2 == 0 else (t3[2], t3[0])
            for j in range(k - 1):
                plant(qi, kind, full, 2 + j)
            plant(qi, kind, full, TIE_D)
            plant(qi, kind, other, TIE_D)
        else:
            if partial and (n // 4) % 2 == 0:                  # the row at the radius in the last tile's partial step
                plant(qi, kind, n_tiles - 1, RADIUS, lo=tiles[-1] - tiles[-1] % 32)
                t3 = [t for t in t3 if t != n_tiles - 1]
            else:
                plant(qi, kind, t3[0], RADIUS)
            plant(qi, kind, t3[1], RADIUS + 1)
    pts = rng.random((n_rows, 3), dtype=np.float32)
    off = np.array([n_rows * i // N_OBJECTS for i in range(N_OBJECTS + 1)], np.uint32)
    return np.ascontiguousarray(desc), pts, off, np.ascontiguousarray(q), plants


def distances(desc, q):
    """Hamming distances, rows x queries"""
    a = np.unpackbits(desc, axis=1).astype(np.float32)
    b = np.unpackbits(q, axis=1).astype(np.float32)
    return (a.sum(1)[:, None] + b.sum(1)[None, :] - 2.0 * (a @ b.T)).astype(np.int64)


def knn(desc, q, k, radius, rows=None):
    """The definition: per query the k smallest keys (distance, row) among `rows` (all) with distance <= radius, ascending.
    Returns a list of lists of (distance, row)."""
    d = distances(desc, q)
    keys = d * (1 << 32) + np.arange(len(desc), dtype=np.int64)[:, None]
    if rows is not None:
        mask = np.zeros(len(desc), bool)
        mask[rows] = True
        keys[~mask] = np.iinfo(np.int64).max
    out = []
    part = np.sort(np.partition(keys, k, axis=0)[:k + 1], axis=0)[:k]
    for qi in range(len(q)):
        out.append([(int(key) >> 32, int(key) & 0xFFFFFFFF) for key in part[:, qi] if (int(key) >> 32) <= radius])
    return out
