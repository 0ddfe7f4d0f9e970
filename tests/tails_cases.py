"""Constructed DBs and queries that pin down WHOSE tail the split-block DB pass reads when a block goes on (hamming_topk_fp4rows' split-2
form loads the fragments behind the split, and the query's words behind it, on demand: tests/test_match_tails_gpu.py and its child
tests/tails_child.py). On fastpath_cases' tilings and query counts, with what the CPU can say about them. No GPU here.

MFMA s of a block covers words s and 4 + s of the 8-word rows (fastpath_cases.PART_WORDS): fragment 2 is words {2, 6}, fragment 3 is
words {3, 7}; "the tail" below is both, the part that split 2 leaves behind (split 3 leaves fragment 3 only; its first part then holds
the plant's `a` differing positions, which still pass the part test at every radius the tests use).

  tail_in    the row equals its query on the first part (words 0, 1, 4, 5) and differs from it in `a` positions of fragment 2 and `b`
             of fragment 3, a != b, a + b <= 35, the pair (a, b) distinct per plant: it must come back with distance exactly a + b
  tail_out   the same with a + b = 36: absent at radius 35, present with distance 36 at radius 36
  decoys     around a plant (row, query): the rows at the same lane position of the step before and of the step after (row -+ 32) and
             the row of the other lane half (row ^ 4) keep their random first part and get the QUERY's tail; the queries 32 below and
             above (the same lane of the neighbouring query blocks) keep their random first part and get the ROW's tail. None of them is
             a match, but a tail taken from the wrong step, lane half or query block gives the plant distance 0: a tail_out becomes a
             hit, a tail_in changes its distance.

A plant is placed in every block position fastpath_cases.make names: first, a middle and the last tile; their first step, their second
(position QT-1 is carried across the trip boundary), the last step of the two-step loop (position QT-1 completes behind the loop), the
masked steps behind it; every block position, the last one in both lane halves; and the last query, which pads the ragged last wave.
Rows and queries are handed out so that no plant or decoy touches another's; where the 128 queries of the four-block case or a short
tile leave no room for one of a plant's decoys, that decoy is left out and the plant records which it has (the CPU test holds the
coverage that remains to a floor)."""
import numpy as np

import fastpath_cases as FC

TAIL_WORDS = [2, 3, 6, 7]
FRAG_WORDS = {2: (2, 6), 3: (3, 7)}


def _flip(words, frag, n, rng):
    """flip n distinct bit positions of fragment `frag` of the 8-word row `words`"""
    for b in rng.choice(64, n, replace=False):
        words[FRAG_WORDS[frag][int(b) >> 5]] ^= np.uint32(1 << (int(b) & 31))


def make(n_rows, nq, qt, seed, clean=False):
    """Returns desc, pts, off, q, plants = [dict(row, query, kind, a, b, step, t, rows=[decoy rows], queries=[decoy queries],
    missing=the decoys that exist (a row or query beyond the ends does not) but were taken)].
    clean: no tail_in plants (every plant is a tail_out): no row lies within radius 35 of any query"""
    rng = np.random.Generator(np.random.PCG64(seed))
    desc = rng.integers(0, 256, (n_rows, 32), dtype=np.uint8)
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    d32, q32 = desc.view(np.uint32), q.view(np.uint32)
    rpt, tiles = FC.tiling(n_rows)
    n_qw = (nq + 32 * qt - 1) // (32 * qt)
    pairs_in = [(a, b) for a in range(1, 35) for b in range(1, 35) if a != b and a + b <= 35]
    pairs_out = [(a, 36 - a) for a in range(0, 37) if a != 18]
    rng.shuffle(pairs_in); rng.shuffle(pairs_out)
    used_r, used_q, plants = set(), set(), []

    def plant(ti, s, t, half, kind, qi_fixed=None):
        # the query: of block position t, itself and -- if any can be had -- its neighbours 32 below and above untouched so far
        if qi_fixed is None:
            cand = [w * 32 * qt + 32 * t + c for w in range(n_qw) for c in range(32)]
            cand = [x for x in cand if x < nq - 1 and x not in used_q]
            if not cand:
                return
            start = int(rng.integers(0, len(cand)))
            cand = cand[start:] + cand[:start]
            full = [x for x in cand if all(y in range(nq) and y not in used_q for y in (x - 32, x + 32))]
            qi = (full or cand)[0]
        else:
            qi = qi_fixed
        # the row: in step s of tile ti, in the lane half asked for, with as many of its three neighbours free as can be had
        base = ti * rpt + 32 * s
        cand = [base + r for r in range(32) if ((r >> 2) & 1) == half and base + r < n_rows and base + r not in used_r]
        if not cand:
            return
        start = int(rng.integers(0, len(cand)))
        cand = cand[start:] + cand[:start]
        free = lambda x: sum(y in range(n_rows) and y not in used_r for y in (x - 32, x + 32, x ^ 4))
        row = max(cand, key=free)
        if kind == "tail_out":                                  # 36 pairs: they repeat where a DB has more tail_out plants than that
            a, b = pairs_out[sum(p["kind"] == "tail_out" for p in plants) % len(pairs_out)]
        else:
            a, b = pairs_in.pop()
        d = q32[qi].copy()
        _flip(d, 2, a, rng); _flip(d, 3, b, rng)
        d32[row] = d
        used_r.add(row); used_q.add(qi)
        p = dict(row=row, query=qi, kind=kind, a=a, b=b, step=s, t=t, rows=[], queries=[], missing=0)
        for y in (row - 32, row + 32, row ^ 4):
            if y in range(n_rows) and y not in used_r:
                d32[y, TAIL_WORDS] = q32[qi, TAIL_WORDS]
                used_r.add(y); p["rows"].append(y)
            elif y in range(n_rows):
                p["missing"] += 1
        for y in (qi - 32, qi + 32):
            if y in range(nq) and y not in used_q:
                q32[y, TAIL_WORDS] = d32[row, TAIL_WORDS]
                used_q.add(y); p["queries"].append(y)
            elif y in range(nq):
                p["missing"] += 1
        plants.append(p)

    n = 0
    kinds = ("tail_out",) if clean else ("tail_in", "tail_out", "tail_in")
    plant(1 if len(tiles) > 1 else 0, 1, 0, 1, kinds[0], qi_fixed=nq - 1)   # the last query: the padded blocks of the last wave go on with it
    for ti in sorted({0, len(tiles) // 2, len(tiles) - 1}):
        n_local, ls = tiles[ti], FC.loop_steps(tiles[ti])
        for s in sorted({0, 1, max(ls - 1, 0), ls, (n_local - 1) // 32}):
            if 32 * s >= n_local:
                continue
            for t in range(qt):
                for half in (((3 + 5 * t) >> 2) & 1,) + ((1 - (((3 + 5 * t) >> 2) & 1),) if t == qt - 1 else ()):
                    plant(ti, s, t, half, kinds[n % len(kinds)])
                    n += 1
    pts = rng.random((n_rows, 3), dtype=np.float32)
    off = np.array([0, n_rows // 3, 2 * n_rows // 3, n_rows], np.uint32)
    return np.ascontiguousarray(desc), pts, off, np.ascontiguousarray(q), plants


def distances(desc, q):
    """all Hamming distances, rows x queries"""
    a = np.unpackbits(desc, axis=1).astype(np.float32)
    b = np.unpackbits(q, axis=1).astype(np.float32)
    return (a.sum(1)[:, None] + b.sum(1)[None, :] - 2.0 * (a @ b.T)).astype(np.int32)
