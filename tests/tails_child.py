"""Child of tests/test_match_tails_gpu.py (TODHIP_K4X_QT is read once per process): hamming_topk_fp4rows on the constructed DBs of
tests/tails_cases.py -- a block that goes on loads the tails of its own step and of its own query -- each block form forced, against
the vector-ALU engine in the same context, bit for bit; then the two counters of the split-2 form against the CPU's count."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from tod_amd import capi
import fastpath_cases as FC
import tails_cases as TC

FIELDS = ("queryIdx", "trainIdx", "imgIdx", "distance")
# radius -> the block forms forced at it (0: whole blocks; their code path has no tails, one radius is enough)
FORMS = ((35, (2, 3, 0)), (36, (2, 3)), (90, (3,)))


def same(a, b):
    return np.array_equal(a[0], b[0]) and all(np.array_equal(a[1][f], b[1][f]) for f in FIELDS) and np.array_equal(a[2], b[2])


def found(res, off, qi):
    """[(row, distance)] of query qi in a match result"""
    m = res[1][int(res[0][qi]):int(res[0][qi + 1])]
    return [(int(off[x["imgIdx"]]) + int(x["trainIdx"]), int(x["distance"])) for x in m]


def main():
    qt = int(os.environ["TODHIP_K4X_QT"])
    assert qt in (4, 6) and os.environ.get("TODHIP_K4X_FP4_ROWS") == "1"
    nq = 192 * 2 + 5 if qt == 6 else 128                       # three query waves of six blocks, the last ragged; one wave of four
    ctx = capi.Context(0)
    n = 0
    for n_rows in FC.ROWS:
        desc, pts, off, q, plants = TC.make(n_rows, nq, qt, 4100 + n_rows)
        ctx.db_load(desc, pts, off)
        for k in (1, 2, 5):
            for radius, splits in FORMS:
                ctx.set_matcher_engine("valu")
                want = ctx.match(q, k, radius)
                if radius < 90:                                # the plants are the answers (the CPU test holds them to the oracle)
                    for p in plants:
                        d = p["a"] + p["b"]
                        assert found(want, off, p["query"]) == ([(p["row"], d)] if d <= radius else []), (n_rows, k, radius, p)
                ctx.set_matcher_engine("mfma")
                for split in splits:
                    ctx.set_matcher_block_split(split)
                    got = ctx.match(q, k, radius)
                    cnt = ctx.counters()
                    assert cnt.last_fp4_rows == 1 and cnt.last_block_split == (4 if split == 0 else split), (n_rows, k, radius, split, cnt.last_block_split)
                    assert same(got, want), (n_rows, k, radius, split)
                    n += 1
        ctx.set_matcher_block_split(-1)
    ctx.close()
    # the counters: no row within the radius, so no threshold moves and both counts are a property of the construction. A launch's
    # report is taken when the next launch starts.
    for n_rows in (2113, 4479, 4065, 2049):
        desc, pts, off, q, plants = TC.make(n_rows, nq, qt, 5200 + n_rows, clean=True)
        tested, passed = FC.split_counts(desc, q, qt, 35)
        c = capi.Context(0)
        c.set_matcher_engine("mfma")
        c.set_matcher_block_split(2)
        c.db_load(desc, pts, off)
        seen = [(0, 0)]
        for _ in range(3):
            row_ptr, _, _ = c.match(q, 2, 35)
            assert int(row_ptr[-1]) == 0
            cnt = c.counters()
            assert cnt.last_block_split == 2 and cnt.last_fp4_rows == 1
            seen.append((int(cnt.k4x_half_blocks), int(cnt.k4x_half_blocks_completed)))
        assert seen[1] == (0, 0) and seen[2] == (tested, passed) and seen[3] == (2 * tested, 2 * passed), (n_rows, seen, tested, passed)
        c.close()
        n += 1
    print("ok %d" % n)


if __name__ == "__main__":
    main()
