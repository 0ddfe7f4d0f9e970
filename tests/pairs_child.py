"""Child of tests/test_match_pairs_gpu.py (TODHIP_K4X_QT and TODHIP_K4X_PAIRS are read once per process): split 2 forced on the
constructed DBs of tests/pairs_cases.py, k 1 and 2, radius 1, 35 and 63 (radius 0 is rejected by the API: asserted here), against the vector-ALU engine of the same context, bit for bit;
then, on DBs without a row inside the radius, the context's counters of blocks tested and blocks that went on against the CPU's count
(tests/fastpath_cases.py: split_counts). Prints "ok <launches compared> <sha256 of every answer>": the parent compares the digests of
the paired step and of the single-block step."""
import hashlib
import os
import sys

import numpy as np

import k4x_children as C
import fastpath_cases as FC
import pairs_cases as PC


def check_counters(desc, pts, off, q, qt, radius, what):
    tested, passed = FC.split_counts(desc, q, qt, radius)
    c = C.capi.Context(0)
    c.set_matcher_engine("mfma")
    c.set_matcher_block_split(2)
    c.db_load(desc, pts, off)
    seen = [(0, 0)]
    for _ in range(3):                                         # a launch's report is taken when the next launch starts
        row_ptr, _, _ = c.match(q, 2, radius)
        assert int(row_ptr[-1]) == 0, what
        cnt = c.counters()
        assert cnt.last_block_split == 2 and cnt.last_fp4_rows == 1
        seen.append((int(cnt.k4x_half_blocks), int(cnt.k4x_half_blocks_completed)))
    print("counters %s: tested %d went on %d, device %s" % (what, tested, passed, seen[2:]), file=sys.stderr)
    assert seen[1] == (0, 0) and seen[2] == (tested, passed) and seen[3] == (2 * tested, 2 * passed), (what, seen, tested, passed)
    c.close()


def main():
    qt = C.qt_from_env()
    assert os.environ.get("TODHIP_K4X_PAIRS") in ("0", "1")
    digest = hashlib.sha256()
    ctx = C.capi.Context(0)
    n = 0
    for n_rows in FC.ROWS:
        for radius in PC.RADII:
            desc, pts, off, q, plants = PC.make(n_rows, qt, radius, 31 * n_rows + radius, within=True)
            ctx.db_load(desc, pts, off)
            if radius == PC.RADII[0]:                          # the lowest radius a match takes
                try:
                    ctx.match(q, 1, 0)
                    raise AssertionError("radius 0 was accepted")
                except C.capi.TodError:
                    pass
            for k in (1, 2):
                want = C.valu_answer(ctx, q, k, radius)
                for row, qi, which, dist, _ in plants:         # a plant at the radius is its query's best answer, one beyond is none
                    lo, hi = int(want[0][qi]), int(want[0][qi + 1])
                    if dist == radius:
                        m = want[1][lo]
                        assert hi > lo and int(off[m["imgIdx"]]) + int(m["trainIdx"]) == row and int(m["distance"]) == radius, (n_rows, radius, row, qi)
                    else:
                        assert hi == lo, (n_rows, radius, row, qi)
                n += C.compare_forms(ctx, q, k, radius, want, (2,), (n_rows, radius))
                ctx.set_matcher_engine("mfma")
                got = ctx.match(q, k, radius)
                digest.update(np.ascontiguousarray(got[0]).tobytes())
                for f in C.FIELDS:
                    digest.update(np.ascontiguousarray(got[1][f]).tobytes())
                digest.update(np.ascontiguousarray(got[2]).tobytes())
            ctx.set_matcher_block_split(-1)
    ctx.close()
    for n_rows, radius in ((2113, 35), (4479, 63), (4065, 1), (2176, 63)):
        desc, pts, off, q, plants = PC.make(n_rows, qt, radius, 17 * n_rows + radius, within=False)
        check_counters(desc, pts, off, q, qt, radius, (n_rows, radius))
        n += 1
    print("ok %d %s" % (n, digest.hexdigest()))


if __name__ == "__main__":
    main()
