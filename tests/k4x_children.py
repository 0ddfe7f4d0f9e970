"""What the children of the K4x GPU tests repeat (tests/fp4_rows_child.py, fastpath_child.py, tails_child.py; each runs as a script in
a process of its own, since TODHIP_K4X_FP4_ROWS and TODHIP_K4X_QT are read once per process): the comparison of every forced block form
of hamming_topk_fp4rows against the vector-ALU engine of the same context, bit for bit, and the split-2 counters against the CPU's
count. The cases, and what is asserted about planted answers, stay with each child."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tod_amd import capi
import fastpath_cases as FC

FIELDS = ("queryIdx", "trainIdx", "imgIdx", "distance")


def same(a, b):
    return np.array_equal(a[0], b[0]) and all(np.array_equal(a[1][f], b[1][f]) for f in FIELDS) and np.array_equal(a[2], b[2])


def qt_from_env():
    """The query blocks per wave this process was started for; the copy must be on"""
    assert os.environ.get("TODHIP_K4X_FP4_ROWS") == "1" and os.environ.get("TODHIP_K4X_QT") in ("4", "6")
    return int(os.environ["TODHIP_K4X_QT"])


def nq_of(qt):
    return 192 * 2 + 5 if qt == 6 else 128                     # three query waves of six blocks, the last ragged; one wave of four


def valu_answer(ctx, q, k, radius):
    ctx.set_matcher_engine("valu")
    return ctx.match(q, k, radius)


def compare_forms(ctx, q, k, radius, want, splits, what):
    """Each block form of `splits` forced (0: whole blocks) on the matrix cores: the launch read the copy, ran the form asked for -- or
    the lowest one the thresholds allow, if that is higher -- and found `want`, bit for bit. Returns the number of launches compared."""
    lowest = 2 if radius + 1 <= 64 else (3 if radius + 1 <= 96 else 4)
    ctx.set_matcher_engine("mfma")
    for split in splits:
        ctx.set_matcher_block_split(split)
        got = ctx.match(q, k, radius)
        cnt = ctx.counters()
        form = 4 if split == 0 else max(split, lowest)
        assert cnt.last_fp4_rows == 1 and cnt.last_block_split == form, (what, k, radius, split, cnt.last_fp4_rows, cnt.last_block_split)
        assert same(got, want), (what, k, radius, split)
    return len(splits)


def check_split_counters(desc, pts, off, q, qt, what):
    """Split 2 forced on a DB without a row within radius 35: no threshold moves, so blocks tested and blocks that went on are a property
    of the construction (FC.split_counts). A launch's report is taken when the next launch starts."""
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
    assert seen[1] == (0, 0) and seen[2] == (tested, passed) and seen[3] == (2 * tested, 2 * passed), (what, seen, tested, passed)
    c.close()
