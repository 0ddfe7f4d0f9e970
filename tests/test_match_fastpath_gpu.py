"""The split-block fast path of hamming_topk_fp4rows (tod_amd/csrc/match_fp4rows.h): the block that goes on to its second part is the
unlikely side of its test, laid out behind the loop, and counts itself there. tests/fastpath_cases.py constructs DBs whose planted rows
make a block go on in every block position of a step -- the last position, whose test is carried into the next step, in the first step
of a tile, across the boundary of a two-step trip, in the last step of the loop, in rows held by either half of the lanes -- over tiles
that leave the loop an odd and an even number of steps, a last tile of 3, 4 and 5 full steps with 0, 1 and 31 rows behind them or with
fewer than two full steps, in 8, 15 and 16 tiles (both work-item decodes). The launcher gives a tile at least 256 rows, so the short
tiles are last tiles. First on the CPU: the planted rows are the oracle's answers. Then on the GPU (tests/fastpath_child.py, a child
per query-block count since the knob is read once per process): 389 queries in three waves of six blocks and 128 in one of four,
k 1, 2, 5, split 2 at radius 35, split 3 at 35 and 90, whole blocks, each bit for bit against the vector engine of the same context;
and with split 2 forced on a DB without any row inside the radius, the context's counters of blocks tested and blocks that went on
equal the CPU's count exactly."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import fastpath_cases as FC

HERE = os.path.dirname(os.path.abspath(__file__))
NQ = {6: 192 * 2 + 5, 4: 128}


def test_tilings_are_the_ones_the_cases_name():
    steps = lambda n: [(t // 32, t % 32) for t in FC.tiling(n)[1]]
    assert steps(2048) == [(8, 0)] * 8 and steps(4096) == [(8, 0)] * 16
    for n, tiles, last in ((2049, 8, (1, 1)), (2112, 8, (3, 0)), (2113, 8, (3, 1)), (2175, 8, (4, 31)), (2176, 8, (5, 0)),
                           (4353, 16, (1, 1)), (4416, 16, (3, 0)), (4417, 16, (3, 1)), (4479, 16, (4, 31)), (4480, 16, (5, 0)), (4065, 15, (1, 1))):
        assert steps(n) == [(9, 0)] * (tiles - 1) + [last], n
    assert set(FC.ROWS) == {2048, 4096, 2049, 2112, 2113, 2175, 2176, 4353, 4416, 4417, 4479, 4480, 4065}


@pytest.mark.parametrize("qt", [6, 4])
def test_planted_rows_are_the_oracles_answers(qt):
    nq = NQ[qt]
    for n_rows in FC.ROWS:
        desc, pts, off, q, plants = FC.make(n_rows, nq, qt, 77 + n_rows)
        keys = O.knn_keys(desc, q, 2)
        rpt, tiles = FC.tiling(n_rows)
        kinds = {kind for _, _, kind in plants}
        assert kinds == {"full", "part2", "part3"} and len(plants) > 3 * qt
        # a plant in every block position; the last position in both lane halves, in a first step, a second step and a last loop step
        pos = {(((qi % (32 * qt)) // 32), (row % rpt) // 32, (row >> 2) & 1) for row, qi, _ in plants}
        assert {t for t, _, _ in pos} == set(range(qt))
        ls = FC.loop_steps(tiles[0])
        for s in (0, 1, ls - 1):
            assert {h for t, st, h in pos if t == qt - 1 and st == s} == {0, 1}, (n_rows, s)
        d2 = FC.part_distances(desc, q, 2)
        d3 = FC.part_distances(desc, q, 3)
        for row, qi, kind in plants:
            best = int(keys[qi][0])
            if kind == "full":
                assert best == row, (n_rows, row, qi)                      # distance 0
            elif kind == "part3":
                assert best == (64 << 32) | row and d3[row, qi] == 0       # passes either part test, fails the whole one at radius 35
            else:
                assert (best >> 32) > 35 and d2[row, qi] == 0 and d3[row, qi] >= 56   # nothing within radius 35, the plant 120 away; passes split 2 only


@pytest.mark.parametrize("qt", [6, 4])
def test_pass_count_of_the_construction(qt):
    nq = NQ[qt]
    n_qw = (nq + 32 * qt - 1) // (32 * qt)
    for n_rows in (2113, 4479, 4065):
        desc, pts, off, q, plants = FC.make(n_rows, nq, qt, 991 + n_rows, only_part2=True)
        assert int(O.knn_keys(desc, q, 1)[:, 0].min() >> 32) > 35          # no row within the radius: the thresholds never move
        tested, passed = FC.split_counts(desc, q, qt, 35)
        rpt, tiles = FC.tiling(n_rows)
        assert tested == sum(FC.loop_steps(t) for t in tiles) * qt * n_qw
        in_loop = {(row // 32, qi // 32) for row, qi, _ in plants if (row % rpt) // 32 < FC.loop_steps(tiles[row // rpt])}
        # every block with a plant in a loop step goes on; the last query's plant makes one more go on per padded position
        assert len(in_loop) <= passed <= len(in_loop) + qt + 2 and passed > 2 * qt


def child(qt):
    env = dict(os.environ, TODHIP_K4X_FP4_ROWS="1", TODHIP_K4X_QT=str(qt))
    return subprocess.run([sys.executable, os.path.join(HERE, "fastpath_child.py")], env=env, capture_output=True, text=True, timeout=600)


@pytest.mark.gpu
@pytest.mark.parametrize("qt", [6, 4])
def test_fast_path_equals_the_vector_engine_and_counts_its_passes(qt):
    p = child(qt)
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout[-2000:] + p.stderr[-4000:]
    assert int(p.stdout.split()[1]) == len(FC.ROWS) * 3 * 4 + 3
