"""The split-2 form of hamming_topk_fp4rows (tod_amd/csrc/match_fp4rows.h) keeps only the fragments in front of the split in its loop; a
block that goes on loads the tails of ITS step from the fp4 copy and the tail words of ITS query, where it goes on (split 3 and whole
blocks keep all four fragments resident and are held to the same answers here). The fast-path tests
(tests/test_match_fastpath_gpu.py) cover "goes on and fails" and "distance 0"; what they do not pin down is whose tail is read.
tests/tails_cases.py does: rows that equal their query in front of the split and differ behind it in a known number of positions of
each fragment (inside the radius with the distance named, or one position outside it), with decoys in the neighbouring steps, the other
lane half and the neighbouring query blocks that carry the very tail a wrong address would fetch -- on fastpath_cases' tilings (loops of
odd and even step counts, last tiles of 0, 1 and 31 rows behind full steps or with fewer than two full steps, 8, 15 and 16 tiles) and
query counts (389 in three waves of six blocks, the last padded; 128 in one of four). First on the CPU: the oracle's answers on these
DBs are exactly the construction. Then on the GPU (tests/tails_child.py, a child per query-block count): k 1, 2, 5, split 2 at radius
35 and 36, split 3 at 35, 36 and 90, whole blocks, each bit for bit against the vector engine of the same context; and with split 2
forced on a DB without any row inside the radius, blocks tested and blocks that went on equal the CPU's count."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import fastpath_cases as FC
import tails_cases as TC

HERE = os.path.dirname(os.path.abspath(__file__))
NQ = {6: 192 * 2 + 5, 4: 128}


@pytest.mark.parametrize("qt", [6, 4])
def test_the_oracles_answers_are_the_construction(qt):
    nq = NQ[qt]
    for n_rows in FC.ROWS:
        desc, pts, off, q, plants = TC.make(n_rows, nq, qt, 4100 + n_rows)
        rpt, tiles = FC.tiling(n_rows)
        D = TC.distances(desc, q)
        d2 = FC.part_distances(desc, q, 2)
        ins = {(p["row"], p["query"]): p["a"] + p["b"] for p in plants if p["kind"] == "tail_in"}
        outs = {(p["row"], p["query"]) for p in plants if p["kind"] == "tail_out"}
        assert len(ins) > 2 * qt and len(outs) > qt and plants[0]["query"] == nq - 1
        # the construction: equal in front of the split, a and b positions in fragments 2 and 3, distinct pairs
        w = lambda x: x.view(np.uint32)
        bits = lambda x: int(np.unpackbits(np.ascontiguousarray(x).view(np.uint8)).sum())
        for p in plants:
            r, c = w(desc[p["row"]]), w(q[p["query"]])
            assert d2[p["row"], p["query"]] == 0 and p["a"] != p["b"]
            assert bits(r[[2, 6]] ^ c[[2, 6]]) == p["a"] and bits(r[[3, 7]] ^ c[[3, 7]]) == p["b"]
            assert p["a"] + p["b"] <= 35 if p["kind"] == "tail_in" else p["a"] + p["b"] == 36
            for y in p["rows"]:                                 # decoys: the tail a wrong step or lane half would fetch, no match themselves
                assert np.array_equal(w(desc[y])[TC.TAIL_WORDS], c[TC.TAIL_WORDS]) and d2[y, p["query"]] > 36
            for y in p["queries"]:                              # the tail a wrong query block would fetch
                assert np.array_equal(w(q[y])[TC.TAIL_WORDS], r[TC.TAIL_WORDS]) and d2[p["row"], y] > 36
        assert len({(p["a"], p["b"]) for p in plants if p["kind"] == "tail_in"}) == len(ins)
        # nothing but the plants within 36, nothing but the tail_in plants within 35
        assert {(int(r), int(c)) for r, c in zip(*np.nonzero(D <= 35))} == set(ins)
        assert {(int(r), int(c)) for r, c in zip(*np.nonzero(D <= 36))} == set(ins) | outs
        # the oracle's answers at radius 35 and 36
        for radius in (35, 36):
            rc, row_ptr, m, _ = O.match(desc, off, pts, q, 2, radius)
            got = {(int(off[x["imgIdx"]]) + int(x["trainIdx"]), int(x["queryIdx"])): int(x["distance"]) for x in m}
            want = dict(ins)
            if radius == 36:
                want.update({k: 36 for k in outs})
            assert rc == 0 and got == want, (n_rows, radius)
        # coverage: a plant in every block position of a first step, a second step, the loop's last step and a step behind the loop;
        # the last position in both lane halves; and of every kind some whose decoys are complete
        ls = FC.loop_steps(tiles[0])
        for s in sorted({0, 1, ls - 1, min(ls, (tiles[0] - 1) // 32)}):   # (8 steps: nothing behind the loop)
            here = [p for p in plants if p["row"] // rpt == 0 and p["step"] == s]
            assert {p["t"] for p in here} == set(range(qt)), (n_rows, s)
            assert {(p["row"] >> 2) & 1 for p in here if p["t"] == qt - 1} == {0, 1}, (n_rows, s)
        for kind in ("tail_in", "tail_out"):
            whole = [p for p in plants if p["kind"] == kind and p["missing"] == 0 and p["rows"] and p["queries"]]
            assert len(whole) >= qt and any(p["t"] == qt - 1 for p in whole), (n_rows, kind, len(whole))


@pytest.mark.parametrize("qt", [6, 4])
def test_count_of_the_blocks_that_go_on(qt):
    nq = NQ[qt]
    n_qw = (nq + 32 * qt - 1) // (32 * qt)
    for n_rows in (2113, 4479, 4065, 2049):
        desc, pts, off, q, plants = TC.make(n_rows, nq, qt, 5200 + n_rows, clean=True)
        assert int(O.knn_keys(desc, q, 1)[:, 0].min() >> 32) == 36          # no row within radius 35: the thresholds never move
        tested, passed = FC.split_counts(desc, q, qt, 35)
        rpt, tiles = FC.tiling(n_rows)
        assert tested == sum(FC.loop_steps(t) for t in tiles) * qt * n_qw
        in_loop = {(p["row"] // 32, p["query"] // 32) for p in plants if (p["row"] % rpt) // 32 < FC.loop_steps(tiles[p["row"] // rpt])}
        # every block with a plant in a loop step goes on; the last query's plant makes one more go on per padded position
        assert len(in_loop) <= passed <= len(in_loop) + qt + 2 and passed > 2 * qt


def child(qt):
    env = dict(os.environ, TODHIP_K4X_FP4_ROWS="1", TODHIP_K4X_QT=str(qt))
    return subprocess.run([sys.executable, os.path.join(HERE, "tails_child.py")], env=env, capture_output=True, text=True, timeout=600)


@pytest.mark.gpu
@pytest.mark.parametrize("qt", [6, 4])
def test_tails_come_from_the_blocks_own_step_and_query(qt):
    p = child(qt)
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout[-2000:] + p.stderr[-4000:]
    assert int(p.stdout.split()[1]) == len(FC.ROWS) * 3 * 6 + 4
