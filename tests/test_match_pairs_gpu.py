"""The paired split-2 step of hamming_topk_fp4rows (tod_amd/csrc/match_fp4rows.h, match_pair_pack.h): two query blocks share an
accumulator as two fixed-point fields, and one OR over 16 registers tests both against the launch's radius. tests/pairs_cases.py plants
rows whose first-part distance to their query is exactly the radius (the block goes on) and exactly one more (it does not), in the first
block of a pair, in the second and in both, in every pair of a step -- the last pair, whose test is carried into the next step, in the
first step of a tile, across the boundary of a two-step trip and in the last step of the loop, where it completes behind the loop -- in
rows of both lane halves, with the partner block's query at dot +128 or -128 to the same row, so that a carry or borrow between the
fields would show. First on the CPU: what the construction claims. Then on the GPU (tests/pairs_child.py, a child per query-block
count and per step form, since both knobs are read once per process): split 2 forced, six and four query blocks per wave, k 1 and 2,
radius 1, 35 and 63 (radius 0 is no search: the API rejects it, which the child asserts; cut 1 of the packing is covered on the host
by tests/test_pair_pack_cpu.py; cut 64: thrp = 0, the edge), DBs of 2048 .. 4480 rows, each answer bit for bit the vector engine's and the same
with TODHIP_K4X_PAIRS=0; and on DBs without a row inside the radius the counters of blocks tested and blocks that went on equal the
CPU's count: a block whose partner alone went on is not counted."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fastpath_cases as FC
import pairs_cases as PC

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("qt", [6, 4])
def test_the_construction_is_what_it_claims(qt):
    for n_rows, radius, within in ((2113, 35, True), (4480, 63, True), (2049, 1, True), (4479, 63, False), (4065, 1, False)):
        desc, pts, off, q, plants = PC.make(n_rows, qt, radius, 31 * n_rows + radius, within)
        assert len(q) == PC.nq_of(qt) and len(q) % (32 * qt) == 5
        rpt, tiles = FC.tiling(n_rows)
        d2 = FC.part_distances(desc, q, 2)
        full = np.unpackbits(desc[:, None, :] ^ q[None, [p[1] for p in plants], :], axis=2).sum(2)
        seen = set()
        for i, (row, qi, which, dist, partner_dot) in enumerate(plants):
            t = (qi % (32 * qt)) // 32
            assert dist in (radius, radius + 1) and d2[row, qi] == dist and t % 2 == (which == "second")
            assert full[row, i] == (dist if within else dist + 128)
            if which == "both":
                assert d2[row, qi + 32] == dist
            else:
                partner = qi + 32 if which == "first" else qi - 32
                assert d2[row, partner] == (0 if partner_dot > 0 else 128)
            seen.add((t // 2, (row % rpt) // 32, (row >> 2) & 1, which, dist - radius, partner_dot))
        ls = FC.loop_steps(tiles[0])
        last = qt // 2 - 1
        for s in (0, 1, ls - 1):                               # the carried pair: every variant, in every place it is carried from
            assert {(w, d) for p, st, _, w, d, _ in seen if p == last and st == s} == {(w, d) for w in ("first", "second", "both") for d in (0, 1)}
            assert {h for p, st, h, _, _, _ in seen if p == last and st == s} == {0, 1}
        assert {p for p, _, _, _, _, _ in seen} == set(range(qt // 2))
        assert {(w, d, pd) for _, _, _, w, d, pd in seen if w != "both"} == {(w, d, pd) for w in ("first", "second") for d in (0, 1) for pd in (128, -128)}
        if not within:                                         # nothing within the radius; the plants at the radius are what goes on
            assert int(np.unpackbits(desc[:, None, :] ^ q[None, ::7, :], axis=2).sum(2).min()) > radius
            tested, passed = FC.split_counts(desc, q, qt, radius)
            assert tested == sum(FC.loop_steps(t) for t in tiles) * qt * ((len(q) + 32 * qt - 1) // (32 * qt)) and passed > 0


def child(qt, pairs):
    env = dict(os.environ, TODHIP_K4X_FP4_ROWS="1", TODHIP_K4X_QT=str(qt), TODHIP_K4X_PAIRS=str(pairs))
    return subprocess.run([sys.executable, os.path.join(HERE, "pairs_child.py")], env=env, capture_output=True, text=True, timeout=600)


@pytest.mark.gpu
@pytest.mark.parametrize("qt", [6, 4])
def test_pairs_equal_the_vector_engine_and_the_single_block_step(qt):
    answers = {}
    for pairs in (1, 0):
        p = child(qt, pairs)
        assert p.returncode == 0 and p.stdout.startswith("ok "), (pairs, p.stdout[-2000:] + p.stderr[-4000:])
        answers[pairs] = p.stdout.split()[1:]
    assert int(answers[1][0]) == len(FC.ROWS) * len(PC.RADII) * 2 + 4
    assert answers[1] == answers[0]
