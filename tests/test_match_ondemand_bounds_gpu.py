"""The paired split-2 step of hamming_topk_fp4rows (tod_amd/csrc/match_fp4rows.h) exchanges the tiles' distance bounds where a
block goes on (fp4rows_pair_complete) instead of every TODHIP_K4X_SHARE steps in the loop. tests/ondemand_bounds_cases.py plants, for
every third query, rows that make that exchange matter: k + 1 rows within the radius in each of three tiles with distances falling and
rising from tile to tile, a tie between two tiles at a full list's bound, a row at exactly the radius and one beyond it, rows in the
last partial step of a tile and for the blocks of a step's carried last pair. First on the CPU: what the construction claims. Then on
the GPU (tests/ondemand_bounds_child.py, a child per set of knobs, all started together): split 2 forced, TODHIP_K4X_WAVES_PER_CU
raised, 380 queries at six blocks per wave and 250 at four, k 2 and 5, radius 35; counts, matches and xyz bit for bit the vector
engine's and the definition's in every child, and the same digest from the paired step, the single-block step (TODHIP_K4X_PAIRS=0) and
the packed-rows pass (TODHIP_K4X_FP4_ROWS=0), with TODHIP_K4X_SHARE at 2 and at 1000000.

The counters of blocks tested and blocks that went on: the paired step tests at the launch's radius, so its count does not depend on any
threshold and equals the CPU's (fastpath_cases.split_counts) even with rows inside the radius, at either TODHIP_K4X_SHARE -- it ignores
the knob. The single-block forms test against each query's tightened threshold and still honour the knob: a threshold is the maximum
of what the own list and the foreign bounds give and only rises with more exchanges, so went-on(share 2) <= went-on(share 1000000) <=
the paired step's count, on the same blocks tested (with share 2 the count depends on which tile published first)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fastpath_cases as FC
import ondemand_bounds_cases as OC

HERE = os.path.dirname(os.path.abspath(__file__))
KS = (2, 5)


def tile_of(row, n_rows):
    return row // FC.tiling(n_rows)[0]


@pytest.mark.parametrize("qt", [6, 4])
def test_the_construction_is_what_it_claims(qt):
    for n_rows in OC.ROWS:
        rpt, tiles = FC.tiling(n_rows)
        assert len(tiles) >= 8
        for k in KS:
            desc, pts, off, q, plants = OC.make(n_rows, qt, k, 7 * n_rows + k)
            nq = len(q)
            assert nq == OC.nq_of(qt) and (nq + 32 * qt - 1) // (32 * qt) == 2 and nq % 32 != 0
            d = OC.distances(desc, q)
            ans = OC.knn(desc, q, k, OC.RADIUS)
            by_q = {}
            for row, qi, kind, dist in plants:
                assert d[row, qi] == dist
                by_q.setdefault(qi, []).append((row, kind, dist))
            assert sorted(by_q) == list(range(0, nq, 3))
            assert all(len(ans[qi]) == 0 for qi in range(nq) if qi not in by_q)        # random rows are far from every query
            kinds, carried, partial_step = set(), set(), 0
            for qi, pl in by_q.items():
                kind = pl[0][1]
                kinds.add(kind)
                t = (qi % (32 * qt)) // 32
                if t >= qt - 2:
                    carried.add(kind)
                ts = sorted({tile_of(r, n_rows) for r, _, _ in pl})
                got_tiles = [tile_of(r, n_rows) for _, r in ans[qi]]
                if kind in ("falling", "rising"):
                    assert len(ts) == 3 and all(sum(tile_of(r, n_rows) == tt for r, _, _ in pl) == k + 1 for tt in ts)
                    assert max(dd for _, _, dd in pl) < OC.RADIUS
                    assert got_tiles == [ts[2] if kind == "falling" else ts[0]] * k
                elif kind == "tie":
                    ties = sorted(r for r, _, dd in pl if dd == OC.TIE_D)
                    assert len(ties) == 2 and tile_of(ties[0], n_rows) != tile_of(ties[1], n_rows)
                    assert len(ans[qi]) == k and ans[qi][-1] == (OC.TIE_D, ties[0])
                else:
                    at = [r for r, _, dd in pl if dd == OC.RADIUS]
                    assert sorted(dd for _, _, dd in pl) == [OC.RADIUS, OC.RADIUS + 1] and ans[qi] == [(OC.RADIUS, at[0])]
                    last = len(tiles) - 1
                    if tiles[-1] % 32 and at[0] >= last * rpt + tiles[-1] - tiles[-1] % 32:
                        partial_step += 1
            assert kinds == set(OC.KINDS) and carried == set(OC.KINDS)
            # the tie's full list stands in the earlier tile for some queries and in the later one for others
            order = set()
            for qi, pl in by_q.items():
                if pl[0][1] == "tie":
                    full = tile_of(pl[0][0], n_rows)
                    other = [tile_of(r, n_rows) for r, _, _ in pl if tile_of(r, n_rows) != full][0]
                    order.add(full < other)
            assert order == {True, False}
            assert (partial_step > 0) == (n_rows % 32 != 0)
    assert any(n % 32 for n in OC.ROWS)


FORMS = {"pairs": dict(PAIRS="1", SHARE="2"), "pairs_noshare": dict(PAIRS="1", SHARE="1000000"),
         "single": dict(PAIRS="0", SHARE="2"), "single_noshare": dict(PAIRS="0", SHARE="1000000"),
         "packed": dict(PAIRS="1", SHARE="2", FP4_ROWS="0")}


def start(qt, knobs, *args):
    env = dict(os.environ, TODHIP_K4X_FP4_ROWS="1", TODHIP_K4X_QT=str(qt), TODHIP_K4X_WAVES_PER_CU="32")
    env.update({"TODHIP_K4X_" + key: v for key, v in knobs.items()})
    return subprocess.Popen([sys.executable, os.path.join(HERE, "ondemand_bounds_child.py")] + list(args), env=env,
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def finish(p, what):
    out, err = p.communicate(timeout=600)
    assert p.returncode == 0 and out.startswith("ok "), (what, out[-2000:] + err[-4000:])
    return out.split()[1:]


@pytest.mark.gpu
@pytest.mark.parametrize("qt", [6, 4])
def test_bounds_exchanged_on_demand_change_no_answer(qt):
    procs = {name: start(qt, knobs) for name, knobs in FORMS.items()}
    out = {name: finish(p, name) for name, p in procs.items()}
    digests = {name: o[0] for name, o in out.items()}
    assert len(set(digests.values())) == 1, digests
    cnt = {name: [tuple(int(x) for x in c.split(":")) for c in o[1:]] for name, o in out.items()}
    cases = [(n_rows, k) for n_rows in OC.ROWS for k in KS]
    assert all(len(c) == len(cases) for c in cnt.values())
    for i, (n_rows, k) in enumerate(cases):
        desc, pts, off, q, plants = OC.make(n_rows, qt, k, 7 * n_rows + k)
        tested, went_on = FC.split_counts(desc, q, qt, OC.RADIUS)
        print("%d rows, k %d: CPU tested %d went on %d; device %s" % (n_rows, k, tested, went_on, {n: c[i] for n, c in cnt.items()}))
        rpt, tiles = FC.tiling(n_rows)
        blocks = {(row // 32, qi // 32) for row, qi, _, dist in plants
                  if dist <= OC.RADIUS and (row % rpt) // 32 < FC.loop_steps(tiles[row // rpt])}
        assert went_on >= len(blocks) > 100                    # every planted row within the radius sends its block on
        assert cnt["pairs"][i] == (tested, went_on) and cnt["pairs_noshare"][i] == (tested, went_on)
        for name in ("single", "single_noshare", "packed"):
            assert cnt[name][i][0] == tested, name
        assert cnt["single"][i][1] <= cnt["single_noshare"][i][1] <= went_on
        assert cnt["packed"][i][1] <= went_on


@pytest.mark.gpu
def test_selected_objects_and_shards_take_the_same_step():
    assert finish(start(6, dict(PAIRS="1", HALF="2"), "extras"), "extras") == ["extras"]
