"""The hypothesis gate after its register diet (eval_kernel<false, ...> at <= 112 registers, tests/test_verify_regs_build.py), at the
smallest shapes where such a diet can go wrong, against the CPU oracle. Everything is compared exactly.

The clique search of the narrow instantiation (clique_search<false, .>, what todhip_test_clique and todhip_test_clique_gate run for
graphs of up to 512 vertices) on candidate sets of kGateMinimal, kGateMinimal + 1, 63, 64, 65, 127, 128, 129, 511 and 512 vertices --
word boundaries of the one-slice bitsets and the 1-, 2- and 8-word forms of the colouring -- each as an empty graph, a complete one
(more than 64 colour classes from 65 vertices on: the two-set colouring whose row prefetch the diet removed), a random one at
density 0.5 and one whose only large clique ends the last word. Then eval_kernel<false> itself through todhip_test_consensus: random
hypotheses on an object of a few hundred matches, hypotheses whose graph needs the deferred pass's big LDS, and a corrupt draw-table
index, which must be reported without anything being dereferenced."""
import numpy as np
import pytest

import oracle_lib as O
from tod_amd import capi, synth
from test_verify_gpu import _clusters_of

pytestmark = pytest.mark.gpu
MINIMAL = 7                                            # kGateMinimal
SIZES = [MINIMAL, MINIMAL + 1, 63, 64, 65, 127, 128, 129, 511, 512]
EVAL_LDS_SMALL = 48 * 1024                             # kEvalLdsSmall: a graph beyond it is deferred to the big-LDS pass


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def graph(kind, m):
    if kind == "empty":
        return np.zeros((0, 2), np.uint32)
    if kind == "complete":
        return synth.random_graph_edges(m, 2.0, 0)
    if kind == "random":
        return synth.random_graph_edges(m, 0.5, 4000 + m)
    last = np.arange(max(0, m - 9), m)                 # the last 9 vertices (all of them below 9): a clique that ends the last word
    iu = np.triu_indices(len(last), 1)
    return np.stack([last[iu[0]], last[iu[1]]], axis=1).astype(np.uint32)


@pytest.mark.parametrize("m", SIZES)
def test_narrow_search_and_gate_on_boundary_sizes(ctx, m):
    for kind in ("empty", "complete", "random", "last_word"):
        edges = graph(kind, m)
        o_size, _, _, o_steps = O.clique(m, edges, minimal_size=MINIMAL)
        size, err, steps = ctx.test_clique(m, edges, MINIMAL)
        print("m %d %s: search size %d steps %d (oracle %d %d) err %d" % (m, kind, size, steps, o_size, o_steps, err))
        assert (size, steps, err) == (o_size, o_steps, 0), (kind, m)
        g_size, g_err, g_steps = ctx.test_clique(m, edges, MINIMAL, gate=True)
        print("m %d %s: gate size %d steps %d" % (m, kind, g_size, g_steps))
        assert g_err == 0 and (g_size > MINIMAL) == (o_size > MINIMAL), (kind, m)
        if o_size < MINIMAL:                           # no leaf ever reaches the minimal size: the gate is the search as it is
            assert (g_size, g_steps) == (o_size, o_steps), (kind, m)
        elif o_size == MINIMAL:                        # it stops at that leaf and leaves out the reference's unwinding
            assert g_size == o_size and g_steps <= o_steps, (kind, m)
        else:                                          # decided early: a lower bound, in no more steps
            assert MINIMAL < g_size <= o_size and g_steps <= o_steps, (kind, m)


def gate_lds_bytes(m):                                 # verify_clique.h
    mw, ma = (m + 63) // 64, (m + 7) & ~3
    return 8 * m * mw + 8 * mw + 8 * 4 * ma + 4 * 2 * ma + 256 + 64


@pytest.fixture(scope="module")
def objects():
    """(train, query, kp of each match, span, oracle cluster, a dozen drawn triples) of an object of ~490 matches, 190 of them true,
    and of one of ~500 matches, nearly all of them consistent: its hypotheses' graphs do not fit the first pass's LDS"""
    out = {}
    for name, (n_kp, per_object, frac, per_kp, seed) in {"mid": (450, 400, 0.40, 5, 41), "big": (580, 600, 0.95, 1, 42)}.items():
        sc = synth.make_verify_scene(n_kp, per_object=per_object, visible=((1, frac),), matches_per_kp=per_kp, seed=seed)
        t, q, qi = _clusters_of(sc)[1]
        assert 64 < len(qi) <= 512, len(qi)            # eval_kernel<false>
        cl = O.Cluster(t, q, qi)
        cl.fill(sc["kp_xy"], float(sc["spans"][1]), 0.01)
        rng = O.rng_new(1)
        triples = np.array([cl.draw(rng) for _ in range(12)], np.uint32)
        out[name] = (t, q, sc["kp_xy"][qi], float(sc["spans"][1]), cl, triples)
    return out


@pytest.mark.parametrize("name", ["mid", "big"])
def test_hypotheses_equal_the_oracle(ctx, objects, name):
    t, q, kp, span, cl, triples = objects[name]
    counts, dbg = ctx.test_consensus(t, q, kp, span, 0.01, triples, dbg_stride=16)
    want = [len(cl.consensus(tr)[0]) for tr in triples]
    print(name, "n", len(t), "counts", counts.tolist(), "oracle", want, "m", dbg[:, 1].tolist(), "steps", dbg[:, -3].tolist())
    assert counts.tolist() == want
    plain, _ = ctx.test_consensus(t, q, kp, span, 0.01, triples)     # and without the diagnostics' stores
    assert plain.tolist() == want
    deferred = [int(m) for m in dbg[:, 1] if gate_lds_bytes(int(m)) > EVAL_LDS_SMALL]
    if name == "big":
        assert deferred and any(c > 0 for c in want), "no hypothesis of this object took the deferred pass"
    else:
        assert not deferred and any(c > 0 for c in want) and any(int(m) > 64 for m in dbg[:, 1])


def test_corrupt_draw_table_index_is_reported(ctx, objects):
    t, q, kp, span, cl, triples = objects["mid"]
    bad = triples.copy()
    bad[5, 1] = len(t)                                 # one past the object's last match
    bad[7, 0] = 0xFFFFFFF0
    with pytest.raises(capi.TodError):
        ctx.test_consensus(t, q, kp, span, 0.01, bad)
    counts, _ = ctx.test_consensus(t, q, kp, span, 0.01, triples)    # the context is as good as before
    assert counts.tolist() == [len(cl.consensus(tr)[0]) for tr in triples]
