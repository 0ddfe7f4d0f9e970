"""The verifier's speculative draw table (drawIndexSampleHelper, sac_model_registration_graph.h:102-132, started at every position of a
window of the rand() stream) through todhip_test_draw_table: every form of the kernel that can hold the object -- one lane per
position (two or eight words a lane), one wave per position with one or with eight slices -- entry for entry against the plain
statement of the helper below.
Sizes are those at which a form or a word count changes (65, 128 | 129, 300, 512 | 513, 4096 | 4097 matches); graphs: a dense
consistent subset (the first pick succeeds), a sparse random graph (second and third picks fail and are removed), a triangle-free
one (every position fails after |valid| + |E| draws), valid sets with an all-zero word in the middle or only their last word set,
and a window that ends right behind the table (the trailing positions overflow)."""
import functools

import numpy as np
import pytest

from tod_amd import capi

DRAW_FAIL, DRAW_OK, DRAW_OVERFLOW = 0, 1, 2
SIZES = [65, 128, 129, 300, 512, 513, 4096, 4097]
GRAPHS = ["dense", "sparse", "no_triangle", "hole", "last_word", "short_window"]
EXTRA = [(300, "one_position"), (129, "sparse_600")]


def reference_table(adj, valid, rnd, S):
    """valid_samples ascending; a pick is valid_samples[rand() % size] (:111); the next level is its intersection with the pick's
    sample neighbours (:113-117); a pick that leads nowhere is removed (:125-128); samples_ come out deepest first (:118-121)."""
    out = np.zeros((S, 6), np.uint32)
    for s in range(S):
        pos, status, trip = s, DRAW_FAIL, (0, 0, 0)
        A = list(np.flatnonzero(valid))
        while A and status == DRAW_FAIL:
            if pos >= len(rnd):
                status = DRAW_OVERFLOW
                break
            a = A[int(rnd[pos]) % len(A)]; pos += 1
            row = adj[a]
            B = [v for v in A if row[v]]
            while B:
                if pos >= len(rnd):
                    status = DRAW_OVERFLOW
                    break
                b = B[int(rnd[pos]) % len(B)]; pos += 1
                row = adj[b]
                C = [v for v in B if row[v]]
                if C:
                    if pos >= len(rnd):
                        status = DRAW_OVERFLOW
                        break
                    c = C[int(rnd[pos]) % len(C)]; pos += 1
                    status, trip = DRAW_OK, (c, b, a)
                    break
                B.remove(b)
            if status == DRAW_FAIL:
                A.remove(a)
        out[s] = (status, pos - s) + trip + (0,)
    return out


def _symmetric(rng, n, p):
    up = np.triu(rng.random((n, n), dtype=np.float32) < p, 1)
    return up | up.T


@functools.lru_cache(maxsize=None)
def case(n, graph):
    """-> (samp u64 [n, W], valid u64 [W], rnd u32 [window_len], S, the reference's entries); computed once, shared by the tests"""
    rng = np.random.default_rng(1000 * n + GRAPHS.index(graph) if graph in GRAPHS else 7 * n)
    W = (n + 63) // 64
    S, look = 200, 4096
    valid = rng.random(n) < 0.7
    if graph == "dense":                                        # 60 % of the valid matches agree with each other
        member = valid & (rng.random(n) < 0.6)
        adj = _symmetric(rng, n, 0.02) | (member[:, None] & member[None, :])
        S = 300
    elif graph == "no_triangle":                                # bipartite between two halves of 30 valid matches spread over the words
        valid = np.zeros(n, bool)
        valid[rng.choice(n, 30, replace=False)] = True
        side = np.zeros(n, bool)
        side[np.flatnonzero(valid)[::2]] = True
        adj = _symmetric(rng, n, 0.3) & (side[:, None] ^ side[None, :])
        S = 80
    else:                                                       # about one common neighbour of two adjacent matches in two
        if graph == "hole":
            valid[64 * (W // 2):64 * (W // 2 + 1)] = False      # an all-zero word in the middle
        if graph == "last_word":
            valid[:64 * (W - 1)] = False
            valid[64 * (W - 1):] = True
        nv = max(int(valid.sum()), 1)
        adj = _symmetric(rng, n, min(0.9, (0.6 / nv) ** 0.5))
        if graph == "last_word" and nv >= 3:                    # one triangle among the few matches of the last word
            v = np.flatnonzero(valid)[:3]
            adj[np.ix_(v, v)] = True
        S = {"sparse": 257, "short_window": 300, "one_position": 1, "sparse_600": 600}.get(graph, 200)
        if graph == "short_window":
            look = 1                                            # the last position cannot draw three
    adj[np.arange(n), np.arange(n)] = False
    rnd = rng.integers(0, 2 ** 31, S + look, dtype=np.uint32)   # rand() values
    bits = np.zeros((n, 64 * W), np.uint8)
    bits[:, :n] = adj
    samp = np.packbits(bits, axis=1, bitorder="little").view("<u8").reshape(n, W)
    vbits = np.zeros(64 * W, np.uint8)
    vbits[:n] = valid
    return samp, np.packbits(vbits, bitorder="little").view("<u8"), rnd, S, reference_table(adj, valid, rnd, S)


def forms_for(n):
    """(the form the routing names, every form that can hold n matches)"""
    if n <= 512:
        return 1, [1, 2, 3, 4]                                  # 4: the eight-word lane kernel also on one or two words
    return (2, [2, 3]) if n <= 4096 else (3, [3])


def test_reference_meets_every_outcome():
    """Conditions on the inputs, not measurements: over these cases the plain statement itself ends attempts in all three ways and
    removes failed picks (an attempt of more than three draws)."""
    seen, long_ok, long_any = set(), 0, 0
    for n in (65, 129, 300):                                    # (the small sizes: enough, and quick without a GPU)
        for g in GRAPHS:
            ref = case(n, g)[4]
            seen |= set(int(x) for x in ref[:, 0])
            long_ok += int(((ref[:, 0] == DRAW_OK) & (ref[:, 1] > 3)).sum())
            long_any += int((ref[:, 1] > 3).sum())
    assert seen == {DRAW_FAIL, DRAW_OK, DRAW_OVERFLOW}
    assert long_ok > 0 and long_any > long_ok                   # successful attempts with removed picks, and failed ones


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,graph", [(n, g) for n in SIZES for g in GRAPHS] + EXTRA)
def test_every_form_writes_the_reference_entries(ctx, n, graph):
    samp, valid, rnd, S, ref = case(n, graph)
    routed, forms = forms_for(n)
    if graph == "dense":
        assert (ref[:, 0] == DRAW_OK).mean() > 0.9
    if graph == "no_triangle":
        assert (ref[:, 0] == DRAW_FAIL).all() and (ref[:, 1] > 30).all()
    if graph == "short_window":
        assert ref[-1, 0] == DRAW_OVERFLOW
    got = {}
    for form in [0] + forms:
        rc, got[form] = ctx.test_draw_table(samp, valid, n, rnd, S, form)
        assert rc == capi.OK, form
        bad = np.flatnonzero((got[form] != ref).any(axis=1))
        assert len(bad) == 0, (form, bad[:5], got[form][bad[:5]], ref[bad[:5]])
    assert np.array_equal(got[0], got[routed])
    for form in (1, 2, 3, 4):                                   # a form that cannot hold the object is refused
        if form not in forms:
            assert ctx.test_draw_table(samp, valid, n, rnd, S, form)[0] == capi.EINVAL
