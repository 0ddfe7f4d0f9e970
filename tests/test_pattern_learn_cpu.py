"""todhip_pattern_learn_* without a GPU: the definition restated in tests/pattern_learn_ref.py, run on response rows that the CPU
restatement of ORB produces (oracle_lib.orb with candidate chunks as `pattern`: the property that defines the response matrix), the
built-in candidate enumeration, the shared inputs of the GPU test, and what the library answers before it touches a device."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import pattern_learn_ref as P
from tod_amd import capi


@pytest.fixture(scope="module")
def crafted():
    """(candidates, R u8 [549, N]) of the GPU test's inputs on the CPU ORB"""
    views = P.learn_views()
    cands = P.crafted_candidates()

    def orb(pat):
        return np.concatenate([O.orb(g, P.NF, P.LEVELS, P.SCALE, pattern=pat, mask=m)[2] for g, m in views])

    return cands, P.rows_from_orb(orb, cands)


def test_shared_inputs_reach_every_round(crafted):
    """What keeps the GPU test from passing vacuously: a few hundred keypoints, not a multiple of 32, the second view starting inside a
    64-bit piece, and every one of the six rounds accepting at least one test."""
    cands, R = crafted
    n_first = len(O.orb(P.learn_views()[0][0], P.NF, P.LEVELS, P.SCALE)[0])
    M, N = R.shape
    assert M == 256 + 256 + 37 and P.in_disc(cands)
    assert 200 <= N <= 600 and N % 32 != 0 and n_first % 64 != 0 and 0 < n_first < N
    chosen, round_of, per_round = P.select(R)
    print("keypoints %d (first view %d), accepted per round %s" % (N, n_first, per_round))
    assert all(n >= 1 for n in per_round) and sum(per_round) == 256
    assert len(set(chosen.tolist())) == 256 and list(round_of) == sorted(round_of)


def test_selection_meets_its_own_conditions(crafted):
    """The selection's result checked pair by pair in Python integers, not by running the walk again: a test accepted in rounds 1-4
    is below its round's threshold against everything accepted before it; round 5 holds only tests with v > 0 that fail even
    |corr| < 1 against something accepted in rounds 1-4; round 6 only constants; nothing with v > 0 is left out."""
    cands, R = crafted
    chosen, round_of, _ = P.select(R)
    M, N = R.shape
    rows = [int("".join(str(b) for b in R[c][::-1]), 2) for c in range(M)]
    ones = [bin(r).count("1") for r in rows]
    v = [o * (N - o) for o in ones]

    def below(a, c, s):
        g = abs(N * bin(rows[a] & rows[c]).count("1") - ones[a] * ones[c])
        return (g * g) << s < v[a] * v[c]

    early = [c for c, r in zip(chosen, round_of) if r <= 4]
    for i, (c, r) in enumerate(zip(chosen, round_of)):
        c = int(c)
        if r <= 4:
            assert v[c] > 0 and all(below(int(a), c, P.SHIFTS[r - 1]) for a in chosen[:i])
        elif r == 5:
            assert v[c] > 0 and not all(below(int(a), c, 0) for a in early)
        else:
            assert v[c] == 0
    left = set(range(M)) - set(chosen.tolist())
    assert all(v[c] == 0 for c in left)
    # first accepted: the largest v, the smallest index among equals
    assert int(chosen[0]) == min(range(M), key=lambda c: (-v[c], c))
    # what the rounds are for: the tests of round 1 are pairwise below 1/8 (exact above; as a float here)
    assert P.max_abs_corr(R, [c for c, r in zip(chosen, round_of) if r == 1]) < 0.125


def test_layouts():
    cands = P.crafted_candidates()
    chosen = np.arange(256, dtype=np.uint32)[::-1] + 100
    rank, matcher = P.layout(cands, chosen, P.ORDER_RANK), P.layout(cands, chosen, P.ORDER_MATCHER)
    assert np.array_equal(rank, cands[chosen])
    for r in (0, 31, 32, 63, 64, 127, 128, 255):
        assert np.array_equal(matcher[32 * P.E[r // 32] + r % 32], cands[chosen[r]])
    # ranks 0-127 occupy dwords 0, 4, 1, 5: what a 2-split block of the matrix-core matcher evaluates first
    assert sorted(set((32 * P.E[r // 32] + r % 32) // 32 for r in range(128))) == [0, 1, 4, 5]


def test_builtin_candidates():
    c = P.builtin_candidates()
    assert 256 <= len(c) <= 65536 and P.in_disc(c)
    assert np.all(c % 2 == 0) and len(np.unique(c, axis=0)) == len(c)
    d = c.astype(np.int64)
    assert np.all((d[:, 0] - d[:, 2]) ** 2 + (d[:, 1] - d[:, 3]) ** 2 >= 16)
    # G starts (-4, -12), (-2, -12), (0, -12): the first pair at distance >= 4 is (G[0], G[2])
    assert c[0].tolist() == [-4, -12, 0, -12] and c[-1].tolist() == [0, 12, 4, 12]
    # lexicographic in (i, j): the first point never moves backwards in (y, x) order
    key = d[:, 1] * 100 + d[:, 0]
    assert np.all(np.diff(key) >= 0)


def test_symbols_are_exported():
    L = capi.lib()
    for name in ("todhip_pattern_learn_begin", "todhip_pattern_learn_add_view", "todhip_pattern_learn_add_view_device",
                 "todhip_pattern_learn_finish", "todhip_pattern_learn_responses", "todhip_pattern_learn_free",
                 "todhip_pipeline_set_pattern"):
        assert name in capi.EXPORTS and hasattr(L, name), name
    assert C.sizeof(capi.PatternStats) == 32


def test_argument_errors_need_no_device():
    """Arguments are judged before anything touches a device or the (here absent) context."""
    L = capi.lib()
    h = C.c_void_p()
    good = P.crafted_candidates()

    def begin(cands, cap):
        return L.todhip_pattern_learn_begin(None, None if cands is None else cands.ctypes.data_as(C.c_void_p),
                                            C.c_uint32(0 if cands is None else len(cands)), C.c_uint32(cap), C.byref(h))

    assert begin(good[:255], 1000) == capi.EINVAL                       # M < 256
    outside = good.copy(); outside[300] = (12, 6, 0, 0)                 # 144 + 36 > 169
    assert begin(outside, 1000) == capi.EINVAL
    outside = good.copy(); outside[5] = (0, 0, -13, 1)
    assert begin(outside, 1000) == capi.EINVAL
    for cap in (0, 32769):
        assert begin(good, cap) == capi.EINVAL and begin(None, cap) == capi.EINVAL
    assert not h.value
    pat = np.zeros((256, 4), np.int8)
    for order in (-1, 2):
        assert L.todhip_pattern_learn_finish(None, None, C.c_int(order), pat.ctypes.data_as(C.c_void_p), None, None, None) == capi.EINVAL
    assert L.todhip_pipeline_set_pattern(None, pat.ctypes.data_as(C.c_void_p)) == capi.EINVAL
    L.todhip_pattern_learn_free(None, None)                             # a null learner is nothing to free
