"""The float matcher on the GPU where its bf16 filter is as wrong as it can be, and on descriptor classes the rest of the suite never
loads (tests/l2_numerics_cases.py; tests/test_l2_numerics_cpu.py shows on a model of the filter that every adversarial case loses its
true neighbours under an eps that allows less than bf16 rounding can do). Every field of todhip_match_l2's result equals the oracle's
(oracle/l2_oracle.c), every field of todhip_match_l2_radius's the numpy statement of its definition (tests/match_l2_radius_ref.py),
bit for bit. DBs have 64 to 2 100 rows except where the one-GEMM path needs 65 536; at most 64 queries; ragged objects, one empty."""
import numpy as np
import pytest

import l2_numerics_cases as K
import match_l2_radius_ref as R
import oracle_lib as O
from tod_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def assert_same(ctx, desc, pts, off, q, k, radius=K.NO_CUT):
    """tests/test_l2_gpu.py's comparison: (row_ptr, matches) of the call, equal to the oracle's in every field"""
    row_ptr, m, xyz = ctx.match_l2(q, k, radius)
    rc, o_row_ptr, o_m, o_xyz = O.l2_match(desc, off, pts, q, k, radius)
    assert rc == 0
    assert np.array_equal(row_ptr, o_row_ptr)
    for f in K.FIELDS:
        assert np.array_equal(m[f], o_m[f]), f                               # distance: sqrtf of the same sequential f32 sum
    assert np.array_equal(xyz, o_xyz)
    return row_ptr, m


def assert_radius_same(ctx, desc, pts, off, q, radius, mpq):
    got = ctx.match_l2_radius(q, radius, mpq)
    want = R.match_l2_radius(desc, off, pts, q, radius, mpq)
    assert np.array_equal(got[0], want[0])
    for f in K.FIELDS:
        assert np.array_equal(got[1][f], want[1][f]), f
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    return got


def run_adversarial(ctx, c):
    ctx.db_load(c.desc, c.pts, c.off)
    row_ptr, m = assert_same(ctx, c.desc, c.pts, c.off, c.q, c.k)
    rows = (c.off[m["imgIdx"]].astype(np.int64) + m["trainIdx"]).reshape(len(c.q), c.k)
    for qi in c.adversarial:
        assert list(rows[qi]) == list(c.highs), (c.name, qi, "the decoys' rows are %s" % list(c.lows))


@pytest.mark.parametrize("scale_exp", [0, -20, 20])
@pytest.mark.parametrize("n", [64, 2100])
def test_the_triple_returns_the_true_nearest_row(ctx, n, scale_exp):
    """k = 1: the true nearest row scores 1.976 too high, a decoy 1.0 farther away 1.976 too low -- a gap of 2.95 against a band
    that used to be 2.09. The classic path (pass 1's A_1 is the decoy's score), two DB sizes, three scales."""
    run_adversarial(ctx, K.adversarial_case(n, 1, scale_exp))


@pytest.mark.parametrize("scale_exp", [-34, 28])
def test_the_triple_at_the_edges_of_the_documented_domain(ctx, scale_exp):
    """squared norms between 2^-64 and 2^64 (include/todhip.h): here 2^-64.4 ... 2^-61 and 2^61.6 ... 2^63"""
    run_adversarial(ctx, K.adversarial_case(64, 1, scale_exp))


@pytest.mark.parametrize("k", range(2, 9))
def test_k_true_neighbours_behind_k_decoys(ctx, k):
    run_adversarial(ctx, K.adversarial_case(2100, k))


@pytest.fixture(scope="module")
def one_gemm_filler():
    return K.one_gemm_filler()


@pytest.mark.parametrize("k", [1, 2])
def test_the_one_gemm_path_keeps_them_too(ctx, one_gemm_filler, k):
    """65 536 rows: the sample's seed is the threshold's base. The decoys sit in k partitions of the sample, so the seed is as tight
    as pass 1 would make it, and only the planted rows are candidates: nothing reaches the exact scan."""
    run_adversarial(ctx, K.one_gemm_case(k, one_gemm_filler))


def test_the_radius_search_on_the_triple(ctx):
    """The radius between the two planted distances, and exactly on the true neighbour's: in_radius and the matches are the
    definition's. The radius path needs the one-sided bound only and has a second eps of slack (l2_radius.h), so this held before
    the bound was corrected, too: it pins that the slack is real."""
    c, radii = K.radius_case()
    ctx.db_load(c.desc, c.pts, c.off)
    for radius in radii:
        for mpq in (1, 4):
            got = assert_radius_same(ctx, c.desc, c.pts, c.off, c.q, radius, mpq)
            for qi in c.adversarial:
                mine = got[1][got[1]["queryIdx"] == qi]
                assert got[3][qi] == 1 and list(c.off[mine["imgIdx"]].astype(np.int64) + mine["trainIdx"]) == [c.highs[0]]


CLASSES = K.descriptor_classes()


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_descriptor_classes(ctx, name):
    desc, off, pts, q, radius = CLASSES[name]
    ctx.db_load(desc, pts, off)
    for k in (1, 8):
        assert_same(ctx, desc, pts, off, q, k)
    assert_same(ctx, desc, pts, off, q, 8, radius)                           # the k-NN call's cut at the class's radius
    assert_radius_same(ctx, desc, pts, off, q, radius, 16)
