"""Keeps the inputs of tests/test_l2_numerics_gpu.py honest without a GPU. A numpy model of the float matcher's filter -- bf16 round to
nearest even, the dot product in binary64, eps(q), the threshold A_k + 2 eps (or seed + 2 eps where the one-GEMM path takes the
sample's seed) -- says per adversarial case that
  * the oracle's answer is the planted true neighbours,
  * with the constant as it stood before the correction, 2^-7 (1 + 2^-6), the filter DROPS them (the case discriminates), and
  * with the library's eps it keeps them. The library's eps is not restated here: tests/l2_bound_host_test.cpp, which includes
    tod_amd/csrc/l2_bound.h, prints it for given norms, and prints what l2_plan decides about the sample."""
import subprocess

import numpy as np
import pytest

import l2_numerics_cases as K
import match_l2_radius_ref as R
import oracle_lib as O
from test_l2_bound_cpu import build_host_test

OLD_LEAD, SUM = np.float32(0.0079345703125), np.float32(6.103515625e-05)     # eps before the correction: 2^-7 (1 + 2^-6), 2^-14


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_host_test(str(tmp_path_factory.mktemp("l2_numerics") / "l2_bound_host_test"))


# ------------------------------------------------------------------------------------------------------ the filter model
def bf16(x):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((b + 0x7FFF + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) << np.uint64(16)).astype(np.uint32).view(np.float32)


def norm2_f32(x):
    """|row|^2 in binary32 in the prepare kernel's order: a lane's two dimensions, then six butterfly steps"""
    x = np.asarray(x, np.float32)
    with np.errstate(under="ignore"):
        s = x[:, 0::2] * x[:, 0::2] + x[:, 1::2] * x[:, 1::2]
        for off in (32, 16, 8, 4, 2, 1):
            s = s + s[:, np.arange(64) ^ off]
    return s[:, 0]


def scores(desc, q):
    """f64[nq, n]: |r|^2 - 2 <q^, r^>, the bf16 products exact"""
    d = np.asarray(desc, np.float64)
    return (d * d).sum(axis=1)[None, :] - 2.0 * bf16(q).astype(np.float64) @ bf16(desc).astype(np.float64).T


def eps_library(exe, qn2, rmax2):
    args = [a for n2 in qn2 for a in (float(n2).hex(), float(rmax2).hex())]
    out = subprocess.run([exe, "--eps"] + args, capture_output=True, text=True, check=True)
    return np.array([float.fromhex(s) for s in out.stdout.split()])


def eps_old(qn2, rmax2):
    nq, rmax = np.sqrt(qn2.astype(np.float32)), np.sqrt(np.float32(rmax2))
    return (OLD_LEAD * nq * rmax + SUM * (nq + rmax) * (nq + rmax)).astype(np.float64)


def plan(exe, n, nq, k, n_cu):
    out = subprocess.run([exe, "--plan", str(n), str(nq), str(k), str(n_cu)], capture_output=True, text=True, check=True)
    return {name: float(v) for name, v in (line.split() for line in out.stdout.splitlines())}


def kth_smallest(s, k):
    return np.partition(s, k - 1, axis=1)[:, k - 1]


def sample_seed(sc, P, k):
    """the one-GEMM path's seed: the k-th smallest of the minima of the sample's partitions (seed chunk x lane half; the half of
    row rho of a tile is bit 2 of rho, l2_gemm.h's register-to-row map)"""
    stride, s_tpc, rows = int(P["sample_stride"]), int(P["s_tpc"]), int(P["tile_rows"])
    minima = []
    for chunk in range(int(P["s_used"])):
        tiles = np.arange(chunk * s_tpc, min((chunk + 1) * s_tpc, int(P["sample_tiles"]))) * stride
        r = (tiles[:, None] * rows + np.arange(rows)[None, :]).ravel()
        for h in (0, 1):
            minima.append(sc[:, r[((r >> 2) & 1) == h]].min(axis=1))
    return kth_smallest(np.stack(minima, axis=1), k)


def check_case(exe, c, base=None):
    """base(scores) -> what the threshold is built on, per query: A_k by default"""
    qn2, rmax2 = norm2_f32(c.q), norm2_f32(c.desc).max()
    sc = scores(c.desc, c.q)
    a_k = kth_smallest(sc, c.k) if base is None else base(sc)
    # the oracle: the planted rows, nearest first, for every adversarial query
    rc, rp, m, _ = O.l2_match(c.desc, c.off, c.pts, c.q, c.k, K.NO_CUT)
    assert rc == 0 and (np.diff(rp.astype(np.int64)) == c.k).all()
    rows = (c.off[m["imgIdx"]].astype(np.int64) + m["trainIdx"]).reshape(len(c.q), c.k)
    d = m["distance"].reshape(len(c.q), c.k)
    old, new = eps_old(qn2, rmax2), eps_library(exe, qn2, rmax2)
    for qi in c.adversarial:
        assert list(rows[qi]) == list(c.highs), (c.name, qi)
        assert (np.diff(d[qi]) > 0).all()                                     # pairwise distinct
        kept_old = sc[qi, c.highs] <= a_k[qi] + 2 * old[qi]
        kept_new = sc[qi, c.highs] <= a_k[qi] + 2 * new[qi]
        assert not kept_old.any(), (c.name, qi, "the old constant keeps a true neighbour: the case does not discriminate")
        assert kept_new.all(), (c.name, qi)
        # not by a hair: the margins are far above what the matrix cores' f32 accumulation can move a score (2^-15.9 (|q| + Rmax)^2)
        noise = 2.0 ** -15 * (np.sqrt(float(qn2[qi])) + np.sqrt(float(rmax2))) ** 2
        assert (sc[qi, c.highs] - a_k[qi] - 2 * old[qi] > 8 * noise).all() and (a_k[qi] + 2 * new[qi] - sc[qi, c.highs] > 8 * noise).all()
    return sc, a_k, new, qn2, rmax2


# ------------------------------------------------------------------------------------------------------ the cases
def test_the_model_reproduces_the_construction_numbers():
    """d2 253.97261 and 254.97258, errors -1.976 and +1.976, eps before the correction 1.043, score gap 2.953"""
    q, highs, lows = K.planted(1)
    assert abs(float(K.d2_f32(q, highs[0])) - 253.97261) < 1e-4 and abs(float(K.d2_f32(q, lows[0])) - 254.97258) < 1e-4
    sc = scores(np.stack([highs[0], lows[0]]), q[None, :])[0]
    n2 = float((q.astype(np.float64) ** 2).sum())
    exact = [float(((q.astype(np.float64) - r) ** 2).sum()) for r in (highs[0], lows[0])]
    assert abs(sc[0] + n2 - exact[0] - 1.976) < 1e-3 and abs(sc[1] + n2 - exact[1] + 1.976) < 1e-3
    assert abs(eps_old(norm2_f32(q[None, :]), norm2_f32(lows).max())[0] - 1.043) < 1e-3 and abs(sc[0] - sc[1] - 2.953) < 1e-3


@pytest.mark.parametrize("scale_exp", [0, -20, 20, -34, 28])
@pytest.mark.parametrize("n", [64, 2100])
def test_triple_k1(exe, n, scale_exp):
    """also the placement: no filler has a larger norm than the planted rows (Rmax, and with it eps, is theirs) and every filler is at
    least 16 eps farther from the query than the decoy"""
    c = K.adversarial_case(n, 1, scale_exp)
    sc, a_k, eps, qn2, rmax2 = check_case(exe, c)
    norms = norm2_f32(c.desc)
    filler = np.setdiff1d(np.arange(n), np.r_[c.highs, c.lows])
    assert norms[filler].max() <= norms[np.r_[c.highs, c.lows]].min()
    qi = c.adversarial[0]
    dd = R.d2(c.desc, c.q[qi:qi + 1])[0].astype(np.float64)
    assert dd[filler].min() >= dd[c.lows[0]] + 16 * eps[qi]
    lo, hi = (2.0 ** -64, 2.0 ** 64)                                          # the documented domain (include/todhip.h)
    assert lo <= min(norms.min(), qn2.min()) and max(norms.max(), qn2.max()) <= hi


@pytest.mark.parametrize("k", range(2, 9))
def test_k_true_neighbours_behind_k_decoys(exe, k):
    check_case(exe, K.adversarial_case(2100, k))


@pytest.fixture(scope="module")
def one_gemm_filler():
    return K.one_gemm_filler()


@pytest.mark.parametrize("k", [1, 2])
def test_one_gemm_path_placement(exe, one_gemm_filler, k):
    """the evenly spaced sample must hold k decoys in k partitions, or its seed is loose and hides the failure; and no candidate
    list may overflow into the exact scan, which would hide it too"""
    c = K.one_gemm_case(k, one_gemm_filler)
    for n_cu in (256, 304, 64):
        P = plan(exe, len(c.desc), len(c.q), k, n_cu)
        assert P["one_gemm"] == 1 and P["margin"] == 2
        assert (P["tile_rows"], P["sample_stride"], P["sample_tiles"]) == (K.TILE_ROWS, K.SAMPLE_STRIDE, K.SAMPLE_TILES)
        in_sample = (c.lows // K.TILE_ROWS) % K.SAMPLE_STRIDE == 0
        assert in_sample.all() and not ((c.highs // K.TILE_ROWS) % K.SAMPLE_STRIDE == 0).any()
        sc, seed, eps, _, _ = check_case(exe, c, base=lambda s: sample_seed(s, P, k))
        for qi in c.adversarial:
            assert seed[qi] == kth_smallest(sc, k)[qi]                        # as tight as pass 1 would make it
            candidates = int((sc[qi] <= seed[qi] + 2 * eps[qi]).sum())
            assert candidates == 2 * k and candidates < P["cand_cap"] / 8     # the planted rows alone: nothing overflows
        others = np.setdiff1d(np.arange(len(c.q)), c.adversarial)
        assert ((sc[others] <= (seed + 2 * eps)[others, None]).sum(axis=1) < P["cand_cap"] / 2).all()
    assert plan(exe, K.ONE_GEMM_ROWS - K.TILE_ROWS, len(c.q), k, 256)["one_gemm"] == 0    # one tile less: the classic path


def test_radius_case_reference_equals_the_oracle():
    """the radius between the two planted distances takes the true neighbour alone; the radius ON its distance takes it too"""
    c, radii = K.radius_case()
    keys = O.l2_knn_keys(c.desc, c.q, len(c.desc))
    d2 = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    for radius in radii:
        got = R.match_l2_radius(c.desc, c.off, c.pts, c.q, radius, 4)
        rc, rp, m, xyz = O.l2_match(c.desc, c.off, c.pts, c.q, 4, radius)
        assert rc == 0 and np.array_equal(got[0], rp) and np.array_equal(got[2], xyz)
        for f in K.FIELDS:
            assert np.array_equal(got[1][f], m[f]), f
        assert np.array_equal(got[3], (~(np.sqrt(d2) > np.float32(radius))).sum(axis=1))
        for qi in c.adversarial:
            mine = got[1][got[1]["queryIdx"] == qi]
            assert got[3][qi] == 1 and list(c.off[mine["imgIdx"]].astype(np.int64) + mine["trainIdx"]) == [c.highs[0]]
    assert np.float32(radii[1]) ** 2 <= K.d2_f32(c.q[0], c.desc[c.highs[0]]) * (1 + 2.0 ** -22)    # on the distance, not beyond


@pytest.mark.parametrize("name", sorted(K.descriptor_classes()))
def test_descriptor_classes_are_what_they_say(name):
    desc, off, pts, q, radius = K.descriptor_classes()[name]
    assert desc.dtype == np.float32 and q.dtype == np.float32 and np.isfinite(desc).all() and np.isfinite(q).all()
    assert 64 <= len(desc) <= 2100 and len(q) <= 64 and off[-1] == len(desc) and (np.diff(off.astype(np.int64)) == 0).any()
    n2 = np.r_[norm2_f32(desc), norm2_f32(q)]
    assert ((n2 == 0) | ((n2 >= 2.0 ** -64) & (n2 <= 2.0 ** 64))).all()       # the documented domain
    inside = R.match_l2_radius(desc, off, pts, q, radius, 16)[3]
    if name != "zero_db":
        assert 0 < inside.sum() < len(q) * len(desc) and inside.min() < inside.max()      # the radius cuts
    if name in ("signed_unit", "rootsift", "rmax_row"):
        rows = np.delete(desc, 1000, 0) if name == "rmax_row" else desc
        assert np.abs(np.sqrt(norm2_f32(rows).astype(np.float64)) - 1).max() < 1e-5
        assert (desc < 0).any() != (name == "rootsift")
    if name == "dominant_coordinate":
        rest = np.delete(desc, 17, 1)
        assert (np.abs(desc[:, 17]) > 5e3 * np.sqrt((rest.astype(np.float64) ** 2).mean(axis=1))).all()
    if name == "zero_vectors":
        assert (norm2_f32(desc) == 0).sum() == 9 and (norm2_f32(q) == 0).sum() == 3
    if name == "negative_zeros":
        assert np.signbit(desc[desc == 0]).any() and np.signbit(desc[77]).all() and np.signbit(q[7]).all()
    if name == "rmax_row":
        # the eps band holds every row for every query: more than a candidate list takes
        qn2, rmax2 = norm2_f32(q), norm2_f32(desc).max()
        sc = scores(desc, q)
        band = 2 * eps_old(qn2, rmax2)                                        # even the narrower band of before
        assert ((sc <= kth_smallest(sc, 1)[:, None] + band[:, None]).sum(axis=1) > 2048).all()
