"""tests/orb_ref.py, the float64 / int64 statement of stage A, against the C restatement (oracle/orb_oracle.c) under the rules of
orb_ref.compare, against plain float64 resize and Gaussian blur, and against properties no implementation chooses (level composition,
transposition). Also pinned here, for every input tests/test_orb_ref_gpu.py uses: the selection has no ambiguous boundary and the
half-integer guard leaves out at most 0.5 % of the bits, so the GPU comparison is as strict as its rules read.

Measured on the restatement over all cases (profiles/orb_ref.json): response within 3.1 u M (bound 20), angle within 2.2e-5 degrees
(bound 4.9e-4), at most 0.065 % of an input's bits left out (bound 0.5 %) and none of those different, resize within 0.56 grey levels
of float64 bilinear (bound 1), blur within 1.33 of the float64 Gaussian (bound 5.4)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import orb_inputs as I
import orb_ref as R


def restatement(name):
    img, nf, nl, sf, kw = R.case_args(name)
    return O.orb(img, nf, nl, sf, **kw)


# ------------------------------------------------------------------------------------------ the documented choices
def test_pattern_geometry_and_weights_as_documented():
    pat = R.default_pattern()
    assert np.array_equal(pat, O.orb_default_pattern())
    p = pat.astype(np.int64).reshape(-1, 2)
    assert ((p * p).sum(axis=1) <= 169).all() and len({tuple(t) for t in pat.tolist()}) > 250
    # the disc's rows: symmetric, 709 pixels, every row end within a pixel of the circle of radius 15
    w = np.array(R.DISC_HALF_WIDTH)
    assert len(w) == 16 and (np.diff(w) <= 0).all() and len(R._disc()) == 31 + 2 * int((2 * w[1:] + 1).sum())
    assert (np.abs(np.hypot(w, np.arange(16)) - 15) < 1.0).all()
    # the blur's weights are the 8-bit roundings of a Gaussian of sigma 2, and the issue's sum of deviations
    g = R.gauss7()
    assert sum(R.GAUSS_8BIT) == 256 and (np.abs(np.array(R.GAUSS_8BIT) - 256 * g) < 0.75).all()
    assert abs(np.abs(np.array(R.GAUSS_8BIT) / 256 - g).sum() * 256 - 2.22) < 0.01
    L = O.lib()
    for H, W, nl, sf, nf in ((160, 200, 4, 1.2, 150), (160, 200, 4, 1.2, 300), (100, 100, 9, 2.0, 50), (480, 640, 8, 1.5, 64),
                             (1080, 1920, 16, 1.2, 2000), (160, 200, 3, 1.2, 1), (100, 130, 2, 1.2, 150)):
        per = (C.c_uint32 * nl)()
        L.orb_features_per_level(C.c_uint32(nf), C.c_uint32(nl), C.c_float(sf), per)
        assert list(per) == R.quotas(nf, nl, sf)
        for lvl in range(nl):
            h, w_, s = C.c_uint32(), C.c_uint32(), C.c_float()
            L.orb_level_size(C.c_uint32(H), C.c_uint32(W), C.c_float(sf), C.c_uint32(lvl), C.byref(h), C.byref(w_), C.byref(s))
            assert (h.value, w_.value) == R.level_size(H, W, lvl, sf) and np.float32(s.value) == R.level_scale(lvl, sf)


def test_pattern_domain():
    sq = R.square_pattern()
    p = sq.astype(np.int64).reshape(-1, 2)
    assert R.in_domain(sq) and ((p * p).sum(axis=1) == 900).sum() >= 6 and (np.abs(p).max(axis=1) == 15).sum() >= 6
    assert R.in_domain(R.default_pattern()) and len(R.bad_patterns()) == 4
    assert not any(R.in_domain(b) for b in R.bad_patterns().values())
    # a rotation keeps a point's distance (<= 30) and rounding half to even does not exceed it: with the 31-pixel border every test
    # of the reference's run with the square pattern read a pixel of its own level (numpy would have wrapped a negative index)
    th = np.linspace(0, 2 * np.pi, 100001)
    for x, y in ((30, 0), (18, 24), (15, 15), (0, -30), (-24, -18)):
        assert np.abs(np.rint(x * np.cos(th) - y * np.sin(th))).max() <= 30 < R.EDGE


# ------------------------------------------------------------------------------------------ against the restatement
EXPECTED_N = {"rect_150_1": 150, "rect_150_3": 150, "rect_300_3": 300, "rect_150_4": 150, "rect_300_4": 300, "rect_1_1": 1, "rect_1_3": 1,
              "rect_all_1": 265, "rect_T_all_1": 265, "rect_300_1": 265, "rect_masked": 150, "rect_square": 150, "rect200": 150,
              "flat200": 0, "rect200_T": 150, "noise": 150, "lattice": 100, "tiny63": 1, "tiny62x200": 0}


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_reference_against_restatement(name):
    ref = R.case_ref(name)
    s = R.compare(restatement(name), ref)
    print("%s: n %d, response %.2f u M, angle %.2e deg, left out %.5f" % (name, s["n"], s["response_err"], s["angle_err"], s["left_out"]))
    assert name not in EXPECTED_N or s["n"] == EXPECTED_N[name]
    # the conditions under which compare() decides everything: no keypoint may change sides, and nearly every bit is compared
    assert ref.ambiguous == []
    assert ref.left_out_share() <= R.LEFT_OUT_LIMIT


def test_every_gpu_input_is_a_case_and_reaches_its_path():
    assert set(R.GPU_CASES) <= set(R.CASES)
    assert {R.CASES[k][2] for k in R.GPU_CASES} >= {1, 3, 4} and {R.CASES[k][1] for k in R.GPU_CASES} >= {1, 150, R.MANY}
    ref = R.case_ref("rect_300_4")
    assert [L.level for L in ref.levels] == [0, 1, 2, 3] and all(L.n_kept == L.quota < len(L.x) for L in ref.levels)   # every level cuts
    assert [L.level for L in R.case_ref("rect_1_3").levels] == [2]                          # quotas 0, 0, 1
    x2 = R.case_ref("rect100_x2")
    assert [im.shape for im in x2.images] == [(100, 100), (50, 50), (25, 25)] and [L.level for L in x2.levels] == [0]
    for k in ("rect_all_1", "rect_T_all_1"):
        L, = R.case_ref(k).levels
        assert L.kept.all() and len(L.x) < R.MANY // 2                                      # nothing is cut, not even to 2 n
    # the lattice: exact Harris ties inside the selection and patches without a direction
    L0 = R.case_ref("lattice").levels[0]
    k = L0.kept
    assert (np.diff(L0.response[k]) == 0).sum() > 10 and ((L0.m10[k] == 0) & (L0.m01[k] == 0)).sum() > 5
    assert (L0.angle[k][(L0.m10[k] == 0) & (L0.m01[k] == 0)] == 0).all()
    # bits near a half-integer exist, so the guard is exercised
    assert sum(int(L.left_out[L.kept].sum()) for L in R.case_ref("rect_300_4").levels) > 10


def test_masked_case_uses_the_mask_rule():
    img, nf, nl, sf, kw = R.case_args("rect_masked")
    mask, ref = kw["mask"], R.case_ref("rect_masked")
    alone = [(x, y) for y, x in zip(*np.nonzero(mask == 255)) if not mask[y - 1:y + 2, x - 1:x + 2].sum() > 255]
    assert len(alone) == 1
    L0 = ref.levels[0]
    assert alone[0] in set(zip(L0.x.tolist(), L0.y.tolist()))                               # the isolated pixel's corner is a candidate
    for L in ref.levels:
        h, w = ref.images[L.level].shape
        assert (mask[R.mask_pixel(L.y, h, 160), R.mask_pixel(L.x, w, 200)] != 0).all()
        # the rule in the float32 form the documentation gives
        fy = np.floor((L.y.astype(np.float32) + np.float32(0.5)) * np.float32(160) / np.float32(h)).astype(np.int64)
        assert np.array_equal(np.minimum(fy, 159), R.mask_pixel(L.y, h, 160))
    unmasked = R.case_ref("rect_150_3")
    assert {(L.level, x, y) for L in ref.levels for x, y in zip(L.x[L.kept].tolist(), L.y[L.kept].tolist())} != \
           {(L.level, x, y) for L in unmasked.levels for x, y in zip(L.x[L.kept].tolist(), L.y[L.kept].tolist())}


def _mutated(got, what):
    kp, aux, desc = (a.copy() for a in got[:3])
    if what == "bit":
        desc[3, 5] ^= 0x10
    elif what == "angle":
        aux[7, 1] = (aux[7, 1] + np.float32(1e-3)) % 360
    elif what == "quadrant":
        aux[7, 1] = (360 - aux[7, 1]) % 360
    elif what == "response":
        aux[:, 2] *= np.float32(1 + 4e-6)                                                   # 67 u of the response itself
    elif what == "position":
        kp[11, 0] += 1
    elif what == "order":
        kp[[20, 21]], aux[[20, 21]], desc[[20, 21]] = kp[[21, 20]], aux[[21, 20]], desc[[21, 20]]
    elif what == "size":
        aux[2, 0] *= np.float32(1.2)
    return kp, aux, desc


@pytest.mark.parametrize("what", ["bit", "angle", "quadrant", "response", "position", "order", "size"])
def test_rules_notice_a_wrong_result(what):
    ref, got = R.case_ref("rect_150_1"), restatement("rect_150_1")
    lo = ref.levels[0].left_out
    rows = R.compare(got, ref)["rows"]
    assert not lo[rows[3][1], 5 * 8 + 4]                                                    # the flipped bit is a compared one
    with pytest.raises(AssertionError):
        R.compare(_mutated(got, what), ref)


# ------------------------------------------------------------------------------------------ the fixed-point stages
RESIZE_SHAPES = [((160, 200), (133, 167)), ((100, 100), (50, 50)), ((1, 200), (1, 167)), ((133, 167), (111, 139))]
RESIZE_BOUND = 1.0                   # 2^-12 per weight and 2^-16 pixel of position move the value by < 0.5 in all, the rounding adds 0.5
BLUR_BOUND = 2 * (255 * 2.22 / 256 + 0.5)                                                  # per pass 255 sum |w - g| + the rounding: 5.4


@pytest.mark.parametrize("src,dst", RESIZE_SHAPES)
def test_fixed_point_resize_against_float64_bilinear(src, dst):
    rng = np.random.Generator(np.random.PCG64(src[0] + dst[1]))
    for img in (rng.integers(0, 256, src, dtype=np.uint8), R.padded_to(R.image("rect"), 200, 200)[:src[0], :src[1]]):
        fixed = R.resize_fixed(img, *dst)
        dev = np.abs(fixed.astype(np.float64) - R.resize_float64(img, *dst)).max()
        print("resize %s -> %s: %.3f" % (src, dst, dev))
        assert dev <= RESIZE_BOUND
        out = np.zeros(dst, np.uint8)
        c = np.ascontiguousarray(img)
        O.lib().orb_resize(O._p(c, C.c_uint8), C.c_uint32(src[0]), C.c_uint32(src[1]), O._p(out, C.c_uint8), C.c_uint32(dst[0]), C.c_uint32(dst[1]))
        assert np.array_equal(out, fixed)


def test_resize_by_two_averages_four_pixels():
    img = R.image("rect100")
    exact = img.astype(np.int64).reshape(50, 2, 50, 2).sum(axis=(1, 3))
    assert np.array_equal(R.resize_fixed(img, 50, 50), (exact + 2) >> 2)                   # weights 1024 / 2048: the mean, rounded half up


@pytest.mark.parametrize("name", ["rect", "noise", "tiny63", "lattice"])
def test_8bit_blur_against_float64_gaussian(name):
    img = R.image(name)
    fixed = R.blur_fixed(img)
    dev = np.abs(fixed.astype(np.float64) - R.blur_float64(img)).max()
    print("blur %s: %.3f" % (name, dev))
    assert dev <= BLUR_BOUND
    out = np.zeros(img.shape, np.uint8)
    c = np.ascontiguousarray(img)
    O.lib().orb_blur(O._p(c, C.c_uint8), C.c_uint32(img.shape[0]), C.c_uint32(img.shape[1]), O._p(out, C.c_uint8))
    assert np.array_equal(out, fixed)


def test_fast_score_by_its_definition():
    """the running-minimum form against the definition read literally, and against the restatement's, on noise"""
    img = R.image("noise")[:40, :50]
    s = R.fast_scores(img)
    a = img.astype(np.int64)
    L = O.lib()
    L.orb_fast_score.restype = C.c_int
    c = np.ascontiguousarray(img)
    for y, x in [(3, 3), (36, 46), (20, 25), (10, 40), (30, 7), (17, 17), (5, 44)]:
        d = [a[y + dy, x + dx] - a[y, x] for dx, dy in R.CIRCLE]
        want = max(0, max(min(sg * d[(i + j) % 16] for j in range(9)) for i in range(16) for sg in (1, -1)))
        assert s[y, x] == want == L.orb_fast_score(O._p(c, C.c_uint8), C.c_uint32(50), C.c_int(x), C.c_int(y))
    assert (s[:3] == 0).all() and (s[:, -3:] == 0).all() and (s > R.FAST_THRESHOLD).sum() > 100


# ------------------------------------------------------------------------------------------ properties
def _kept(L):
    k = L.kept
    return L.x[k], L.y[k], L.response[k], L.angle[k], L.bits[k], L.abc[k]


@pytest.mark.parametrize("name", ["rect_150_3", "rect_300_4", "lattice"])
def test_level_composition(name):
    """level l of an L-level call is the one-level call on that level's resized image with the level's quota"""
    img, nf, nl, sf, kw = R.case_args(name)
    ref = R.case_ref(name)
    assert len(ref.levels) == nl
    for L in ref.levels:
        assert ref.images[L.level].shape == R.level_size(*img.shape, L.level, sf)
        one, = R.orb(ref.images[L.level], L.quota, 1, sf).levels
        for a, b in zip(_kept(L), _kept(one)):
            assert np.array_equal(a, b)
        got = O.orb(ref.images[L.level], L.quota, 1, sf)                                    # and the restatement's one-level call
        whole = O.orb(img, nf, nl, sf)
        sel = whole[1][:, 3] == L.level
        assert np.array_equal(got[2], whole[2][sel]) and np.array_equal(got[1][:, 1:3], whole[1][sel][:, 1:3])
        assert np.array_equal(got[3], whole[3][sel])


def test_transposition():
    ra, rb = R.case_ref("rect_all_1"), R.case_ref("rect_T_all_1")
    La, Lb = ra.levels[0], rb.levels[0]
    assert La.kept.all() and Lb.kept.all()
    ia, ib = np.lexsort((La.y, La.x)), np.lexsort((Lb.x, Lb.y))
    assert np.array_equal(La.x[ia], Lb.y[ib]) and np.array_equal(La.y[ia], Lb.x[ib])
    assert np.array_equal(La.response[ia], Lb.response[ib]) and np.array_equal(La.abc[ia][:, [1, 0, 2]], Lb.abc[ib])
    assert np.array_equal(La.m10[ia], Lb.m01[ib]) and np.array_equal(La.m01[ia], Lb.m10[ib])
    assert R.circular(90.0 - La.angle[ia], Lb.angle[ib]).max() < 1e-12
    print("transposed angles, restatement: %.2e" % R.transposition_holds(restatement("rect_all_1"), restatement("rect_T_all_1"), ra))


def test_a_permuted_pattern_moves_bits_not_keypoints():
    img, nf, nl, sf, _ = R.case_args("rect_150_3")
    perm = np.random.Generator(np.random.PCG64(9)).permutation(256)
    a, b = R.case_ref("rect_150_3"), R.orb(img, nf, nl, sf, pattern=R.default_pattern()[perm])
    for La, Lb in zip(a.levels, b.levels):
        assert np.array_equal(La.kp_xy, Lb.kp_xy) and np.array_equal(La.bits[:, perm], Lb.bits) and not np.array_equal(La.bits, Lb.bits)


def test_tiny_inputs():
    assert R.case_ref("tiny62x200").n == I.TINY_SHAPES[(62, 200)] == 0
    L, = R.case_ref("tiny63").levels
    assert I.TINY_SHAPES[(63, 63)] == 1 and (L.x.tolist(), L.y.tolist()) == ([31], [31]) and L.m10[0] == L.m01[0] == 0 and L.angle[0] == 0
