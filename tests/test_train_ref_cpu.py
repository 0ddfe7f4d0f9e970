"""tests/train_ref.py against the C restatement of the training path (oracle/train_oracle.c), bit for bit on every input that
tests/test_train_edges_gpu.py uses, and what each of those inputs is for: the keypoint counts that set the append's keypoints per
thread, the classes of validateKeyPoints, the special depth values met. These are conditions on the inputs, not tolerances: one that
fails means the input changed."""
import numpy as np
import pytest

import oracle_lib as O
import train_ref as TR


def _classes(name, depth_m=None):
    c = TR.case(name)
    kp, _ = TR.keypoints(name)
    return TR.validate(kp, c["mask"], np.ones_like(c["z"]) if depth_m is None else depth_m)


@pytest.mark.parametrize("name", sorted(TR.CASES))
def test_erosion_equals_the_restatement(name):
    mask = TR.case(name)["mask"]
    assert np.array_equal(TR.erode4(mask), O.train_erode4(mask))


@pytest.mark.parametrize("shape", [(9, 9), (5, 30), (30, 5), (23, 41)])
def test_erosion_at_the_border_and_on_small_images(shape):
    """what the GPU tests cannot reach (ORB keeps its keypoints away from the border): windows clipped by the image, images smaller
    than the window, single closed pixels"""
    rng = np.random.Generator(np.random.PCG64(shape[0] * 100 + shape[1]))
    for mask in (np.full(shape, 255, np.uint8), np.where(rng.random(shape) < 0.02, 0, 255).astype(np.uint8), np.zeros(shape, np.uint8)):
        er = TR.erode4(mask)
        assert np.array_equal(er, O.train_erode4(mask))
        assert (er == 255).all() == (mask != 0).all()


@pytest.mark.parametrize("name", sorted(TR.CASES))
@pytest.mark.parametrize("rot", sorted(TR.ROTATIONS))
@pytest.mark.parametrize("u16", [False, True])
def test_observation_equals_the_restatement(name, rot, u16):
    c = TR.case(name)
    kp, desc = TR.keypoints(name)
    od, op, src = TR.oracle_rows(name, rot, u16)
    rd, rp, rs = TR.observation(kp, desc, c["mask"], c["d16"] if u16 else c["z"], c["K"], TR.ROTATIONS[rot](), c["T"])
    assert np.array_equal(rs, src) and np.array_equal(rd, od)
    assert TR.same_points(rp, op)                                      # NaN where the restatement has NaN, the same bytes elsewhere
    if u16:
        assert np.isfinite(op).all()


def test_observation_with_a_permuted_pattern_equals_the_restatement():
    c = TR.case("qvga")
    kp, desc = TR.keypoints("qvga", 11)
    kp0, desc0 = TR.keypoints("qvga")
    assert np.array_equal(kp, kp0) and not np.array_equal(desc, desc0)          # the pattern moves bits, not keypoints
    od, op, src = TR.oracle_rows("qvga", "rotation", False, 11)
    rd, rp, rs = TR.observation(kp, desc, c["mask"], c["z"], c["K"], TR.ROTATIONS["rotation"](), c["T"])
    assert np.array_equal(rs, src) and np.array_equal(rd, od) and TR.same_points(rp, op)


def test_cameras_and_rotations_are_what_they_are_for():
    for W in (131, 320, 323, 640):
        K = TR.camera(W)
        assert K[0, 0] != K[1, 1] and K[0, 2] != K[1, 2] and K[0, 2] != np.rint(K[0, 2])
    assert TR.camera(320)[1, 2] == np.float32(118.5) and TR.camera(640)[1, 2] == 237
    assert TR.case("open_mask_integer_cx")["K"][0, 2] == 160
    R = TR.rotation_skew_axis().astype(np.float64)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R) - 1) < 1e-6
    assert np.abs(R - R.T).max() > 0.3 and (np.abs(R) > 0.02).all()             # no axis of the frame is kept: every entry takes part
    G = TR.general_matrix().astype(np.float64)
    assert np.abs(G @ G.T - np.eye(3)).max() > 0.5 and np.abs(G - G.T).max() > 0.3
    assert (TR.T != 0).all()


def test_vga_comb_has_three_keypoints_per_append_thread_and_every_class():
    cls, _ = _classes("vga")
    counts = np.bincount(cls, minlength=4)
    print("vga: keypoints %d, direct %d, rescued %d, no_mask %d" % (len(cls), counts[0], counts[1], counts[2]))
    assert len(cls) > 2048 and (len(cls) + 1023) // 1024 == 3
    assert counts[TR.DIRECT] >= 200 and counts[TR.RESCUED] >= 200 and counts[TR.NO_MASK] >= 200


def test_chunk2_case_has_two_keypoints_per_append_thread():
    kp, _ = TR.keypoints("vga_chunk2")
    assert len(kp) == 1600 and 1025 <= len(kp) <= 2048 and (len(kp) + 1023) // 1024 == 2
    cls, _ = _classes("vga_chunk2")
    counts = np.bincount(cls, minlength=4)
    assert counts[TR.DIRECT] >= 200 and counts[TR.RESCUED] >= 200 and counts[TR.NO_MASK] >= 200


@pytest.mark.parametrize("name", ["qvga", "odd", "qvga_one_level", "qvga_scale_1_5"])
def test_quarter_size_cases_have_every_class(name):
    cls, _ = _classes(name)
    counts = np.bincount(cls, minlength=4)
    print("%s: keypoints %d, direct %d, rescued %d, no_mask %d" % (name, len(cls), counts[0], counts[1], counts[2]))
    assert min(counts[TR.DIRECT], counts[TR.RESCUED], counts[TR.NO_MASK]) >= 30


def test_rescue_ties_and_fractions_occur():
    """With the scale factor 1.5 the coordinates of level 1 are multiples of 1.5: a keypoint at k + 0.5 lies at the same float32 distance
    from two open pixels, and the rescue's tie rule decides which depth it reads. The comb's stripes alone give no tie (the nearest pixel
    of a rectangle is unique for every other fraction). At the default scale factor most coordinates are no integers."""
    c = TR.case("qvga_scale_1_5")
    kp, _ = TR.keypoints("qvga_scale_1_5")
    cls, pix = TR.validate(kp, c["mask"], c["z"])
    er = TR.erode4(c["mask"]) != 0
    ties = changed = 0
    for i in np.flatnonzero(cls == TR.RESCUED):
        x, y = np.rint(kp[i]).astype(int)
        d = {(ii, jj): (np.float32(ii) - kp[i, 0]) * (np.float32(ii) - kp[i, 0]) + (np.float32(jj) - kp[i, 1]) * (np.float32(jj) - kp[i, 1])
             for ii in range(x - 2, x + 3) for jj in range(y - 2, y + 3) if er[jj, ii]}
        nearest = [p for p in d if d[p] == min(d.values())]
        assert tuple(pix[i]) == min(nearest)                           # the lowest column, then the lowest row
        if len(nearest) > 1:
            ties += 1
            changed += c["z"].view(np.uint32)[max(nearest)[1], max(nearest)[0]] != c["z"].view(np.uint32)[pix[i, 1], pix[i, 0]]
    assert ties >= 5 and changed >= 5                                  # taking the last of the equals instead changes that many rows
    kp, _ = TR.keypoints("vga")
    assert int((kp != np.rint(kp)).any(axis=1).sum()) >= 1000


@pytest.mark.parametrize("name", ["vga", "qvga"])
def test_every_special_depth_value_is_met_and_the_accepted_ones_come_out(name):
    c = TR.case(name)
    kp, _ = TR.keypoints(name)
    cls, pix = _classes(name)                                          # by the mask alone: the pixel each keypoint reads its depth at
    on = cls != TR.NO_MASK
    band = c["band"][pix[on, 1], pix[on, 0]]
    hits = {n: int((band == i).sum()) for i, (n, _) in enumerate(TR.SPECIALS)}
    print(name, hits)
    assert min(hits.values()) >= 1
    cls_z, _ = TR.validate(kp, c["mask"], c["z"])
    assert int((cls_z == TR.BAD_DEPTH).sum()) == hits["nan"] + hits["flt_max"] + hits["neg_flt_max"] + hits["flt_min"]
    for rot in sorted(TR.ROTATIONS):
        _, op, src = TR.oracle_rows(name, rot, False)
        got = c["band"][pix[src, 1], pix[src, 0]]
        for n in TR.ACCEPTED_SPECIALS:
            assert int((got == [s for s, _ in TR.SPECIALS].index(n)).sum()) == hits[n]
    # the rows they give, under the rotation: inf -> not finite; 0 -> exactly -T R (both ends of (u - cx) * 0 are zeros); negative -> behind the camera
    _, op, src = TR.oracle_rows(name, "rotation", False)
    got = c["band"][pix[src, 1], pix[src, 0]]
    names = [s for s, _ in TR.SPECIALS]
    assert not np.isfinite(op[got == names.index("inf")]).all(axis=1).any()
    zero = op[got == names.index("zero")]
    assert np.array_equal(zero, np.broadcast_to(TR.backproject([[0, 0]], [0.0], np.eye(3), TR.rotation_skew_axis(), TR.T), zero.shape))
    R64, T64 = TR.rotation_skew_axis().astype(np.float64), TR.T.astype(np.float64)
    assert ((op[got == names.index("negative")].astype(np.float64) @ R64.T + T64)[:, 2] < -0.7).all()
    assert np.isfinite(op[got == -1]).all()
    # uint16 millimetres hold none of the specials: 0 = no measurement for all of them
    assert (c["d16"][c["band"] >= 0] == 0).all() and (c["d16"][c["band"] < 0] >= 500).all()


def test_integer_cx_meets_an_inf_pixel():
    """(u - cx) * z with u == cx and z == inf is 0 * inf: NaN on both sides, with payloads that differ between x86 and the GPU"""
    c = TR.case("open_mask_integer_cx")
    kp, _ = TR.keypoints("open_mask_integer_cx")
    cls, pix = TR.validate(kp, c["mask"], c["z"])
    assert (cls != TR.NO_MASK).all() and (cls != TR.RESCUED).all()
    n = int(((pix[:, 0] == 160) & (cls == TR.DIRECT)).sum())
    assert n >= 2
    _, op, src = TR.oracle_rows("open_mask_integer_cx", "general", False)
    assert np.isnan(op[pix[src, 0] == 160]).all()


def test_tiny_case_has_keypoints():
    kp, _ = TR.keypoints("tiny")
    od, _, _ = TR.oracle_rows("tiny", "rotation", False)
    assert len(kp) >= 10 and 3 <= len(od) < len(kp)
