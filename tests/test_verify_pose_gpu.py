"""The verifier's pose (svd3, kabsch_solve, pose_invert in tod_amd/csrc/verify_growth.h, and the centroid and H sums in front of them)
at general rotations against float64, on the scenes of tests/pose_cases.py.

Every case runs through test_verify_gpu._compare_frame as the other frames do (rounds, stream position, inliers, pose within 1e-3
of the oracle) and is then held to a float64 Kabsch over the inliers it reports: |R - R64| <= 16 kappa 2^-23,
|t - t64| <= 3 tol_R |c_query| + n 2^-24 (|c_train| + |c_query|), R orthonormal with det 1 to 8 * 2^-23 (pose_cases.py). The scenes are
built so that the fitted set is the reported set: asserted here on the oracle's trace of every scene (the GPU equals its rounds), and
in test_pose_cases_cpu.py without a GPU.

Which form of the solve runs is a matter of the object's size (routing constants: kSprintN = 64 in verify_sprint.h,
kGrowthLdsPoints = 2048 in verify_growth.h): 40 on-object keypoints -> sprint_kernel (the counters show its launches), 120 ->
growth_kernel with the inliers staged in LDS, 2100 -> growth_kernel summing from global memory. The library does not expose which
of the two growth forms ran; the sizes rest on the constant.

todhip_test_kabsch runs kabsch_solve alone on matrices no frame can produce (pose_cases.kabsch_matrices).

MEASURED on an MI355X, |R - R64| / (kappa 2^-23), bound 16, worst per family (test_report_measured_ratios prints them with -s):
  frames  sprint / staged: gen 1.41 / 1.47 (unstaged 1.58), pi 0.84 / 1.03, pi_minus_1e-4 1.51 / 1.41, axis90 0.71 / 1.92,
          axis180 1.22 / 0.88, identity 0.91 / 1.12, planar 0.94 / 1.02, thin 0.41 / 0.91, elongated 0.002 / 0.001, far 0.58 / 0.73,
          near 0.69 / 1.31, off_centre 0.52 / 0.67, tiny_object 1.50 / 0.60
  hook    separated 2.04, equal 1.45, two_equal_top 2.00, two_equal_bottom 1.57, rank2 1.03, ratio1e-3 1.10, ratio1e-6 1.19,
          ratio1e-8 1.01, diagonal and permuted-diagonal 0.00
The same figures as the CPU definition's (test_pose_cases_cpu.py): both compile without contraction. Also in DESIGN.md section 3.
"""
import numpy as np
import pytest

import oracle_lib as O
import pose_cases as pc
from test_verify_gpu import _compare_frame, _pack_scene, _verify_device_from_scene
from tod_amd import capi

pytestmark = pytest.mark.gpu

MEASURED = {}                                                    # family -> largest |R - R64| / (kappa 2^-23) seen by this run


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _one_pose(ctx, sc, name, n_iter=300):
    """GPU == oracle on the frame; then, on the oracle's own trace (the library's does not carry these fields), that nothing was
    admitted after the fit, so that a miss of the float64 bound below is the arithmetic's and not the scene's."""
    poses, _ = _compare_frame(ctx, sc, 8, n_iter, err=pc.err_of(name))
    rc, o_poses, o_rounds = O.verify(sc["kp_xy"], sc["cloud"], sc["row_ptr"], sc["matches"], sc["matches_xyz"], sc["spans"], 8, n_iter,
                                     pc.err_of(name), O.rng_new(1))
    assert rc == 0
    pc.check_fitted_set_is_reported_set(sc, o_poses, o_rounds)
    assert [p["object"] for p in poses] == [sc["object"]] and np.array_equal(poses[0]["inliers"], o_poses[0]["inliers"])
    return poses[0]


@pytest.mark.parametrize("n_on", [40, 120])
@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_frame_pose_equals_float64_kabsch(ctx, name, n_on):
    sc = pc.clean_scene(name) if n_on == 120 else pc.sprint_scene(name)
    p = _one_pose(ctx, sc, name)
    cnt = ctx.counters()
    assert len(p["inliers"]) >= (100 if n_on == 120 else 30)
    if n_on == 40:
        assert cnt.last_sprint_launches >= 1 and cnt.last_sprint_rounds >= 1
    ratio = pc.check_pose_against_kabsch64(sc, p)
    key = "%s/%s" % (pc.family(name), "sprint" if n_on == 40 else "staged")
    MEASURED[key] = max(MEASURED.get(key, 0.0), ratio)
    print("%s n_on %d: |R - R64| / (kappa 2^-23) = %.3f" % (name, n_on, ratio))


def test_unstaged_growth_pose_equals_float64_kabsch(ctx):
    """2100 on-object keypoints (> kGrowthLdsPoints = 2048 inliers), a 1080p camera so that every keypoint has a pixel of its own."""
    sc = pc.unstaged_scene()
    p = _one_pose(ctx, sc, "gen0", n_iter=100)
    assert len(p["inliers"]) > 2048
    ratio = pc.check_pose_against_kabsch64(sc, p)
    MEASURED["gen/unstaged"] = ratio
    print("gen0 n_on 2100: |R - R64| / (kappa 2^-23) = %.3f" % ratio)


def test_device_and_batch_forms_give_the_host_form_pose(ctx):
    """One scene through verify_device, and the same scene at three rotations through verify_batch_device: poses equal to the host
    form's (same kernels, same inputs), which is held to float64 here as well."""
    import torch
    turns = [pc.CASES["gen1"], pc.CASES["pi_xy"], dict(axis=(0.3, -0.5, 0.8), angle=2.0)]
    scs = [pc.case_scene("gen1", axis=t["axis"], angle=t["angle"], seed=5) for t in turns]
    assert all(np.array_equal(s["spans"], scs[0]["spans"]) for s in scs)              # the same models, turned three ways
    host = []
    for sc in scs:
        host.append(ctx.verify(sc["kp_xy"], sc["cloud"], sc["row_ptr"], sc["matches"], sc["matches_xyz"], sc["spans"], 8, 300, 0.01,
                               capi.rng_new(1)))
        assert [p["object"] for p in host[-1]] == [sc["object"]]
        pc.check_pose_against_kabsch64(sc, host[-1][0])
    dev, _, _ = _verify_device_from_scene(ctx, scs[0], 1, 8, 300)
    assert len(dev) == 1 and np.array_equal(dev[0]["R"], host[0][0]["R"]) and np.array_equal(dev[0]["t"], host[0][0]["t"])
    assert np.array_equal(dev[0]["inliers"], host[0][0]["inliers"])
    nq, F = len(scs[0]["kp_xy"]), len(scs)
    packed = [_pack_scene(s, 1) for s in scs]
    d_kp = torch.from_numpy(np.stack([s["kp_xy"] for s in scs])).cuda()
    d_cloud = torch.from_numpy(np.stack([s["cloud"] for s in scs])).cuda()
    d_counts = torch.from_numpy(np.stack([p[0] for p in packed])).cuda()
    d_m = torch.from_numpy(np.stack([p[1] for p in packed])).cuda()
    d_xyz = torch.from_numpy(np.stack([p[2] for p in packed])).cuda()
    torch.cuda.synchronize()
    rngs = (capi.Rng * F)(*[capi.rng_new(1) for _ in range(F)])
    got = ctx.verify_batch_device(F, d_kp.data_ptr(), nq, d_cloud.data_ptr(), 480, 640, d_counts.data_ptr(), d_m.data_ptr(),
                                  d_xyz.data_ptr(), 1, scs[0]["spans"], 8, 300, 0.01, rngs)
    for f in range(F):
        assert len(got[f]) == 1 and got[f][0]["object"] == scs[f]["object"]
        assert np.array_equal(got[f][0]["R"], host[f][0]["R"]) and np.array_equal(got[f][0]["t"], host[f][0]["t"])
        assert np.array_equal(got[f][0]["inliers"], host[f][0]["inliers"])


@pytest.mark.parametrize("name", ["gen0", "pi_x", "planar0"])
def test_noisy_frames_equal_the_oracle_and_stay_near_the_truth(ctx, name):
    """sigma = 2 mm and two distractor matches per keypoint: GPU == oracle as everywhere, the truth within the tolerances of
    test_verify_gpu's truth tests. No float64 claim: the fitted set is not observable here."""
    sc = pc.case_scene(name, matches_per_kp=3, noise=0.002)
    poses, _ = _compare_frame(ctx, sc, 8, 500)
    mine = [p for p in poses if p["object"] == sc["object"]]
    assert len(mine) == 1
    assert np.abs(mine[0]["R"] - sc["R_true"]).max() < 0.05 and np.abs(mine[0]["t"] - sc["t_true"]).max() < 0.02


def test_pose_solve_hook_on_matrices_no_frame_can_produce(ctx):
    names, Hd, Cc, ranks = pc.kabsch_matrices()
    R, T = ctx.test_kabsch(Hd, Cc)
    worst = pc.check_kabsch_solutions(names, Hd, Cc, ranks, R, T, "gpu")
    for fam, v in worst.items():
        MEASURED["hook/" + fam] = v
    # the definition on the same list, and the two against each other (no bit equality: two compilers)
    R_o, T_o = O.kabsch_solve(Hd, Cc)
    pc.check_kabsch_solutions(names, Hd, Cc, ranks, R_o, T_o, "oracle")
    for i, name in enumerate(names):
        if ranks[i] <= 1:
            continue
        kappa = pc.kabsch64_of_H(Hd[i], Cc[i, :3], Cc[i, 3:])[2]
        if np.isfinite(kappa) and kappa < 1e4:
            assert np.abs(R[i].astype(np.float64) - R_o[i]).max() <= pc.r_tol(kappa), (name, kappa)


def test_report_measured_ratios():
    """Prints what the tests above measured (run with -s): the largest |R - R64| / (kappa 2^-23) per family and form. Run alone it
    has nothing to print and passes: the tests above assert every figure themselves."""
    for k in sorted(MEASURED):
        print("measured %-28s %.3f" % (k, MEASURED[k]))
    assert all(v <= pc.R_BOUND for v in MEASURED.values())
