"""The pose scenes of tests/pose_cases.py, their float64 references, and the CPU oracle against those references (no GPU).

What is pinned here: the builder's invariants; that kabsch64 and pnp64 recover the truth on exact data; that the oracle's 3D pose
(oracle/tod_oracle.cpp: svd3, kabsch) on every case of the list lies within 16 kappa 2^-23 of a float64 Kabsch over the inliers it
reports -- measured 0.12 of that bound at the most, orc_kabsch_solve on the hook's matrices 2.04 of 16 -- and that the 2D definition
(oracle/pnp_oracle.c) lies within 2^-21 of a float64 Gauss-Newton run to convergence -- measured 3.0e-8 (R and t) at the
most. tests/test_verify_pose_gpu.py and tests/test_pnp_pose_gpu.py hold the kernels to the same bounds.

Range. The matrix list goes from 1e-30 to 0.9 FLT_MAX and to both sides of the point where the product of two squared column norms
leaves the float range. Two things were wrong at its ends before these tests, in kernel and oracle alike, and are fixed in both: that
product overflowed from s1 s2 = 1.8e19 on (no rotation applied, |R R^T - I| = 0.5); and far from 1 the squares of the entries
themselves overflowed (NaN from 1e19 on) or went denormal -- from 1e-20 down for a full-rank H, but already at a largest entry of
1e-12 for the rounding residue that stands in for a zero singular value (rank 1: |R R^T - I| of 2 to 4 times the bound for two in
a hundred random factors, which is why every spectrum has three draws per pair of determinants). svd3 now scales such an H by a power
of two first; between 2^-32 and 2^40 nothing is scaled. include/todhip.h states the range at todhip_verify: every finite H.
"""
import numpy as np
import pytest

import oracle_lib as O
import pose_cases as pc

CAMS = pc.CAMS


# ------------------------------------------------------------------------------------------ the builder
@pytest.mark.parametrize("name", pc.CASE_NAMES)
@pytest.mark.parametrize("k,noise", [(1, 0.0), (3, 0.002)])
def test_builder_invariants(name, k, noise):
    sc = pc.clean_scene(name) if (k, noise) == (1, 0.0) else pc.case_scene(name, matches_per_kp=k, noise=noise)
    kp, cam = sc["kp_xy"], sc["cam"]
    n_kp = len(kp)
    assert n_kp == 320 and len(sc["matches"]) == n_kp * k and sc["row_ptr"][-1] == n_kp * k
    px = kp.astype(np.int64)
    assert len({(a, b) for a, b in px}) == n_kp                                    # a pixel of its own for every keypoint
    assert (kp > 0).all() and (kp[:, 0] < cam["W"] - 1).all() and (kp[:, 1] < cam["H"] - 1).all()
    assert np.isfinite(sc["cloud"][px[:, 1], px[:, 0]]).all() and np.isfinite(sc["cloud"]).all(axis=2).sum() == n_kp
    on = sc["true_match"] >= 0
    assert on.sum() == 120
    tm = sc["true_match"][on]
    assert (sc["matches"]["queryIdx"][tm] == np.nonzero(on)[0]).all() and (sc["matches"]["imgIdx"][tm] == sc["object"]).all()
    assert (tm >= sc["row_ptr"][:-1][on]).all() and (tm < sc["row_ptr"][1:][on]).all()
    # the true match's model point, posed, is the keypoint's own cloud point (to float rounding, or to the noise)
    posed = sc["matches_xyz"][tm].astype(np.float64) @ sc["R_true"].T + sc["t_true"]
    seen = sc["cloud"][px[on, 1], px[on, 0]]
    assert np.abs(posed - seen).max() <= (6 * noise if noise else 2.0 ** -23 * np.abs(seen).max())
    if k == 1:                                                                     # clutter never votes for the visible object
        assert (sc["matches"]["imgIdx"][sc["row_ptr"][:-1][~on]] != sc["object"]).all()
        assert (sc["matches"]["imgIdx"] == sc["object"]).sum() == 120


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_float64_references_recover_the_truth_on_exact_data(name):
    sc = pc.clean_scene(name)
    on = sc["true_match"] >= 0
    X = sc["matches_xyz"][sc["true_match"][on]].astype(np.float64)
    q = X @ sc["R_true"].T + sc["t_true"]
    R, t, kappa = pc.kabsch64(X, q)
    assert np.abs(R - sc["R_true"]).max() < 1e-12 and np.abs(t - sc["t_true"]).max() < 1e-12 and np.isfinite(kappa)
    for cam in CAMS.values():
        sc2 = pc.case_scene(name, cam=cam, with_cloud=False)                       # (the case's translation depends on the camera)
        X = sc2["matches_xyz"][sc2["true_match"][sc2["true_match"] >= 0]].astype(np.float64)
        P = X @ sc2["R_true"].T + sc2["t_true"]
        uv = np.stack([cam["fx"] * P[:, 0] / P[:, 2] + cam["cx"], cam["fy"] * P[:, 1] / P[:, 2] + cam["cy"]], 1)
        R0 = pc.rot((1, 2, 3), 0.03) @ sc2["R_true"]
        t0 = sc2["t_true"] * 1.01 + np.array([0.004, -0.003, 0.0])
        R, t = pc.pnp64(pc.cam_K(cam), X, uv, R0, t0)
        assert np.abs(R - sc2["R_true"]).max() < 1e-12 and np.abs(t - sc2["t_true"]).max() < 1e-12 * max(1.0, sc2["t_true"][2])


# ------------------------------------------------------------------------------------------ the 3D oracle against float64
@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_oracle_pose_equals_float64_kabsch_over_its_inliers(name):
    sc = pc.clean_scene(name)
    rc, poses, rounds = O.verify(sc["kp_xy"], sc["cloud"], sc["row_ptr"], sc["matches"], sc["matches_xyz"], sc["spans"], 8, 300,
                                 pc.err_of(name), O.rng_new(1))
    assert rc == 0
    p = pc.check_fitted_set_is_reported_set(sc, poses, rounds)
    assert len(p["inliers"]) >= 100
    pc.check_pose_against_kabsch64(sc, p)
    # and the truth, as far as float32 inputs allow: a coordinate's rounding (2^-24 * 5.75 m at the most, the far case) over the
    # smallest lever arm of the list (5 mm, tiny_object and elongated) is 7e-5
    assert np.abs(p["R"] - sc["R_true"]).max() < 1e-4 and np.abs(p["t"] - sc["t_true"]).max() < 1e-4 * max(1.0, sc["t_true"][2])


@pytest.mark.parametrize("name", pc.CASE_NAMES + ["unstaged"])
def test_oracle_on_the_scenes_of_the_other_forms_of_the_solve(name):
    """The 40-keypoint scenes (the single-wave form on the GPU) and the 2100-keypoint one (sums from global memory) are scenes of their
    own: the same proof for them, so that test_verify_pose_gpu.py's float64 comparison rests on it there too."""
    sc = pc.unstaged_scene() if name == "unstaged" else pc.sprint_scene(name)
    rc, poses, rounds = O.verify(sc["kp_xy"], sc["cloud"], sc["row_ptr"], sc["matches"], sc["matches_xyz"], sc["spans"], 8,
                                 100 if name == "unstaged" else 300, pc.err_of(name) if name != "unstaged" else 0.01, O.rng_new(1))
    assert rc == 0
    p = pc.check_fitted_set_is_reported_set(sc, poses, rounds)
    assert len(p["inliers"]) >= (2049 if name == "unstaged" else 30)
    pc.check_pose_against_kabsch64(sc, p)


def test_oracle_pose_solve_on_the_matrix_list():
    names, Hd, Cc, ranks = pc.kabsch_matrices()
    R, T = O.kabsch_solve(Hd, Cc)
    worst = pc.check_kabsch_solutions(names, Hd, Cc, ranks, R, T, "oracle")
    print("oracle |R - R64| / (kappa 2^-23), worst per family:", {k: round(v, 2) for k, v in worst.items()})


# ------------------------------------------------------------------------------------------ the 2D definition against float64
@pytest.mark.parametrize("cam_name", list(CAMS))
@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_2d_definition_equals_float64_gauss_newton(name, cam_name):
    sc = pc.pnp_scene(name, cam_name)
    cam = CAMS[cam_name]
    rc, poses, _ = O.verify_2d(sc["kp_xy"], pc.cam_K(cam), sc["row_ptr"], sc["matches"], sc["matches_xyz"], sc["spans"], 8, 300, 2.0,
                               O.rng_new(1))
    assert rc == 0 and [p["object"] for p in poses] == [sc["object"]]
    assert len(poses[0]["inliers"]) == 120
    pc.check_pnp_pose(sc, cam, poses[0])


@pytest.mark.parametrize("cam_name", list(CAMS))
@pytest.mark.parametrize("name", pc.NOISY_2D_CASES)
def test_noisy_2d_definition_stays_near_the_truth(name, cam_name):
    sc, cam = pc.pnp_scene(name, cam_name, noise=0.002), CAMS[cam_name]
    rc, poses, _ = O.verify_2d(sc["kp_xy"], pc.cam_K(cam), sc["row_ptr"], sc["matches"], sc["matches_xyz"], sc["spans"], 8, 300,
                               pc.NOISY_2D_PX[cam_name], O.rng_new(1))
    assert rc == 0 and [p["object"] for p in poses] == [sc["object"]]
    assert np.abs(poses[0]["R"] - sc["R_true"]).max() < 0.03 and np.abs(poses[0]["t"] - sc["t_true"]).max() < 0.015
