"""todhip_verify_2d (tod_amd/csrc/pnp.hip: Grunert's P3P, the quartic by bracketing, five Gauss-Newton steps) at general rotations
against float64, on the scenes of tests/pose_cases.py with two cameras: 525 / 320 / 240 at 640 x 480, and fx != fy with the
principal point off the centre (1400 / 1390, 900 / 500) at 1080p.

Every case runs through test_pnp_gpu._same (bit for bit against oracle/pnp_oracle.c) and is then held to pnp64, a float64
Gauss-Newton run to convergence from the truth on the reported inliers' float32 inputs: |R - R64| <= 2^-21,
|t - t64| <= 2^-21 max(1, |t|), the float32 rounding of the output with a margin of 8. The comparison is with pnp64, not with the
truth, so that the keypoints' float32 rounding is not charged to the kernel; the planar cases, which have a mirrored second
minimum, must also lie within 1e-3 of the truth. 120 on-object keypoints, 300 hypotheses, 2 px.

The noisy variants (sigma = 2 mm) keep the 0.03 / 0.015 truth tolerances of test_pnp_gpu; pose_cases.NOISY_2D_CASES says which cases
and thresholds and why.

MEASURED on an MI355X (test_report_measured_differences prints them per family and camera with -s): |R - R64| <= 2.98e-8 and
|t - t64| / max(1, |t|) <= 2.97e-8 over all 58 cases (29 on two cameras; bound 2^-21 = 4.8e-7); the rotations about one
coordinate axis (pi, axis90, axis180, identity) reach 1e-14 in R. Also in DESIGN.md section 3.
"""
import numpy as np
import pytest

import pose_cases as pc
from test_pnp_gpu import _same
from tod_amd import capi

pytestmark = pytest.mark.gpu

MEASURED = {}


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("cam_name", list(pc.CAMS))
@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_2d_pose_equals_float64_gauss_newton(ctx, name, cam_name):
    sc, cam = pc.pnp_scene(name, cam_name), pc.CAMS[cam_name]
    poses = _same(ctx, sc, 8, 300, 2.0, K=pc.cam_K(cam))
    assert [p["object"] for p in poses] == [sc["object"]] and len(poses[0]["inliers"]) == 120
    dR, dt = pc.check_pnp_pose(sc, cam, poses[0])
    key = "%s/%s" % (pc.family(name), cam_name)
    MEASURED[key] = max(MEASURED.get(key, (0, 0)), (dR, dt))
    print("%s %s: |R - R64| = %.2e, |t - t64| / max(1, |t|) = %.2e" % (name, cam_name, dR, dt))


@pytest.mark.parametrize("cam_name", list(pc.CAMS))
@pytest.mark.parametrize("name", pc.NOISY_2D_CASES)
def test_noisy_2d_frames_equal_the_definition_and_stay_near_the_truth(ctx, name, cam_name):
    """sigma = 2 mm: the tolerances of test_pnp_gpu's truth tests (pose_cases.NOISY_2D_CASES says why these cases and thresholds)."""
    sc, cam = pc.pnp_scene(name, cam_name, noise=0.002), pc.CAMS[cam_name]
    poses = _same(ctx, sc, 8, 300, pc.NOISY_2D_PX[cam_name], K=pc.cam_K(cam))
    assert [p["object"] for p in poses] == [sc["object"]]
    assert np.abs(poses[0]["R"] - sc["R_true"]).max() < 0.03 and np.abs(poses[0]["t"] - sc["t_true"]).max() < 0.015


def test_report_measured_differences():
    """Prints what the tests above measured (run with -s): the largest |R - R64| per family and camera, with its |t - t64|. Run alone
    it has nothing to print and passes: the tests above assert every figure themselves."""
    for k in sorted(MEASURED):
        print("measured %-24s dR %.2e dt %.2e" % (k, MEASURED[k][0], MEASURED[k][1]))
    assert all(v[0] <= pc.PNP_TOL and v[1] <= pc.PNP_TOL for v in MEASURED.values())
