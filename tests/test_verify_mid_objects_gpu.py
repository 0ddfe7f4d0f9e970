"""Whole verify calls on frames whose objects have 65 .. 512 matches each -- the sizes whose draw table is built with one lane per
stream position and eight words per lane: poses, inlier lists, their order, every round's iteration counts and the position of the
rand() stream must equal the CPU oracle's (tests/scene_checks.py, as tests/test_verify_gpu.py does for its own scenes)."""
import numpy as np
import pytest

import scene_checks as TS
from tod_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from tod_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def _matches_per_object(sc):
    """matches ClusterPerObject keeps (the keypoint has a point in the cloud), per object"""
    kp, n_obj = sc["kp_xy"], len(sc["spans"])
    kept = ~np.isnan(sc["cloud"][kp[:, 1].astype(np.int64), kp[:, 0].astype(np.int64), 0])
    q = sc["matches"]["queryIdx"].astype(np.int64)
    return np.bincount(sc["matches"]["imgIdx"][kept[q]].astype(np.int64), minlength=n_obj)


def test_one_visible_object(ctx):
    sc = synth.make_verify_scene(400, n_objects=6, visible=((1, 0.30),), matches_per_kp=3, seed=811)
    per = _matches_per_object(sc)
    assert per.min() >= 65 and per.max() <= 512 and per[1] > 256           # the visible one needs five words
    poses, rounds, _ = TS.compare_frame(ctx, sc, 8, 300)
    assert [p["object"] for p in poses] == [1]


def test_two_visible_objects(ctx):
    sc = synth.make_verify_scene(500, n_objects=6, visible=((1, 0.25), (4, 0.20)), matches_per_kp=3, seed=812)
    per = _matches_per_object(sc)
    assert per.min() >= 65 and per.max() <= 512
    poses, rounds, _ = TS.compare_frame(ctx, sc, 8, 300)
    assert sorted(p["object"] for p in poses) == [1, 4]


def test_one_hopeless_object(ctx):
    """random matches only: no pose, every iteration's attempts burn draws on picks that lead nowhere"""
    sc = synth.make_verify_scene(110, n_objects=1, visible=(), matches_per_kp=3, seed=813)
    per = _matches_per_object(sc)
    assert len(per) == 1 and 256 < per[0] <= 512
    poses, rounds, _ = TS.compare_frame(ctx, sc, 8, 150)
    assert poses == [] and len(rounds) == 1
    assert rounds[0].draws_after - rounds[0].draws_before > 3 * rounds[0].iterations   # failed picks were drawn and removed
