"""todhip_verify_2d (tod_amd/csrc/pnp.hip) against its definition, oracle/pnp_oracle.c. PARITY UNPINNED BY CONSTRUCTION with
respect to the reference: GuessGenerator.cpp:147-152 leaves the 2D-only branch as a TODO (doc/source/index.rst:36-46), so the
oracle DEFINES the result. The bar is the integer one all the same: same objects, same consensus sets, poses equal bit for bit
(f64 arithmetic with + - * / sqrt in a fixed order on both sides)."""
import numpy as np
import pytest

import oracle_lib as O
from tod_amd import capi, synth

pytestmark = pytest.mark.gpu

K = np.array([[525.0, 0, 320.0], [0, 525.0, 240.0], [0, 0, 1]], np.float32)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _same(ctx, sc, min_inliers, n_iter, err_px, K=K, seed=1):
    rng_o, rng_g = O.rng_new(seed), capi.rng_new(seed)
    rc, want, (bh, bc) = O.verify_2d(sc["kp_xy"], K, sc["row_ptr"], sc["matches"], sc["matches_xyz"], sc["spans"], min_inliers, n_iter, err_px, rng_o)
    assert rc == 0
    got = ctx.verify_2d(sc["kp_xy"], K, sc["row_ptr"], sc["matches"], sc["matches_xyz"], sc["spans"], min_inliers, n_iter, err_px, rng_g)
    assert rng_g.draws == rng_o.draws == 1
    assert [p["object"] for p in got] == [p["object"] for p in want]
    for g, w in zip(got, want):
        assert np.array_equal(g["inliers"], w["inliers"])
        assert np.array_equal(g["R"], w["R"]) and np.array_equal(g["t"], w["t"]), (g["R"] - w["R"], g["t"] - w["t"])
    return got


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_two_visible_objects_equal_the_definition_and_the_truth(ctx, seed):
    sc = synth.make_verify_scene(700, n_objects=6, per_object=300, visible=((1, 0.30), (4, 0.20)), matches_per_kp=3, seed=seed)
    poses = _same(ctx, sc, 12, 500, 3.0, seed=seed + 1)
    assert [p["object"] for p in poses] == [1, 4]
    for p in poses:
        R_true, t_true = sc["poses"][p["object"]]
        assert np.abs(p["R"] - R_true).max() < 0.03 and np.abs(p["t"] - t_true).max() < 0.015


def test_noise_free_keypoints_give_the_exact_pose(ctx):
    sc = synth.make_verify_scene(500, n_objects=4, per_object=300, visible=((2, 0.4),), matches_per_kp=2, seed=9, noise=0.0)
    poses = _same(ctx, sc, 15, 300, 2.0)
    assert len(poses) == 1 and poses[0]["object"] == 2
    R_true, t_true = sc["poses"][2]
    assert np.abs(poses[0]["R"] - R_true).max() < 2e-4 and np.abs(poses[0]["t"] - t_true).max() < 2e-4


def test_edge_cases_empty_few_matches_no_object(ctx):
    sc = synth.make_verify_scene(300, n_objects=5, per_object=200, visible=((0, 0.3),), matches_per_kp=2, seed=5)
    # nothing visible reaches an impossible min_inliers; zero hypotheses; zero keypoints
    assert _same(ctx, sc, 10_000, 200, 3.0) == []
    assert _same(ctx, sc, 10, 0, 3.0) == []
    empty = dict(kp_xy=np.zeros((0, 2), np.float32), row_ptr=np.zeros(1, np.uint32), matches=np.zeros(0, capi.DMATCH_DTYPE),
                 matches_xyz=np.zeros((0, 3), np.float32), spans=sc["spans"])
    assert _same(ctx, empty, 5, 100, 3.0) == []
    # a threshold so tight that only near-exact hypotheses count, and one so loose that everything in front of the camera does
    _same(ctx, sc, 8, 300, 0.25)
    loose = _same(ctx, sc, 8, 50, 5000.0)
    assert len(loose) >= 1
    # clutter only: no pose, and the stream still advances by exactly one draw (checked in _same)
    clutter = synth.make_verify_scene(300, n_objects=5, per_object=200, visible=(), matches_per_kp=2, seed=6)
    assert _same(ctx, clutter, 10, 300, 2.0) == []


def test_other_intrinsics_many_objects_and_a_big_object(ctx):
    K2 = np.array([[1400.0, 0, 960.0], [0, 1390.0, 540.0], [0, 0, 1]], np.float32)
    sc = synth.make_verify_scene(2000, n_objects=40, per_object=400, visible=((3, 0.25), (17, 0.2), (31, 0.15)), matches_per_kp=5, seed=11,
                                 H=1080, W=1920, f=1400.0)
    # the scene was projected with f = 1400 on both axes; fy = 1390 makes the model slightly wrong, the definition does not care
    poses = _same(ctx, sc, 15, 1000, 4.0, K=K2)
    assert {p["object"] for p in poses} >= {3, 17, 31}


def test_bad_arguments(ctx):
    sc = synth.make_verify_scene(100, n_objects=3, per_object=100, visible=((1, 0.5),), matches_per_kp=2, seed=1)
    with pytest.raises(capi.TodError):
        ctx.verify_2d(sc["kp_xy"], K, sc["row_ptr"], sc["matches"], sc["matches_xyz"], sc["spans"], 8, 100, 0.0, capi.rng_new(1))
    with pytest.raises(capi.TodError):
        ctx.verify_2d(sc["kp_xy"], K, sc["row_ptr"], sc["matches"], sc["matches_xyz"], sc["spans"][:1], 8, 100, 3.0, capi.rng_new(1))


def test_device_form_after_the_device_matcher_equals_the_host_form(ctx):
    """todhip_match_device -> todhip_verify_2d_device on the device buffers == todhip_match -> todhip_verify_2d through the host."""
    import torch
    desc, pts, off = synth.make_db(6, per_object=800)
    fr = synth.make_frame(desc, pts, off, 500, frame=3, visible_object=4)
    spans = ctx.db_load(desc, pts, off)
    row_ptr, m, xyz = ctx.match(fr["q_desc"], 3, 35)
    host = ctx.verify_2d(fr["kp_xy"], K, row_ptr, m, xyz, spans, 8, 400, 3.0, capi.rng_new(5))
    d_q = torch.from_numpy(fr["q_desc"]).cuda(); d_kp = torch.from_numpy(fr["kp_xy"]).cuda()
    cnt = torch.zeros(500, dtype=torch.int32, device="cuda"); mm = torch.zeros((1500, 4), dtype=torch.int32, device="cuda")
    xx = torch.zeros((1500, 3), dtype=torch.float32, device="cuda")
    ctx.match_device(d_q.data_ptr(), 500, 3, 35, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr())
    dev = ctx.verify_2d_device(d_kp.data_ptr(), 500, K, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr(), 3, spans, 8, 400, 3.0, capi.rng_new(5))
    assert len(host) == len(dev) == 1 and host[0]["object"] == dev[0]["object"] == 4
    assert np.array_equal(host[0]["R"], dev[0]["R"]) and np.array_equal(host[0]["t"], dev[0]["t"]) and np.array_equal(host[0]["inliers"], dev[0]["inliers"])
    assert np.abs(dev[0]["R"] - synth.pose_R()).max() < 0.03 and np.abs(dev[0]["t"] - synth.POSE_T).max() < 0.015


def test_batch_of_frames_equals_frame_by_frame(ctx):
    """todhip_match_device on 5 frames' descriptors -> todhip_verify_2d_batch_device == the single-frame host form per frame (objects,
    poses, consensus sets bit for bit; every generator advanced by its one draw); one frame has no visible object, one pads with counts 0."""
    import torch
    desc, pts, off = synth.make_db(8, per_object=600)
    nq, k, F = 400, 2, 5
    frames = [synth.make_frame(desc, pts, off, nq, frame=20 + f, visible_object=(3 * f) % 8) for f in range(F)]
    frames[3]["q_desc"] = np.random.Generator(np.random.PCG64(1)).integers(0, 256, (nq, 32), dtype=np.uint8)        # clutter only
    spans = ctx.db_load(desc, pts, off)
    d_q = torch.from_numpy(np.concatenate([fr["q_desc"] for fr in frames])).cuda()
    d_kp = torch.from_numpy(np.concatenate([fr["kp_xy"] for fr in frames])).cuda()
    cnt = torch.zeros(F * nq, dtype=torch.int32, device="cuda"); mm = torch.zeros((F * nq * k, 4), dtype=torch.int32, device="cuda")
    xx = torch.zeros((F * nq * k, 3), dtype=torch.float32, device="cuda")
    ctx.match_device(d_q.data_ptr(), F * nq, k, 35, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr())
    cnt.view(F, nq)[4, 300:] = 0                                                  # frame 4 has only 300 keypoints
    rngs = (capi.Rng * F)(*[capi.rng_new(3 + f) for f in range(F)])
    got = ctx.verify_2d_batch_device(F, d_kp.data_ptr(), nq, K, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr(), k, spans, 8, 300, 3.0, rngs)
    n_found = 0
    for f, fr in enumerate(frames):
        q = fr["q_desc"] if f != 4 else fr["q_desc"][:300]
        kp = fr["kp_xy"] if f != 4 else fr["kp_xy"][:300]
        row_ptr, m, xyz = ctx.match(q, k, 35)
        rng = capi.rng_new(3 + f)
        want = ctx.verify_2d(kp, K, row_ptr, m, xyz, spans, 8, 300, 3.0, rng)
        assert rngs[f].draws == rng.draws == 1
        assert [p["object"] for p in got[f]] == [p["object"] for p in want], f
        for g, w in zip(got[f], want):
            assert np.array_equal(g["R"], w["R"]) and np.array_equal(g["t"], w["t"]) and np.array_equal(g["inliers"], w["inliers"])
        n_found += len(want)
    assert got[3] == [] and n_found >= 3


def test_capacity_returns_of_the_three_forms(ctx):
    """No room for the pose that is there: every form reports TODHIP_ECAPACITY, and its generator has still made the frame's one
    draw. Set-up of test_device_form_after_the_device_matcher_equals_the_host_form; then the two-visible-objects scene with room
    for one pose only."""
    import torch
    desc, pts, off = synth.make_db(6, per_object=800)
    fr = synth.make_frame(desc, pts, off, 500, frame=3, visible_object=4)
    spans = ctx.db_load(desc, pts, off)
    row_ptr, m, xyz = ctx.match(fr["q_desc"], 3, 35)
    d_q = torch.from_numpy(fr["q_desc"]).cuda(); d_kp = torch.from_numpy(fr["kp_xy"]).cuda()
    cnt = torch.zeros(500, dtype=torch.int32, device="cuda"); mm = torch.zeros((1500, 4), dtype=torch.int32, device="cuda")
    xx = torch.zeros((1500, 3), dtype=torch.float32, device="cuda")
    ctx.match_device(d_q.data_ptr(), 500, 3, 35, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr())
    rng_h, rng_d, rngs = capi.rng_new(5), capi.rng_new(5), (capi.Rng * 1)(capi.rng_new(5))
    calls = [lambda: ctx.verify_2d(fr["kp_xy"], K, row_ptr, m, xyz, spans, 8, 400, 3.0, rng_h, max_poses=0),
             lambda: ctx.verify_2d_device(d_kp.data_ptr(), 500, K, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr(), 3, spans, 8, 400, 3.0, rng_d,
                                          max_poses=0),
             lambda: ctx.verify_2d_batch_device(1, d_kp.data_ptr(), 500, K, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr(), 3, spans, 8, 400, 3.0,
                                                rngs, max_poses=0)]
    for call, rng in zip(calls, (rng_h, rng_d, rngs[0])):
        with pytest.raises(capi.TodError) as e:
            call()
        assert e.value.status == capi.ECAPACITY
        assert rng.draws == 1
    sc = synth.make_verify_scene(700, n_objects=6, per_object=300, visible=((1, 0.30), (4, 0.20)), matches_per_kp=3, seed=0)
    rng = capi.rng_new(1)
    with pytest.raises(capi.TodError) as e:
        ctx.verify_2d(sc["kp_xy"], K, sc["row_ptr"], sc["matches"], sc["matches_xyz"], sc["spans"], 12, 500, 3.0, rng, max_poses=1)
    assert e.value.status == capi.ECAPACITY and rng.draws == 1
