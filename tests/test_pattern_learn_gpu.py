"""todhip_pattern_learn_* on the GPU. The response matrix is checked by the property that defines it (its rows are the descriptor bits
todhip_orb_masked computes when chunks of the candidates are passed as `pattern`), the selection entry for entry against the
definition restated in tests/pattern_learn_ref.py on the rows read back, and the learned pattern by use: through training, ORB,
matcher and verifier on the rendered view of tests/test_end_to_end_gpu.py, and through todhip_pipeline_set_pattern. The shared inputs
(two small views, 549 crafted candidates) reach every round of the selection: tests/test_pattern_learn_cpu.py holds that condition."""
import numpy as np
import pytest

import oracle_lib as O
import pattern_learn_ref as P

pytestmark = pytest.mark.gpu


def learn(ctx, views, capacity, candidates):
    from tod_amd import capi
    L = capi.PatternLearner(ctx, capacity, candidates)
    added = [L.add_view(g, m, P.NF, P.LEVELS, P.SCALE) for g, m in views]
    return L, added


def same_as_reference(L, cands, res_rank, res_matcher):
    """finish() against the definition, run on the rows read back"""
    M, N = len(cands), L.n_keypoints
    R, pad = P.unpack_rows(L.responses(0, M), N)
    assert not pad.any()
    chosen, round_of, per_round = P.select(R)
    for res, order in ((res_rank, P.ORDER_RANK), (res_matcher, P.ORDER_MATCHER)):
        assert np.array_equal(res["chosen"], chosen) and np.array_equal(res["round_of"], round_of)
        assert res["n_keypoints"] == N and res["n_candidates"] == M and res["accepted_in_round"] == per_round
        assert np.array_equal(res["pattern"], P.layout(cands, chosen, order))
    return R, per_round


@pytest.fixture(scope="module")
def env():
    from tod_amd import capi
    e = dict(capi=capi, ctx=capi.Context(0), views=P.learn_views(), cands=P.crafted_candidates())
    e["L"], e["added"] = learn(e["ctx"], e["views"], 1000, e["cands"])
    yield e
    e["L"].close()
    e["ctx"].close()


def test_responses_are_orb_bits(env):
    ctx, L, views, cands = env["ctx"], env["L"], env["views"], env["cands"]
    counts = None
    N = sum(env["added"])
    assert L.n_keypoints == N and N % 32 != 0 and env["added"][0] % 64 != 0      # the second view starts inside a 64-bit piece
    words = L.responses(0, len(cands))
    assert words.shape == (len(cands), (N + 31) // 32)
    R, pad = P.unpack_rows(words, N)
    assert not pad.any()
    for first, count, pat in P.chunks_of(cands):
        desc = [ctx.orb(g, P.NF, P.LEVELS, P.SCALE, pattern=pat, mask=m)[2] for g, m in views]
        if counts is None:
            counts = [len(d) for d in desc]
            assert counts == env["added"]
        bits = np.unpackbits(np.concatenate(desc), axis=1, bitorder="little")
        assert np.array_equal(R[first:first + count], bits[:, :count].T), "candidates %d..%d" % (first, first + count - 1)
        part, _ = P.unpack_rows(L.responses(first, count), N)                   # the hook's own first / count
        assert np.array_equal(part, R[first:first + count])
    # and the CPU restatement of ORB yields the same matrix
    cpu = P.rows_from_orb(lambda pat: np.concatenate([O.orb(g, P.NF, P.LEVELS, P.SCALE, pattern=pat, mask=m)[2] for g, m in views]), cands)
    assert np.array_equal(R, cpu)


def test_selection_is_the_definition(env):
    capi, L = env["capi"], env["L"]
    res_rank, res_matcher = L.finish(capi.PATTERN_ORDER_RANK), L.finish(capi.PATTERN_ORDER_MATCHER)
    _, per_round = same_as_reference(L, env["cands"], res_rank, res_matcher)
    print("accepted per round", per_round)
    assert all(n >= 1 for n in per_round)                                       # every round's code ran
    lib = capi.lib()
    pat = np.zeros((256, 4), np.int8)
    assert lib.todhip_pattern_learn_finish(env["ctx"]._h, L._h, 2, capi._np_ptr(pat), None, None, None) == capi.EINVAL
    assert lib.todhip_pattern_learn_finish(env["ctx"]._h, L._h, 0, capi._np_ptr(pat), None, None, None) == capi.OK   # optional outputs
    assert np.array_equal(pat, res_rank["pattern"])


def test_capacity(env):
    capi, ctx, views, cands = env["capi"], env["ctx"], env["views"], env["cands"]
    cap = env["added"][0] - 7
    L, added = learn(ctx, views, cap, cands)
    assert added == [cap, 0] and L.n_keypoints == cap
    got, pad = P.unpack_rows(L.responses(0, len(cands)), cap)
    full, _ = P.unpack_rows(env["L"].responses(0, len(cands)), env["L"].n_keypoints)
    assert np.array_equal(got, full[:, :cap]) and not pad.any()
    L.close()
    # an empty learner has nothing to select from; argument errors with a live context
    import ctypes as C
    E = capi.PatternLearner(ctx, 10, cands)
    pat = np.zeros((256, 4), np.int8)
    assert capi.lib().todhip_pattern_learn_finish(ctx._h, E._h, 0, capi._np_ptr(pat), None, None, None) == capi.EINVAL
    E.close()
    h = C.c_void_p()
    bad = cands.copy(); bad[1] = (13, 1, 0, 0)
    for c, n, k in ((bad, len(bad), 10), (cands, 255, 10), (cands, len(cands), 0), (cands, len(cands), 32769)):
        assert capi.lib().todhip_pattern_learn_begin(ctx._h, capi._np_ptr(c), n, k, C.byref(h)) == capi.EINVAL


def test_builtin_candidates(env):
    capi, ctx = env["capi"], env["ctx"]
    cands = P.builtin_candidates()
    L, added = learn(ctx, env["views"][:1], 32768, None)
    assert added == env["added"][:1]
    res_rank, res_matcher = L.finish(capi.PATTERN_ORDER_RANK), L.finish(capi.PATTERN_ORDER_MATCHER)
    assert res_rank["n_candidates"] == len(cands)
    same_as_reference(L, cands, res_rank, res_matcher)
    L.close()


def render(texture, theta, shift_px, noise_seed):
    """tests/test_end_to_end_gpu.py's view of the fronto-parallel plane, for any image size"""
    H, W = texture.shape
    c, s = np.cos(theta), np.sin(theta)
    v2, u2 = np.mgrid[0:H, 0:W].astype(np.float32)
    x = u2 - W / 2.0 - shift_px[0]; y = v2 - H / 2.0 - shift_px[1]
    u1 = c * x + s * y + W / 2.0; v1 = -s * x + c * y + H / 2.0
    u0 = np.clip(np.floor(u1).astype(np.int64), 0, W - 2); v0 = np.clip(np.floor(v1).astype(np.int64), 0, H - 2)
    fu = np.clip(u1 - u0, 0, 1); fv = np.clip(v1 - v0, 0, 1)
    t = texture.astype(np.float32)
    img = (t[v0, u0] * (1 - fu) * (1 - fv) + t[v0, u0 + 1] * fu * (1 - fv) + t[v0 + 1, u0] * (1 - fu) * fv + t[v0 + 1, u0 + 1] * fu * fv)
    inside = (u1 >= 0) & (u1 <= W - 1) & (v1 >= 0) & (v1 <= H - 1)
    img = np.where(inside, img, 128.0)
    img += np.random.Generator(np.random.PCG64(noise_seed)).normal(0, 1.5, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def true_pose(theta, shift, Z, F):
    c, s = np.cos(theta), np.sin(theta)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float32)
    t = np.array([shift[0] * Z / F, shift[1] * Z / F, 0.0], np.float32)
    return R, t + (np.eye(3, dtype=np.float32) - R) @ np.array([0, 0, Z], np.float32)


def train(capi, ctx, texture, K, Z, n_features, pattern, border):
    H, W = texture.shape
    mask = np.zeros((H, W), np.uint8); mask[border:H - border, border:W - border] = 255
    model = capi.Model(ctx, 4000)
    model.add_observation(texture, mask, np.full((H, W), Z, np.float32), K, np.eye(3, dtype=np.float32), np.zeros(3, np.float32),
                          n_features=n_features, n_levels=3, scale_factor=1.2, pattern=pattern)
    desc, pts = model.finish(); model.close()
    return desc, pts, mask


def test_learned_pattern_in_use(env):
    """tests/test_end_to_end_gpu.py's 25 degree case with a pattern learned from the training view, in the matcher's order."""
    from tod_amd import synth
    capi, ctx = env["capi"], env["ctx"]
    H, W, F, Z = 480, 640, 525.0, 0.8
    K = np.array([[F, 0, W / 2.0], [0, F, H / 2.0], [0, 0, 1]], np.float32)
    texture = synth.make_image(321)
    mask = np.zeros((H, W), np.uint8); mask[40:H - 40, 40:W - 40] = 255
    L = capi.PatternLearner(ctx, 32768)
    assert L.add_view(texture, mask, 1500, 3, 1.2) > 800
    res = L.finish(capi.PATTERN_ORDER_MATCHER)
    L.close()
    pattern = res["pattern"]
    print("accepted per round", res["accepted_in_round"])
    assert P.in_disc(pattern) and len(np.unique(pattern, axis=0)) == 256
    desc, pts, _ = train(capi, ctx, texture, K, Z, 1500, pattern, 40)
    assert len(desc) > 800
    rng = np.random.Generator(np.random.PCG64(9))
    d2 = rng.integers(0, 256, (2000, 32), dtype=np.uint8); p2 = (rng.random((2000, 3)) * 0.2).astype(np.float32)
    off = np.array([0, len(d2), len(d2) + len(desc)], np.uint32)
    spans = ctx.db_load(np.concatenate([d2, desc]), np.concatenate([p2, pts]), off)
    theta, shift = np.deg2rad(25.0), (30.0, -18.0)
    view = render(texture, theta, shift, 5)
    kp, aux, qd = ctx.orb(view, 1000, 3, 1.2, pattern=pattern)
    o_kp, _, o_qd, _ = O.orb(view, 1000, 3, 1.2, pattern=pattern)
    assert len(kp) == len(o_kp) > 800 and np.array_equal(kp, o_kp) and np.array_equal(qd, o_qd)
    assert not np.array_equal(qd, ctx.orb(view, 1000, 3, 1.2)[2])                # (and they are not the built-in pattern's)
    v, u = np.mgrid[0:H, 0:W].astype(np.float32)
    cloud = np.stack([(u - K[0, 2]) * Z / F, (v - K[1, 2]) * Z / F, np.full((H, W), Z, np.float32)], axis=2).astype(np.float32)
    row_ptr, m, xyz = ctx.match(qd, 5, 55)
    poses = ctx.verify(kp, cloud, row_ptr, m, xyz, spans, 8, 2500, 0.01, capi.rng_new(1))
    assert len(poses) >= 1 and poses[0]["object"] == 1
    print("inlier keypoints", len(poses[0]["inliers"]))
    R_true, t_true = true_pose(theta, shift, Z, F)
    assert np.abs(poses[0]["R"] - R_true).max() < 0.02, (poses[0]["R"], R_true)
    assert np.abs(poses[0]["t"] - t_true).max() < 0.004, (poses[0]["t"], t_true)


def test_pipeline_set_pattern(env):
    """Two 240 x 320 frames through todhip_pipeline_* with a learned pattern and a DB trained with it: each frame as the
    single-frame device chain computes it with that pattern; NULL brings the built-in pattern's results back."""
    import torch
    from tod_amd import synth
    capi, ctx = env["capi"], env["ctx"]
    H, W, F, Z = 240, 320, 262.5, 0.8
    NF, KNN, RADIUS, VERIFY, TIMEOUT_MS = 400, 5, 55, (8, 2500, 0.01), 60000
    K = np.array([[F, 0, W / 2.0], [0, F, H / 2.0], [0, 0, 1]], np.float32)
    texture = np.ascontiguousarray(synth.make_image(77)[100:100 + H, 150:150 + W])
    L = capi.PatternLearner(ctx, 4096)
    assert L.add_view(texture, None, 600, 3, 1.2) > 200
    learned = L.finish(capi.PATTERN_ORDER_MATCHER)["pattern"]
    L.close()
    views = [(np.deg2rad(12.0), (9.0, -6.0)), (np.deg2rad(-20.0), (-8.0, 5.0))]
    frames = np.stack([render(texture, th, sh, 40 + i) for i, (th, sh) in enumerate(views)])
    d_frames = torch.from_numpy(frames).cuda()
    d_depth = torch.full((2, H, W), Z, dtype=torch.float32, device="cuda")
    kp = torch.zeros((NF, 2), device="cuda"); aux = torch.zeros((NF, 4), device="cuda")
    desc = torch.zeros((NF, 32), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(NF, dtype=torch.int32, device="cuda")
    matches = torch.zeros((NF * KNN, 4), dtype=torch.int32, device="cuda"); xyz = torch.zeros((NF * KNN, 3), device="cuda")
    torch.cuda.synchronize()

    def chain(f, pattern, spans):
        n = ctx.orb_device(d_frames[f].data_ptr(), H, W, W, NF, 3, 1.2, kp.data_ptr(), aux.data_ptr(), desc.data_ptr(), NF, pattern=pattern)
        ctx.match_device(desc.data_ptr(), n, KNN, RADIUS, counts.data_ptr(), matches.data_ptr(), xyz.data_ptr())
        poses = ctx.verify_device_depth(kp.data_ptr(), n, d_depth[f].data_ptr(), False, H, W, K, counts.data_ptr(), matches.data_ptr(),
                                        xyz.data_ptr(), KNN, spans, *VERIFY, capi.rng_new(1))
        ctx.synchronize()
        return dict(n_kp=n, kp_xy=kp[:n].cpu().numpy(), poses=poses)

    def same_frame(got, ref):
        assert got["n_kp"] == ref["n_kp"] and np.array_equal(got["kp_xy"], ref["kp_xy"])
        assert [p["object"] for p in got["poses"]] == [p["object"] for p in ref["poses"]]
        for a, b in zip(got["poses"], ref["poses"]):
            assert np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"]) and np.array_equal(a["inliers"], b["inliers"])

    pipe = capi.Pipeline(0, frames_per_step=2, H=H, W=W, K=K, n_features=NF, n_levels=3, scale_factor=1.2, k=KNN, radius=RADIUS,
                         verify=VERIFY, ring_depth=3)
    results = {}
    for name, pattern in (("learned", learned), ("built-in", None)):
        d, p, _ = train(capi, ctx, texture, K, Z, 600, pattern, 20)
        db = (d, p, np.array([0, len(d)], np.uint32))
        spans = ctx.db_load(*db)
        want = [chain(f, pattern, spans) for f in range(2)]
        for f, (th, sh) in enumerate(views):                                    # the comparison is not one of empty results
            R_true, t_true = true_pose(th, sh, Z, F)
            assert len(want[f]["poses"]) >= 1, "%s pattern: the reference chain finds nothing in frame %d" % (name, f)
            assert np.abs(want[f]["poses"][0]["R"] - R_true).max() < 0.03 and np.abs(want[f]["poses"][0]["t"] - t_true).max() < 0.006
        assert pipe.db_load(*db) == capi.OK
        assert pipe.set_pattern(pattern) == capi.OK
        rc, t = pipe.submit_device(d_frames.data_ptr(), d_depth.data_ptr(), 2)
        assert rc == capi.OK
        assert pipe.set_pattern(learned) == capi.EBUSY and pipe.set_pattern(None) == capi.EBUSY   # a ticket is outstanding
        rc, got = pipe.wait(t, TIMEOUT_MS)
        assert rc == capi.OK
        for f in range(2):
            same_frame(got[f], want[f])
        results[name] = want
    pipe.close()
    # the pattern changes what ORB describes, not what it detects
    assert np.array_equal(results["learned"][0]["kp_xy"], results["built-in"][0]["kp_xy"])
