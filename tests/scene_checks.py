"""Scenes and the frame-against-oracle comparison shared by tests/test_sprint_gpu.py (and its child process) and the driver's
smoke(): a plain module, no pytest."""
import os

import numpy as np

import oracle_lib as O
from tod_amd import capi, synth

POSE_TOL = 1e-3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chained_frames.npz")


def chained_scene(d, f, H=480, W=640):
    """Frame f of tests/golden/chained_frames.npz (this library's ORB keypoints + matcher output on rendered views against a DB
    of 200 trained objects, tools/chained_objects.py) as the host-buffer inputs of todhip_verify / the oracle."""
    K, Z = d["K"], np.float32(d["Z"])
    v, u = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    cloud = np.stack([(u - K[0, 2]) * Z / K[0, 0], (v - K[1, 2]) * Z / K[1, 1], np.full((H, W), Z, np.float32)], -1).astype(np.float32)
    cnt = d["counts"][f].astype(np.int64)
    k = d["matches"].shape[2]
    row_ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    sel = np.arange(k)[None, :] < cnt[:, None]
    m = d["matches"][f][sel]
    mm = np.zeros(len(m), capi.DMATCH_DTYPE)
    mm["queryIdx"], mm["trainIdx"], mm["imgIdx"] = m[:, 0], m[:, 1], m[:, 2]
    mm["distance"] = np.ascontiguousarray(m[:, 3]).view(np.float32)
    return dict(kp_xy=np.ascontiguousarray(d["kp"][f]), cloud=cloud, row_ptr=row_ptr, matches=mm,
                matches_xyz=np.ascontiguousarray(d["xyz"][f][sel], np.float32), spans=d["spans"])


def compare_frame(ctx, sc, min_inliers=8, n_iter=2500, err=0.01, seed=1):
    rng_o, rng_g = O.rng_new(seed), capi.rng_new(seed)
    rc, o_poses, o_rounds = O.verify(sc["kp_xy"], sc["cloud"], sc["row_ptr"], sc["matches"], sc["matches_xyz"], sc["spans"],
                                     min_inliers, n_iter, err, rng_o)
    assert rc == 0
    g_poses = ctx.verify(sc["kp_xy"], sc["cloud"], sc["row_ptr"], sc["matches"], sc["matches_xyz"], sc["spans"], min_inliers, n_iter,
                         err, rng_g)
    g_rounds = ctx.verify_trace()
    cnt = ctx.counters()
    o_r = [r for r in o_rounds if not (r.iterations == 0 and r.draws_after == r.draws_before and r.best_count == 0)]
    g_r = [r for r in g_rounds if not (r.iterations == 0 and r.draws_after == r.draws_before)]
    got = [(g.iterations, g.best_iteration, g.best_count, g.draws_before, g.draws_after) for g in g_r]
    want = [(o.iterations, o.best_iteration, o.best_count, o.draws_before, o.draws_after) for o in o_r]
    first_bad = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None)
    assert first_bad is None, (first_bad, got[first_bad], want[first_bad], g_r[first_bad].object)
    assert len(got) == len(want)
    assert rng_g.draws == rng_o.draws and list(rng_g.s) == list(rng_o.s) and (rng_g.f, rng_g.b) == (rng_o.f, rng_o.b)
    assert [p["object"] for p in g_poses] == [p["object"] for p in o_poses]
    for g, o in zip(g_poses, o_poses):
        assert np.array_equal(g["inliers"], o["inliers"])
        assert np.abs(g["R"] - o["R"]).max() < POSE_TOL and np.abs(g["t"] - o["t"]).max() < POSE_TOL
    return g_poses, g_r, cnt


def small_objects_scene(seed, n_kp=700, n_objects=120, small=((5, 0.05), (33, 0.045), (34, 0.06), (90, 0.035)), big=(60, 0.25),
                        matches_per_kp=2):
    """Several objects that are really there with 20-45 true matches each (poses accepted by the device path: growth, invalidation,
    a second round), one of ~175 matches in between (the tick-by-tick path), and ~115 objects of random matches."""
    vis = tuple(sorted(small + (big,)))
    place = [(0.3 + 0.5 * i, (-0.36 + 0.18 * i, -0.2 + 0.1 * (i % 3), 0.9 + 0.05 * i)) for i in range(len(vis))]   # all in view
    return synth.make_verify_scene(n_kp, n_objects=n_objects, per_object=300, visible=vis, matches_per_kp=matches_per_kp, seed=seed,
                                   nan_frac=0.05, placements=place)
