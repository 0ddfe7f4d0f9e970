#!/usr/bin/env python3
"""Train an object model from one RGB-D view and detect it in another view -- the whole path on one MI355X:

    todhip_model_*  (masked ORB, keypoint validation, back-projection)   <- src/training/Trainer.cpp
    todhip_db_load                                                        <- DescriptorMatcher::parameter_callback
    todhip_orb -> todhip_match -> todhip_verify                           <- detector.py: features -> matcher -> guess generator

Synthetic data (a textured plane rendered at a known pose), so that the recovered pose can be checked.
Run on a machine with an MI355X:  python examples/train_and_detect.py [--learn-pattern] [--compact DIST,HAM] [--batched]
--learn-pattern: first learn an rBRIEF test pattern from the training view (todhip_pattern_learn_*), then train and detect with it.
--compact DIST,HAM: train from two views a few degrees apart and merge the model's near-duplicate rows (todhip_model_compact: rows
within DIST metres and HAM descriptor bits of a row kept before them go), e.g. --compact 0.003,24.
--batched: train from the same two views, resident on the device, in one call (todhip_model_add_observations_device; needs torch to
hold the device buffers). The model is the one that two todhip_model_add_observation calls give.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tod_amd import capi, synth   # noqa: E402

H, W, F, Z = 480, 640, 525.0, 0.8
K = np.array([[F, 0, W / 2.0], [0, F, H / 2.0], [0, 0, 1]], np.float32)


def render(texture, theta, shift_px):
    """The plane rotated by theta about the optical axis and shifted in the image (bilinear resampling)."""
    c, s = np.cos(theta), np.sin(theta)
    v2, u2 = np.mgrid[0:H, 0:W].astype(np.float32)
    x, y = u2 - W / 2.0 - shift_px[0], v2 - H / 2.0 - shift_px[1]
    u1, v1 = c * x + s * y + W / 2.0, -s * x + c * y + H / 2.0
    u0 = np.clip(np.floor(u1).astype(np.int64), 0, W - 2); v0 = np.clip(np.floor(v1).astype(np.int64), 0, H - 2)
    fu, fv = np.clip(u1 - u0, 0, 1), np.clip(v1 - v0, 0, 1)
    t = texture.astype(np.float32)
    img = t[v0, u0] * (1 - fu) * (1 - fv) + t[v0, u0 + 1] * fu * (1 - fv) + t[v0 + 1, u0] * (1 - fu) * fv + t[v0 + 1, u0 + 1] * fu * fv
    inside = (u1 >= 0) & (u1 <= W - 1) & (v1 >= 0) & (v1 <= H - 1)
    return np.clip(np.rint(np.where(inside, img, 128.0)), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--learn-pattern", action="store_true", help="learn the ORB test pattern from the training view first")
    ap.add_argument("--compact", metavar="DIST,HAM", help="train from two views and merge near-duplicate rows, e.g. 0.003,24")
    ap.add_argument("--batched", action="store_true", help="train from two device-resident views in one call")
    args = ap.parse_args()
    ctx = capi.Context(0)
    texture = synth.make_image(321)
    depth = np.full((H, W), Z, np.float32)
    mask = np.zeros((H, W), np.uint8); mask[40:H - 40, 40:W - 40] = 255

    # --- optionally the test pattern itself: model and queries must then both be described with it
    pattern = None
    if args.learn_pattern:
        learner = capi.PatternLearner(ctx)
        n = learner.add_view(texture, mask, n_features=1500, n_levels=3, scale_factor=1.2)
        res = learner.finish(capi.PATTERN_ORDER_MATCHER); learner.close()
        pattern = res["pattern"]
        print("pattern: learned from %d keypoints and %d candidate tests, accepted per round %s" %
              (n, res["n_candidates"], res["accepted_in_round"]))

    # --- training: one observation (two with --compact or --batched); the object frame is the training camera frame (R = I, T = 0)
    model = capi.Model(ctx, 4000)
    views = [(texture, np.eye(3, dtype=np.float32), np.zeros(3, np.float32))]
    if args.compact or args.batched:
        # a second view, 5 degrees on and shifted: p_cam = R2 p_obj + t2, which is what cameraToWorld undoes
        th2, shift2 = np.deg2rad(5.0), (7.0, -5.0)
        c2, s2 = np.cos(th2), np.sin(th2)
        R2 = np.array([[c2, -s2, 0], [s2, c2, 0], [0, 0, 1]], np.float32)
        t2 = np.array([shift2[0] * Z / F, shift2[1] * Z / F, 0.0], np.float32) + (np.eye(3, dtype=np.float32) - R2) @ np.array([0, 0, Z], np.float32)
        views.append((render(texture, th2, shift2), R2, t2.astype(np.float32)))
    if args.batched:
        import torch
        n = len(views)
        d_gray = torch.from_numpy(np.stack([v[0] for v in views])).cuda()
        d_mask = torch.from_numpy(np.stack([mask] * n)).cuda()
        d_depth = torch.from_numpy(np.stack([depth] * n)).cuda()
        torch.cuda.synchronize()                                   # the uploads ran on torch's stream, the call runs on the context's
        added = model.add_observations_device(d_gray.data_ptr(), d_mask.data_ptr(), d_depth.data_ptr(), n, H, W, K,
                                              np.stack([v[1] for v in views]), np.stack([v[2] for v in views]), n_features=1500,
                                              n_levels=3, scale_factor=1.2, pattern=pattern)
        print("batched: %d views in one call, rows added per view %s" % (n, added.tolist()))
    else:
        for img, R, t in views:
            model.add_observation(img, mask, depth, K, R, t, n_features=1500, n_levels=3, scale_factor=1.2, pattern=pattern)
    if args.compact:
        dist, ham = args.compact.split(",")
        before, after = model.compact(float(dist), int(ham))
        print("compact: %d rows before, %d after" % (before, after))
    desc, pts = model.finish(); model.close()
    print("model: %d descriptors with 3D points" % len(desc))
    spans = ctx.db_load(desc, pts, np.array([0, len(desc)], np.uint32))

    # --- detection in a rotated, shifted view
    theta, shift = np.deg2rad(33.0), (24.0, -15.0)
    view = render(texture, theta, shift)
    kp, aux, q = ctx.orb(view, 1000, 3, 1.2, pattern=pattern)
    v, u = np.mgrid[0:H, 0:W].astype(np.float32)
    cloud = np.stack([(u - K[0, 2]) * Z / F, (v - K[1, 2]) * Z / F, np.full((H, W), Z, np.float32)], axis=2).astype(np.float32)
    row_ptr, matches, xyz = ctx.match(q, 5, 55)
    poses = ctx.verify(kp, cloud, row_ptr, matches, xyz, spans, 8, 2500, 0.01, capi.rng_new(1))
    c, s = np.cos(theta), np.sin(theta)
    R_true = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float32)
    t_true = np.array([shift[0] * Z / F, shift[1] * Z / F, 0.0], np.float32) + (np.eye(3, dtype=np.float32) - R_true) @ np.array([0, 0, Z], np.float32)
    for p in poses:
        print("object %d: %d inlier keypoints\nR =\n%s\nt = %s" % (p["object"], len(p["inliers"]), np.round(p["R"], 4), np.round(p["t"], 4)))
    if poses:
        print("max |R - R_true| = %.4f, max |t - t_true| = %.4f m" % (np.abs(poses[0]["R"] - R_true).max(), np.abs(poses[0]["t"] - t_true).max()))
    # --- the same detection from pixels alone (no depth, no cloud): the PnP branch, todhip_verify_2d
    poses2 = ctx.verify_2d(kp, K, row_ptr, matches, xyz, spans, 8, 1000, 3.0, capi.rng_new(1))
    for p in poses2:
        print("2D only -- object %d: %d inlier keypoints, max |R - R_true| = %.4f, max |t - t_true| = %.4f m" %
              (p["object"], len(p["inliers"]), np.abs(p["R"] - R_true).max(), np.abs(p["t"] - t_true).max()))
    ctx.close()


if __name__ == "__main__":
    main()
