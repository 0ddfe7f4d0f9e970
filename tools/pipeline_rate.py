"""Frames/s of the C pipeline (todhip_pipeline_*) on bench.py's data-chained workload: the DB trained by todhip_model_* on rendered
views of --objects textured planes, 4 batches of --batch rendered detection frames resident on the GPU, device-form submit with
ring_depth tickets in flight. The figure to set beside `chained.frames_per_s` of `python bench.py --full` (same batch size, worker
counts, ring depth, matcher and verifier parameters: the defaults here are bench.py's). Prints one JSON line.

    python tools/pipeline_rate.py [--steps 120] [--repeats 5]"""
import os
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")      # as bench.py: before the HIP runtime starts (streams and hardware queues)
import argparse
import json
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=200)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--radius", type=int, default=35)
    ap.add_argument("--iterations", type=int, default=2500)
    ap.add_argument("--min-inliers", type=int, default=8)
    ap.add_argument("--orb-workers", type=int, default=1)
    ap.add_argument("--verify-workers", type=int, default=2)
    ap.add_argument("--ring-depth", type=int, default=4)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--engine", choices=("auto", "valu", "mfma"), default="auto")
    args = ap.parse_args()
    import torch
    from tod_amd import capi, scenes
    B, D = args.batch, args.ring_depth
    textures = scenes.make_textures(args.objects)
    tctx = capi.Context(0)
    desc, pts, off = scenes.train_db(tctx, textures, rows_per_object=5000)
    tctx.close()
    batches = scenes.make_detection_batches(textures, 4, B)
    torch.cuda.synchronize()
    pipe = capi.Pipeline(0, frames_per_step=B, H=scenes.H, W=scenes.W, K=scenes.K, n_features=args.nq, n_levels=3, scale_factor=1.2,
                         k=args.k, radius=args.radius, verify=(args.min_inliers, args.iterations, 0.01), orb_workers=args.orb_workers,
                         verify_workers=args.verify_workers, ring_depth=D, max_poses_per_frame=16)
    m = pipe.matcher()
    m.set_matcher_engine(args.engine)
    assert pipe.db_load(desc, pts, off) == capi.OK
    tally = dict(frames=0, right_object=0, pose_ok=0, poses=0)

    def take(ticket, step):
        rc, res = pipe.wait(ticket, 120000, want_kp=False)
        if rc != capi.OK:
            raise capi.TodError(rc, "todhip_pipeline_wait")
        bt = batches[step % len(batches)]
        for f, r in enumerate(res):
            tally["frames"] += 1
            tally["poses"] += len(r["poses"])
            hit = [p for p in r["poses"] if p["object"] == bt["objects"][f]]
            if hit:
                tally["right_object"] += 1
                Rt, tt = bt["poses"][f]
                tally["pose_ok"] += bool(np.abs(hit[0]["R"] - Rt).max() < 0.03 and np.abs(hit[0]["t"] - tt).max() < 0.006)

    def run(n_steps):
        """n_steps steps, D tickets in flight: submit until the ring is full, then take the oldest."""
        flight = []
        for i in range(n_steps):
            bt = batches[i % len(batches)]
            while True:
                rc, t = pipe.submit_device(bt["images"].data_ptr(), bt["depth"].data_ptr(), B)
                if rc != capi.EBUSY:
                    break
                take(*flight.pop(0))
            if rc != capi.OK:
                raise capi.TodError(rc, "todhip_pipeline_submit_device")
            flight.append((t, i))
        for item in flight:
            take(*item)

    run(max(3, 2 * D))                                   # fill: buffers, ORB graphs, the matcher's block form
    m.set_kernel_timing(True)
    for key in tally:
        tally[key] = 0
    s0 = pipe.stats()
    secs = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        run(args.steps)
        secs.append(time.perf_counter() - t0)
    s1 = pipe.stats()
    fps = sorted(args.steps * B / s for s in secs)
    n_steps = max(s1["steps"] - s0["steps"], 1)
    n_f = max(tally["frames"], 1)
    launches = s1["n_match_kernel_launches"] - s0["n_match_kernel_launches"]
    out = {"what": "todhip_pipeline_submit_device / todhip_pipeline_wait on the data-chained workload, %d tickets in flight" % D,
           "db_rows": int(off[-1]), "db_objects": args.objects, "k": args.k, "radius": args.radius, "frames_per_step": B,
           "steps": args.steps, "repeats": args.repeats, "orb_workers": args.orb_workers, "verify_workers": args.verify_workers,
           "ring_depth": D, "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"),
           "frames_per_s": {"median": statistics.median(fps), "min": fps[0], "max": fps[-1]},
           "ms_per_step": statistics.median(secs) / args.steps * 1e3,
           "stage_host_ms_per_step": {key: 1e3 * (s1[key] - s0[key]) / n_steps for key in ("orb_s", "match_issue_s", "verify_s")},
           "matcher_launch_ms": (s1["sum_match_kernel_ms"] - s0["sum_match_kernel_ms"]) / max(launches, 1), "matcher_launches": launches,
           "keypoints_per_frame": (s1["keypoints"] - s0["keypoints"]) / max(s1["frames"] - s0["frames"], 1),
           "poses_per_frame": tally["poses"] / n_f, "frames_with_the_right_object": tally["right_object"] / n_f,
           "frames_with_the_rendering_pose": tally["pose_ok"] / n_f}
    pipe.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
