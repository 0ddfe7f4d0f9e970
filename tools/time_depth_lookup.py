"""What depth images of the sensor's own size cost the verifier, on the data of bench.py's `chained` block: the DB trained by
scenes.train_db (200 objects x 5000 rows), 32 rendered detection frames, their ORB keypoints (1000 per frame) and matches (k = 2,
radius 35) in HBM, verifier settings 8 / 2500 / 0.01.
  unchanged : todhip_verify_batch_device_depth on the 32 frames with their 480 x 640 depth -- the call that existed before the depth
              lookup got a geometry. Run this with the library of the commit before and of this one in alternating processes
              (TODHIP_LIB_PATH names the library; --only-unchanged for one that lacks the new calls) and compare.
  new       : todhip_verify_batch_device_depth_rescaled on 240 x 320 depth images
  old       : 32 x todhip_rescale_depth_device into 480 x 640 images + todhip_verify_batch_device_depth on them: what a host had to do
Each call is timed on the host (the calls return when the poses are there); per route: mean, median, min and max in ms over --calls
calls after --warmup. new and old alternate call by call and must return the same poses. Prints one JSON object (and writes it to --out).

    timeout 600 python tools/time_depth_lookup.py --out profiles/depth_lookup.json"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from tod_amd import capi, scenes

K, RADIUS, NQ, FRAMES, VERIFY = 2, 35, 1000, 32, (8, 2500, 0.01)
DH, DW = 240, 320
ap = argparse.ArgumentParser()
ap.add_argument("--objects", type=int, default=200)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--calls", type=int, default=40)
ap.add_argument("--only-unchanged", action="store_true", help="time the existing call alone (a library from before the new calls)")
ap.add_argument("--label", default="", help="copied into the output (which library, which turn)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
H, W = scenes.H, scenes.W

# ---- the chained block's DB, frames, keypoints and matches
tex = scenes.make_textures(args.objects)
ctx = capi.Context(0)
desc, pts, off = scenes.train_db(ctx, tex, rows_per_object=5000)
spans = ctx.db_load(desc, pts, off)
bt = scenes.make_detection_batches(tex, 1, FRAMES)[0]
kp = torch.zeros((FRAMES, NQ, 2), device="cuda")
aux = torch.zeros((FRAMES, NQ, 4), device="cuda")
d_q = torch.zeros((FRAMES, NQ, 32), dtype=torch.uint8, device="cuda")
n = FRAMES * NQ
d_c = torch.zeros(n, dtype=torch.int32, device="cuda")
d_m = torch.zeros((n * K, 4), dtype=torch.int32, device="cuda")
d_x = torch.zeros((n * K, 3), device="cuda")
n_kp = ctx.orb_batch_device(bt["images"].data_ptr(), FRAMES, H * W, H, W, W, NQ, 3, 1.2, kp.data_ptr(), aux.data_ptr(), d_q.data_ptr(), NQ)
ctx.match_device(d_q.data_ptr(), n, K, RADIUS, d_c.data_ptr(), d_m.data_ptr(), d_x.data_ptr())
c2 = d_c.view(FRAMES, NQ)
for f, nf in enumerate(n_kp):                                     # a frame with fewer keypoints pads with counts 0 (todhip.h)
    if nf < NQ:
        c2[f, nf:] = 0
d_half = bt["depth"][:, ::2, ::2].contiguous()
d_full = torch.zeros((FRAMES, H, W), device="cuda")
torch.cuda.synchronize()
ctx.synchronize()


def rngs():
    return (capi.Rng * FRAMES)(*[capi.rng_new(1) for _ in range(FRAMES)])


def unchanged(depth=None):
    d = bt["depth"] if depth is None else depth
    return ctx.verify_batch_device(FRAMES, kp.data_ptr(), NQ, 0, H, W, d_c.data_ptr(), d_m.data_ptr(), d_x.data_ptr(), K, spans, *VERIFY,
                                   rngs(), depth=(d.data_ptr(), False, scenes.K))


def new():
    return ctx.verify_batch_device_depth_rescaled(FRAMES, kp.data_ptr(), NQ, d_half.data_ptr(), False, DH, DW, False, H, W, scenes.K,
                                                  d_c.data_ptr(), d_m.data_ptr(), d_x.data_ptr(), K, spans, *VERIFY, rngs())


def old():
    for f in range(FRAMES):
        ctx.rescale_depth_device(d_half[f].data_ptr(), False, DH, DW, d_full[f].data_ptr(), H, W)
    return unchanged(d_full)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def summary(ms):
    a = np.array(ms)
    return {"mean_ms": round(float(a.mean()), 4), "median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a.min()), 4),
            "max_ms": round(float(a.max()), 4), "calls": len(ms)}


def same(a, b):
    return all(len(x) == len(y) and all(p["object"] == q["object"] and np.array_equal(p["R"], q["R"]) and np.array_equal(p["t"], q["t"])
                                        and np.array_equal(p["inliers"], q["inliers"]) for p, q in zip(x, y)) for x, y in zip(a, b))


out = {"what": __doc__.split("\n")[0], "label": args.label, "library": os.environ.get("TODHIP_LIB_PATH", "in-tree"),
       "objects": args.objects, "db_rows": int(off[-1]), "frames": FRAMES, "nq": NQ, "k": K, "radius": RADIUS, "verify": list(VERIFY),
       "keypoints": int(sum(n_kp))}
for _ in range(args.warmup):
    ref = unchanged()
ms = [timed(unchanged)[0] for _ in range(args.calls)]
out["unchanged"] = summary(ms)
out["unchanged"]["poses"] = sum(len(p) for p in ref)
out["unchanged"]["frames_with_the_rendered_object"] = sum(any(p["object"] == bt["objects"][f] for p in ref[f]) for f in range(FRAMES))
if not args.only_unchanged:
    for _ in range(args.warmup):
        r_new, r_old = new(), old()
    t_new, t_old = [], []
    for _ in range(args.calls):                                   # alternating, so that clocks and neighbours are shared
        t_new.append(timed(new)[0])
        t_old.append(timed(old)[0])
    out["new_240x320"] = summary(t_new)
    out["old_32_rescales_then_verify"] = summary(t_old)
    out["new_equals_old"] = bool(same(r_new, r_old))
    out["new_240x320"]["poses"] = sum(len(p) for p in r_new)
    out["new_240x320"]["frames_with_the_rendered_object"] = sum(any(p["object"] == bt["objects"][f] for p in r_new[f]) for f in range(FRAMES))
ctx.close()
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
