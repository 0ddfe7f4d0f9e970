"""What training from a batch of device-resident views costs, on views of bench.py's `chained` block: scenes.render_views of 8 textures
x scenes.TRAIN_VIEWS = 32 views of 480 x 640, their masks (the plane minus a border) and the constant depth, 1300 features, 3 levels.
  single    : todhip_model_add_observation on the views in turn, host time per call -- the call that existed before the batch. Run this
              with the library of the commit before and of this one in alternating processes (TODHIP_LIB_PATH names the library;
              --only-single for one that lacks the batch call) and compare.
  a         : 32 single calls from host arrays into a fresh model, host time of the 32 together
  b         : one todhip_model_add_observations_device call on the same views, resident on the device
  c         : b plus uploading the same bytes (gray, mask, depth of the 32 views) from host arrays first
  train_db  : scenes.train_db on --textures textures with batched off and on, seconds per call
a, b and c alternate call by call; the models of a and b must be the same bytes. Each timed call ends in the library's own stream
synchronization (and c's uploads in torch's). Prints one JSON object (and writes it to --out).

    timeout 600 python tools/time_train_batch.py --out profiles/train_batch.json"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from tod_amd import capi, scenes

NF, LEVELS, SCALE = 1300, 3, 1.2
ap = argparse.ArgumentParser()
ap.add_argument("--views", type=int, default=32)
ap.add_argument("--warmup", type=int, default=32)
ap.add_argument("--calls", type=int, default=320, help="single calls timed")
ap.add_argument("--reps", type=int, default=20, help="timed repetitions of a, b and c")
ap.add_argument("--textures", type=int, default=20, help="of the train_db comparison (0: skip)")
ap.add_argument("--only-single", action="store_true", help="time the existing call alone (a library from before the batch call)")
ap.add_argument("--label", default="", help="copied into the output (which library, which turn)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
H, W, V = scenes.H, scenes.W, args.views
assert 0 < V <= capi.MAX_TRAIN_BATCH_VIEWS

# ---- the views, as scenes.train_db makes them
n_tex = (V + len(scenes.TRAIN_VIEWS) - 1) // len(scenes.TRAIN_VIEWS)
tex = torch.from_numpy(scenes.make_textures(n_tex)).cuda()
ids = [v // len(scenes.TRAIN_VIEWS) for v in range(V)]
views = [scenes.TRAIN_VIEWS[v % len(scenes.TRAIN_VIEWS)] for v in range(V)]
d_imgs, inside = scenes.render_views(tex, ids, [v[0] for v in views], [v[1] for v in views], 700000)
border = torch.zeros((H, W), dtype=torch.bool, device="cuda")
border[40:H - 40, 40:W - 40] = True
d_masks = ((inside & border).to(torch.uint8) * 255).contiguous()
d_imgs = d_imgs.contiguous()
d_depth = torch.full((V, H, W), scenes.Z, dtype=torch.float32, device="cuda")
torch.cuda.synchronize()
imgs, masks, depth = d_imgs.cpu().numpy(), d_masks.cpu().numpy(), d_depth.cpu().numpy()
poses = [scenes.view_pose(*v) for v in views]
R, T = np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses])
ctx = capi.Context(0)
ORB = dict(n_features=NF, n_levels=LEVELS, scale_factor=SCALE)


def summary(ms):
    a = np.array(ms)
    return {"mean_ms": round(float(a.mean()), 4), "median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a.min()), 4),
            "max_ms": round(float(a.max()), 4), "calls": len(ms)}


def single_calls(model, n, first=0):
    ms, rows = [], 0
    for i in range(first, first + n):
        v = i % V
        t0 = time.perf_counter()
        rows += model.add_observation(imgs[v], masks[v], depth[v], scenes.K, R[v], T[v], **ORB)
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms, rows


def route_a():
    model = capi.Model(ctx, V * NF + 16)
    t0 = time.perf_counter()
    single_calls(model, V)
    ms = (time.perf_counter() - t0) * 1e3
    return ms, model


def batch_call(model, g, m, d):
    return model.add_observations_device(g.data_ptr(), m.data_ptr(), d.data_ptr(), V, H, W, scenes.K, R, T, **ORB)


def route_b():
    model = capi.Model(ctx, V * NF + 16)
    t0 = time.perf_counter()
    batch_call(model, d_imgs, d_masks, d_depth)
    return (time.perf_counter() - t0) * 1e3, model


def route_c():
    model = capi.Model(ctx, V * NF + 16)
    t0 = time.perf_counter()
    g, m, d = torch.from_numpy(imgs).cuda(), torch.from_numpy(masks).cuda(), torch.from_numpy(depth).cuda()
    torch.cuda.synchronize()
    batch_call(model, g, m, d)
    return (time.perf_counter() - t0) * 1e3, model


out = {"what": __doc__.split("\n")[0], "label": args.label, "library": os.environ.get("TODHIP_LIB_PATH", "in-tree"), "views": V,
       "H": H, "W": W, "n_features": NF, "n_levels": LEVELS}
model = capi.Model(ctx, (args.warmup + args.calls) * NF + 16)
single_calls(model, args.warmup)
ms, rows = single_calls(model, args.calls, args.warmup)
model.close()
out["single"] = summary(ms)
out["single"]["rows_per_call"] = round(rows / args.calls, 1)
if not args.only_single:
    for _ in range(3):
        for fn in (route_a, route_b, route_c):
            fn()[1].close()
    t = {"a": [], "b": [], "c": []}
    for rep in range(args.reps):                                  # alternating, so that clocks and neighbours are shared
        got = {}
        for key, fn in (("a", route_a), ("b", route_b), ("c", route_c)):
            ms, model = fn()
            t[key].append(ms)
            if rep == 0:
                got[key] = model.finish()
            model.close()
        if rep == 0:
            same = all(np.array_equal(got[k][0], got["a"][0]) and np.array_equal(got[k][1].view(np.uint32), got["a"][1].view(np.uint32)) for k in "bc")
            out["models_equal"], out["model_rows"] = bool(same), int(len(got["a"][0]))
    out["a_32_single_calls_from_host"] = summary(t["a"])
    out["b_one_batch_call_device_resident"] = summary(t["b"])
    out["c_upload_then_batch_call"] = summary(t["c"])
    out["upload_bytes"] = int(imgs.nbytes + masks.nbytes + depth.nbytes)
    if args.textures:
        textures = scenes.make_textures(args.textures)
        scenes.train_db(ctx, textures[:2], batched=False); scenes.train_db(ctx, textures[:2], batched=True)
        secs = {False: [], True: []}
        res = {}
        for _ in range(2):
            for batched in (False, True):
                t0 = time.perf_counter()
                res[batched] = scenes.train_db(ctx, textures, batched=batched)
                secs[batched].append(round(time.perf_counter() - t0, 4))
        out["train_db"] = {"textures": args.textures, "views_per_texture": len(scenes.TRAIN_VIEWS), "rows": int(res[False][2][-1]),
                           "unbatched_s": secs[False], "batched_s": secs[True],
                           "equal": bool(all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(res[False], res[True])))}
ctx.close()
print(json.dumps(out))
if args.out:
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
