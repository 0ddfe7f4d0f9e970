"""What a pattern learned by todhip_pattern_learn_* does on the rendered-view workload of tod_amd/scenes.py, next to the built-in
pattern IN THE SAME RUN (the counterpart of tools/bit_order_chained.py, which can only reorder the bits it is given). The pattern is
learned from the training views of the first objects (as many views as fill the learner), in TODHIP_PATTERN_ORDER_MATCHER; then, per
pattern, the DB is trained (scenes.train_db, --objects x 5000 rows) and 32 detection views are described (32 x 1000 queries). Recorded:

  bits          on the detection views' descriptors (held out: other poses, other noise, 70 % clutter): mean |p - 1/2| of the bit means
                and mean / max |correlation| between two bits, over the first 128 ranks (positions 32 E[r / 32] + r % 32, r < 128: what a
                2-split block of the matrix-core matcher evaluates first) and over all 256
  non_match     mean Hamming distance between 2000 queries and 2000 random DB rows
  clutter       share of the keypoints of 16 pure-clutter images (textures in no model) with two DB rows inside radius 35
  matcher       k = 2, radius 35, matrix-core engine, adaptive block split: the split after 100 launches, the fraction of split blocks
                that went on to their second part, and the mean time of the DB-pass kernel (todhip_set_kernel_timing)
  learner       wall time of the add_view calls and of finish, keypoints, candidates, accepted per round

Prints one JSON object (and writes it to --out). Nothing here is a threshold.

    timeout 900 python tools/learned_pattern_chained.py --out profiles/learned_pattern_chained.json"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from tod_amd import capi, scenes, synth

K, RADIUS, NQ, FRAMES = 2, 35, 1000, 32
E = (0, 4, 1, 5, 2, 6, 3, 7)
ap = argparse.ArgumentParser()
ap.add_argument("--objects", type=int, default=200)
ap.add_argument("--capacity", type=int, default=32768, help="keypoints the learner collects")
ap.add_argument("--launches", type=int, default=50, help="timed matcher launches per pattern")
ap.add_argument("--out", default=None)
args = ap.parse_args()

H, W = scenes.H, scenes.W
tex = scenes.make_textures(args.objects)
ctx = capi.Context(0)

# ---- learn from the training views, object by object, until the learner is full
d_tex = torch.from_numpy(tex).cuda()
border = torch.zeros((H, W), dtype=torch.bool, device="cuda")
border[40:H - 40, 40:W - 40] = True
learner = capi.PatternLearner(ctx, args.capacity)
add_s, n_views = 0.0, 0
for o in range(args.objects):
    if learner.n_keypoints >= args.capacity:
        break
    views = scenes.TRAIN_VIEWS
    imgs, inside = scenes.render_views(d_tex, [o] * len(views), [v[0] for v in views], [v[1] for v in views], 700000 + o)
    masks = ((inside & border).to(torch.uint8) * 255).cpu().numpy()
    imgs = imgs.cpu().numpy()
    for vi in range(len(views)):
        if learner.n_keypoints >= args.capacity:
            break
        t0 = time.perf_counter()
        learner.add_view(imgs[vi], masks[vi], n_features=1300, n_levels=3, scale_factor=1.2)
        add_s += time.perf_counter() - t0
        n_views += 1
t0 = time.perf_counter()
res = learner.finish(capi.PATTERN_ORDER_MATCHER)
finish_s = time.perf_counter() - t0
t0 = time.perf_counter()
learner.finish(capi.PATTERN_ORDER_MATCHER)                             # once more: buffers exist, code objects are loaded
finish_again_s = time.perf_counter() - t0
learner.close()
out = {"what": "learned rBRIEF pattern against the built-in pattern on the rendered-view workload, one run",
       "objects": args.objects, "queries": FRAMES * NQ, "k": K, "radius": RADIUS,
       "learner": {"views": n_views, "keypoints": res["n_keypoints"], "candidates": res["n_candidates"],
                   "accepted_in_round": res["accepted_in_round"], "add_views_s": add_s, "finish_s_first_call": finish_s,
                   "finish_s": finish_again_s, "wall_s": add_s + finish_s},
       "patterns": {}}

first128 = np.array([32 * E[r // 32] + r % 32 for r in range(128)])


def bit_stats(desc, pos):
    X = np.unpackbits(desc, axis=1, bitorder="little")[:, pos].astype(np.float64)
    p = X.mean(axis=0)
    C = np.corrcoef(X, rowvar=False)
    C = np.abs(np.nan_to_num(C))
    iu = np.triu_indices(len(pos), 1)
    return {"mean_abs_p_minus_half": float(np.abs(p - 0.5).mean()), "p_min": float(p.min()), "p_max": float(p.max()),
            "mean_abs_corr": float(C[iu].mean()), "max_abs_corr": float(C[iu].max())}


bts = scenes.make_detection_batches(tex, FRAMES // 16, 16)
clutter = torch.from_numpy(np.stack([synth.make_image(scenes.TEXTURE_SEED + 500000 + f) for f in range(16)])).cuda()
d_q = torch.zeros((FRAMES, NQ, 32), dtype=torch.uint8, device="cuda")
d_qc = torch.zeros((16, NQ, 32), dtype=torch.uint8, device="cuda")
kp = torch.zeros((16, NQ, 2), device="cuda")
aux = torch.zeros((16, NQ, 4), device="cuda")
n = FRAMES * NQ
d_c = torch.zeros(n, dtype=torch.int32, device="cuda")
d_m = torch.zeros((n * K, 4), dtype=torch.int32, device="cuda")
d_x = torch.zeros((n * K, 3), device="cuda")
torch.cuda.synchronize()
rng = np.random.default_rng(7)

for name, pattern in (("built-in", None), ("learned", res["pattern"])):
    desc, pts, off = scenes.train_db(ctx, tex, rows_per_object=5000, pattern=pattern)
    n_q = []
    for b, bt in enumerate(bts):
        n_q += ctx.orb_batch_device(bt["images"].data_ptr(), 16, H * W, H, W, W, NQ, 3, 1.2, kp.data_ptr(), aux.data_ptr(),
                                    d_q[16 * b:].data_ptr(), NQ, pattern=pattern)
    n_c = ctx.orb_batch_device(clutter.data_ptr(), 16, H * W, H, W, W, NQ, 3, 1.2, kp.data_ptr(), aux.data_ptr(), d_qc.data_ptr(), NQ,
                               pattern=pattern)
    ctx.synchronize()
    q = np.concatenate([d_q[f, :n_q[f]].cpu().numpy() for f in range(FRAMES)])
    r = {"db_rows": int(off[-1]), "query_rows": int(len(q)),
         "bits_first_128_ranks": bit_stats(q, first128), "bits_all": bit_stats(q, np.arange(256))}
    qs, ds = q[rng.choice(len(q), 2000, replace=False)], desc[rng.choice(len(desc), 2000, replace=False)]
    lut = np.array([bin(i).count("1") for i in range(256)], np.uint16)
    r["mean_non_match_distance"] = float(np.mean([lut[qs[i][None, :] ^ ds].sum(axis=1).mean() for i in range(len(qs))]))
    m = capi.Context(0)
    m.set_matcher_engine("mfma")
    m.db_load(desc, pts, off)
    # clutter keypoints with two rows inside the radius
    m.match_device(d_qc.data_ptr(), 16 * NQ, K, RADIUS, d_c.data_ptr(), d_m.data_ptr(), d_x.data_ptr())
    m.synchronize()
    cc = d_c[:16 * NQ].cpu().numpy().reshape(16, NQ)
    live = np.arange(NQ)[None, :] < np.asarray(n_c)[:, None]
    r["clutter_keypoints"] = int(live.sum())
    r["clutter_share_with_two_rows_inside_radius"] = float((cc[live] == K).mean())
    # the matcher on the detection views: the adaptive split settles, then timed launches
    for _ in range(100):
        m.match_device(d_q.data_ptr(), n, K, RADIUS, d_c.data_ptr(), d_m.data_ptr(), d_x.data_ptr())
    m.synchronize()
    m.match_device(d_q.data_ptr(), n, K, RADIUS, d_c.data_ptr(), d_m.data_ptr(), d_x.data_ptr())
    m.synchronize()
    c0 = m.counters()
    m.set_kernel_timing(True)
    for _ in range(args.launches):
        m.match_device(d_q.data_ptr(), n, K, RADIUS, d_c.data_ptr(), d_m.data_ptr(), d_x.data_ptr())
    m.synchronize()
    m.set_kernel_timing(False)
    m.match_device(d_q.data_ptr(), n, K, RADIUS, d_c.data_ptr(), d_m.data_ptr(), d_x.data_ptr())   # reads the timed launches' report
    m.synchronize()
    c1 = m.counters()
    blocks = int(c1.k4x_half_blocks - c0.k4x_half_blocks)
    r["block_split_settled"] = int(c1.last_block_split)
    r["k4x_half_blocks"] = blocks
    r["k4x_half_blocks_completed"] = int(c1.k4x_half_blocks_completed - c0.k4x_half_blocks_completed)
    r["fraction_completed"] = r["k4x_half_blocks_completed"] / blocks if blocks else None
    r["mean_match_kernel_ms"] = float((c1.sum_match_kernel_ms - c0.sum_match_kernel_ms) /
                                      max(c1.n_match_kernel_launches - c0.n_match_kernel_launches, 1))
    r["queries_with_a_match_inside_radius"] = float((d_c.cpu().numpy() > 0).mean())
    m.close()
    out["patterns"][name] = r

ctx.close()
print(json.dumps(out))
if args.out:
    json.dump(out, open(args.out, "w"), indent=1)
