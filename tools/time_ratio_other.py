"""Cost and effect of Lowe's ratio test against another object (todhip_set_ratio_test_other; tod_amd/csrc/match_other.hip).

Cost: todhip_match_device at the C3 shape -- 32 frames x 1000 queries, k = 2, radius 35, 1M rows -- with the setting off and on in one
process, alternating call by call after a warm-up, each call between two events on the context's stream; medians with min / max per
turn. Independent-bit descriptors put no row inside radius 35 of a random query (every limit would be 0 and the pass would never look
at a block), so the DB is tools/time_cross_check.py's: 200 000 base rows in 5 consecutive variants each (0-8 flipped bits), 200 objects,
queries = rows with 0-20 flipped bits. A library without the setter (TODHIP_LIB_PATH naming the parent commit's build) is timed with
"off" alone: the same call, the same way, for the comparison across commits. --kernel-stats takes the CSV of a separate
`rocprofv3 --kernel-trace --stats` run of this script and copies the other-object kernel's own time from it.

Effect: on the rendered-view DB of tod_amd/scenes.py (the chained workload: objects trained from four views each, detection frames
showing ~30 % object and ~70 % clutter), a query's nearest match is TRUE when it names the visible object and its model point, under
the frame's true pose, projects within 3 px of the keypoint; every other nearest match is clutter. Reported: the share of true and of
clutter nearest matches that survive the classic test and this one at --ratio.

    timeout 900 python tools/time_ratio_other.py --out profiles/ratio_other.json"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from tod_amd import capi, scenes

ap = argparse.ArgumentParser()
ap.add_argument("--bases", type=int, default=200000)
ap.add_argument("--frames", type=int, default=32)
ap.add_argument("--queries", type=int, default=1000, help="per frame")
ap.add_argument("--radius", type=int, default=35)
ap.add_argument("--ratio", type=float, default=0.8)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--launches", type=int, default=30, help="timed calls per setting and turn")
ap.add_argument("--turns", type=int, default=3)
ap.add_argument("--objects", type=int, default=24, help="objects of the rendered-view DB")
ap.add_argument("--skip-cost", action="store_true")
ap.add_argument("--skip-effect", action="store_true")
ap.add_argument("--kernel-stats", default=None, help="kernel stats CSV of a rocprofv3 --kernel-trace --stats run of this script")
ap.add_argument("--parent", default=None, help="JSON this script wrote with TODHIP_LIB_PATH = the parent commit's build, in the same GPU visit")
ap.add_argument("--out", default=None)
args = ap.parse_args()
K, VARIANTS = 2, 5
NOT = "not measured"
HAVE = hasattr(capi.lib(), "todhip_set_ratio_test_other")
rng = np.random.default_rng(1)


def flip(rows, max_bits):
    """every row with 0..max_bits random bit positions toggled (a position drawn twice toggles back: fewer flips, never more)"""
    out = rows.copy()
    n = rng.integers(0, max_bits + 1, len(rows))
    for j in range(max_bits):
        pos = rng.integers(0, 256, len(rows))
        on = n > j
        out[np.nonzero(on)[0], pos[on] >> 3] ^= (1 << (pos[on] & 7)).astype(np.uint8)
    return out


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms)), "n": len(ms)}


def set_other(c, ratio):
    capi._call("todhip_set_ratio_test_other", c._h, ratio)


def cost():
    base = rng.integers(0, 256, (args.bases, 32), dtype=np.uint8)
    desc = flip(np.repeat(base, VARIANTS, axis=0), 8)
    rows = len(desc)
    pts = rng.standard_normal((rows, 3)).astype(np.float32)
    off = np.linspace(0, rows, 201).astype(np.uint32)
    F, Q = args.frames, args.queries
    nq = F * Q
    pick = np.concatenate([rng.choice(rng.choice(args.bases, 400, replace=False), Q) for _ in range(F)])
    q = flip(base[pick], 20)
    c = capi.Context(0)
    c.db_load(desc, pts, off)
    d_q = torch.from_numpy(q).cuda()
    cnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
    mm = torch.zeros((nq * K, 4), dtype=torch.int32, device="cuda")
    xx = torch.zeros((nq * K, 3), device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.ExternalStream(c.stream)
    settings = ("off", "on") if HAVE else ("off",)

    def call(setting):
        if HAVE:
            set_other(c, args.ratio if setting == "on" else 0.0)
        with torch.cuda.stream(st):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            c.match_device(d_q.data_ptr(), nq, K, args.radius, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr())
            e1.record()
            e1.synchronize()
        return e0.elapsed_time(e1)
    for _ in range(args.warmup):
        for s in settings:
            call(s)
    kept = {}
    for s in settings:
        call(s)
        c.synchronize()
        kept[s] = int((cnt > 0).sum())
    turns = {s: [] for s in settings}
    for _ in range(args.turns):
        ms = {s: [] for s in settings}
        for _ in range(args.launches):
            for s in settings:                                   # alternating, call by call
                ms[s].append(call(s))
        for s in settings:
            turns[s].append(stats(ms[s]))
    if HAVE:
        set_other(c, 0.0)
    c.close()
    out = {"what": "todhip_match_device, %d frames x %d queries, k = %d, radius %d, %d rows in 200 objects (%d base rows x %d consecutive "
                   "variants, queries = rows with 0-20 flipped bits); one call between two events, setting off / on alternating"
                   % (F, Q, K, args.radius, rows, args.bases, VARIANTS),
           "queries_with_a_match": kept, "call_ms_turns": turns}
    for s in settings:
        med = [t["median"] for t in turns[s]]
        out["call_ms_" + s] = {"median_of_turn_medians": float(np.median(med)), "min": min(t["min"] for t in turns[s]),
                               "max": max(t["max"] for t in turns[s]), "turn_median_spread": float(max(med) - min(med))}
    out["on_over_off"] = out["call_ms_on"]["median_of_turn_medians"] / out["call_ms_off"]["median_of_turn_medians"] if HAVE else NOT
    return out


def effect():
    textures = scenes.make_textures(args.objects)
    c = capi.Context(0)
    desc, pts, off = scenes.train_db(c, textures)
    c.db_load(desc, pts, off)
    batches = scenes.make_detection_batches(textures, 4, 8)
    NF, RADIUS = 1000, 55
    kp = torch.zeros((NF, 2), device="cuda")
    aux = torch.zeros((NF, 4), device="cuda")
    dd = torch.zeros((NF, 32), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(NF, dtype=torch.int32, device="cuda")
    mm = torch.zeros((NF * K, 4), dtype=torch.int32, device="cuda")
    xx = torch.zeros((NF * K, 3), device="cuda")
    tally = {name: {"true": 0, "clutter": 0} for name in ("no_test", "classic", "other_object")}
    off64 = off.astype(np.int64)
    for b in batches:
        for f in range(len(b["objects"])):
            torch.cuda.synchronize()
            n = c.orb_device(b["images"][f].data_ptr(), scenes.H, scenes.W, scenes.W, NF, 3, 1.2, kp.data_ptr(), aux.data_ptr(), dd.data_ptr(), NF)
            if not n:
                continue
            alive = {}
            for name, classic, other in (("no_test", 0.0, 0.0), ("classic", args.ratio, 0.0), ("other_object", 0.0, args.ratio)):
                c.set_ratio_test(classic)
                set_other(c, other)
                c.match_device(dd.data_ptr(), n, K, RADIUS, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr())
                c.synchronize()
                alive[name] = cnt[:n].cpu().numpy() > 0
                if name == "no_test":
                    m0 = mm.cpu().numpy().view(capi.DMATCH_DTYPE).reshape(NF, K)[:n, 0].copy()
            c.set_ratio_test(0.0)
            set_other(c, 0.0)
            # the nearest match of a query is true when its model point, under the frame's pose, lands on the keypoint
            R, t = b["poses"][f]
            rows = off64[np.clip(m0["imgIdx"], 0, len(off) - 2)] + m0["trainIdx"]
            cam = pts[np.clip(rows, 0, len(pts) - 1)] @ R.T + t
            uv = (cam @ scenes.K.T)[:, :2] / cam[:, 2:3]
            true = alive["no_test"] & (m0["imgIdx"] == b["objects"][f]) & (np.abs(uv - kp[:n].cpu().numpy()).max(axis=1) <= 3.0)
            for name in tally:
                tally[name]["true"] += int((alive[name] & true).sum())
                tally[name]["clutter"] += int((alive[name] & alive["no_test"] & ~true).sum())
    c.close()
    base = tally["no_test"]
    return {"what": "rendered-view DB of tod_amd/scenes.py: %d objects x 4 training views (%d rows), 32 detection frames of %d keypoints, "
                    "~30 %% object and ~70 %% clutter; k = %d, radius %d; nearest matches, true = names the visible object and its model "
                    "point projects within 3 px of the keypoint under the true pose" % (args.objects, len(desc), NF, K, RADIUS),
            "ratio": args.ratio, "nearest_matches": tally,
            "share_of_true_kept": {n: tally[n]["true"] / max(base["true"], 1) for n in ("classic", "other_object")},
            "share_of_clutter_kept": {n: tally[n]["clutter"] / max(base["clutter"], 1) for n in ("classic", "other_object")}}


def kernel_stats(path):
    import csv
    rows = [r for r in csv.DictReader(open(path)) if "other_object_min_mfma" in r.get("Name", "")]
    return [{"kernel": r["Name"].split("(")[0], "calls": int(r["Calls"]), "average_ms": float(r["AverageNs"]) / 1e6,
             "min_ms": float(r["MinNs"]) / 1e6, "max_ms": float(r["MaxNs"]) / 1e6} for r in rows] or NOT


out = {"library_has_the_setter": HAVE,
       "cost": NOT if args.skip_cost else cost(),
       "effect": NOT if args.skip_effect or not HAVE else effect(),
       "other_object_kernel_rocprofv3": kernel_stats(args.kernel_stats) if args.kernel_stats else NOT,
       "parent_commit_same_call": json.load(open(args.parent)).get("cost", NOT) if args.parent else NOT}
if args.parent and out["cost"] != NOT and out["parent_commit_same_call"] != NOT:
    a, b = out["cost"]["call_ms_off"], out["parent_commit_same_call"]["call_ms_off"]
    out["off_versus_parent"] = {"this_ms": a["median_of_turn_medians"], "parent_ms": b["median_of_turn_medians"],
                                "difference_ms": a["median_of_turn_medians"] - b["median_of_turn_medians"],
                                "turn_median_spread_ms": {"this": a["turn_median_spread"], "parent": b["turn_median_spread"]}}
print(json.dumps(out))
if args.out:
    json.dump(out, open(args.out, "w"), indent=1)
