"""What todhip_model_compact costs and what it changes. Writes profiles/model_compact.json.

  python tools/time_model_compact.py [--out profiles/model_compact.json]

Two parts, every step a process of its own under its own time limit, run one after the other; the first step that fails ends the run
(nothing further is started on the device) and the JSON says which:
  synthetic   the wall time of one compact call (time.perf_counter around it; the call synchronizes) on seeded models of 4096, 32 768
              and 2^18 rows at about 10 % and about 90 % kept: the median of REPEATS calls after one warm-up, each on a freshly
              loaded model. A dropped row is an exact copy of an earlier row -- the cost depends on the row count and on the size of
              the kept front, not on how near a near-duplicate is -- merge_dist 0.001, max_hamming 10.
  workload    scenes.train_db's rendered-view models with and without compact=(0.003, 24): rows per object, the DB-pass kernel time
              (todhip_set_kernel_timing) of the same detection frames' queries against both DBs, and the share of frames whose
              rendering pose is recovered (tests/test_end_to_end_gpu.py's tolerances) against each.
The only comparison is the uncompacted DB of the same commit."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

REPEATS = 5
SYNTH = [(4096, 0.1), (4096, 0.9), (32768, 0.1), (32768, 0.9), (1 << 18, 0.1), (1 << 18, 0.9)]
SYNTH_MERGE = (0.001, 10)
WORK_OBJECTS, WORK_BATCHES, WORK_FRAMES, WORK_MERGE = 16, 2, 8, (0.003, 24)
LIMIT_S = {"synthetic": 240, "workload": 420}


def synthetic_model(n, kept_share, seed):
    """n rows of which about kept_share * n are distinct (random descriptors, random points of the unit cube); the others repeat one"""
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(seed))
    n_base = max(int(n * kept_share), 1)
    base_d = rng.integers(0, 256, (n_base, 32), dtype=np.uint8)
    base_p = rng.random((n_base, 3)).astype(np.float32)
    which = np.concatenate([np.arange(n_base), rng.integers(0, n_base, n - n_base)])
    which = which[rng.permutation(n)]
    return base_d[which], base_p[which]


def step_synthetic(n, share):
    import numpy as np
    from tod_amd import capi
    desc, pts = synthetic_model(n, share, 1000 + n)
    ctx = capi.Context(0)
    times, rows = [], None
    for r in range(REPEATS + 1):                                           # the first call is the warm-up
        model = capi.Model(ctx, n)
        model.add_rows(desc, pts)
        ctx.synchronize()
        t0 = time.perf_counter()
        rows = model.compact(*SYNTH_MERGE)
        times.append((time.perf_counter() - t0) * 1e3)
        model.close()
    ctx.close()
    t = times[1:]
    return dict(rows=n, rows_after=rows[1], kept_share=rows[1] / n, compact_ms=dict(median=float(np.median(t)), min=min(t), max=max(t)),
                launches=2 * ((n + 63) // 64) - 1)


def step_workload():
    import numpy as np
    from tod_amd import capi, scenes
    F, Z, H, W, K = scenes.F, scenes.Z, scenes.H, scenes.W, scenes.K
    textures = scenes.make_textures(WORK_OBJECTS)
    ctx = capi.Context(0)
    dbs = {"uncompacted": scenes.train_db(ctx, textures), "compacted": scenes.train_db(ctx, textures, compact=WORK_MERGE)}
    batches = scenes.make_detection_batches(textures, WORK_BATCHES, WORK_FRAMES)
    v, u = np.mgrid[0:H, 0:W].astype(np.float32)
    cloud = np.stack([(u - K[0, 2]) * Z / F, (v - K[1, 2]) * Z / F, np.full((H, W), Z, np.float32)], axis=2).astype(np.float32)
    frames = []
    for b in batches:
        imgs = b["images"].cpu().numpy()
        for f in range(len(imgs)):
            kp, aux, q = ctx.orb(imgs[f], 1000, 3, 1.2)
            frames.append((kp, q, b["objects"][f], b["poses"][f]))
    out = {}
    ctx.set_kernel_timing(True)
    for name, (desc, pts, off) in dbs.items():
        spans = ctx.db_load(desc, pts, off)
        for kp, q, obj, pose in frames[:2]:
            ctx.match(q, 5, 55)                                            # warm-up
        ctx.synchronize()
        found, kern = 0, []
        for kp, q, obj, (R_true, t_true) in frames:
            c0 = ctx.counters().sum_match_kernel_ms
            row_ptr, m, xyz = ctx.match(q, 5, 55)
            ctx.synchronize()
            kern.append(ctx.counters().sum_match_kernel_ms - c0)
            poses = ctx.verify(kp, cloud, row_ptr, m, xyz, spans, 8, 2500, 0.01, capi.rng_new(1))
            found += any(p["object"] == obj and np.abs(p["R"] - R_true).max() < 0.02 and np.abs(p["t"] - t_true).max() < 0.004
                         for p in poses)
        out[name] = dict(rows_per_object=np.diff(off.astype(np.int64)).tolist(), db_rows=int(off[-1]), frames=len(frames),
                         db_pass_kernel_ms_per_frame=dict(median=float(np.median(kern)), min=float(min(kern)), max=float(max(kern))),
                         frames_with_the_rendering_pose=found, share_recovered=found / len(frames))
    ctx.close()
    return dict(objects=WORK_OBJECTS, train_views=len(scenes.TRAIN_VIEWS), compact=list(WORK_MERGE), k=5, radius=55, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "model_compact.json"))
    ap.add_argument("--step", help="internal: synthetic:<rows>:<kept share> or workload; prints one JSON line")
    a = ap.parse_args()
    if a.step:
        part = a.step.split(":")
        res = step_workload() if part[0] == "workload" else step_synthetic(int(part[1]), float(part[2]))
        print("RESULT " + json.dumps(res))
        return 0
    steps = ["synthetic:%d:%g" % s for s in SYNTH] + ["workload"]
    res = dict(measured=True, method=dict(repeats=REPEATS, warmup=1, merge_synthetic=list(SYNTH_MERGE),
                                          timing="time.perf_counter around todhip_model_compact (it synchronizes); "
                                                 "todhip_set_kernel_timing for the DB pass"), synthetic=[], workload=None)
    for s in steps:                                                        # chained: a failing step ends the run
        limit = LIMIT_S[s.split(":")[0]]
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", s],
                           stdout=subprocess.PIPE, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            res["stopped_at"] = dict(step=s, exit_status=p.returncode)
            break
        part = json.loads(line[-1][7:])
        print(s, part)
        if s == "workload":
            res["workload"] = part
        else:
            res["synthetic"].append(part)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 1 if "stopped_at" in res else 0


if __name__ == "__main__":
    sys.exit(main())
