"""Times todhip_match_l2_device over a float DB of 64 x f32 rows (desc_bytes 256) against the yardstick of the same run:
the same call at the same shape over 128 x f32 rows. One process, two contexts, alternating turns. Per turn and contender: the
HIP-event time of the pass over the DB (todhip_set_kernel_timing: l2_gemm_kernel<2, 4, D> on the one-GEMM path) and the host clock
around `--launches` calls that end in a synchronise.

Shape: BASELINE configs[3]'s, 1000 queries x 500 000 rows of synth.make_sift_db at k = 2, once with dim=64 and once with dim=128.
Acceptance: the 64-wide pass's mean over the turns may not exceed the 128-wide pass's by more than the spread (max - min) of the
yardstick's own turns. Prints one JSON object and writes it to --out.

    timeout 600 python tools/time_l2_dim64.py --out profiles/l2_dim64.json"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from tod_amd import capi, synth

ap = argparse.ArgumentParser()
ap.add_argument("--objects", type=int, default=100, help="objects of 5000 rows")
ap.add_argument("--queries", type=int, default=1000)
ap.add_argument("--k", type=int, default=2)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--launches", type=int, default=20, help="timed calls per turn")
ap.add_argument("--turns", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()


def contender(dim):
    desc, pts, off = synth.make_sift_db(args.objects, dim=dim)
    q, truth = synth.make_sift_queries(desc, args.queries, frame=1)
    c = capi.Context(0)
    c.db_load(desc, pts, off)
    assert c.desc_bytes() == 4 * dim
    nq, k = len(q), args.k
    d_q = torch.from_numpy(q).cuda()
    cnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
    mm = torch.zeros((nq * k, 4), dtype=torch.int32, device="cuda")
    xx = torch.zeros((nq * k, 3), device="cuda")
    torch.cuda.synchronize()

    def call():
        c.match_l2_device(d_q.data_ptr(), nq, k, 1.0e9, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr())
    for _ in range(args.warmup):
        call()
    c.synchronize()
    # the planted row is the nearest: the timed call answers the question
    m = mm.cpu().numpy().reshape(nq, k, 4)
    glob = off[m[:, 0, 2]].astype(np.int64) + m[:, 0, 1]
    planted = truth >= 0
    assert (glob[planted] == truth[planted]).all()
    return dict(ctx=c, call=call, rows=int(off[-1]), keep=(d_q, cnt, mm, xx), pass_ms=[], host_ms=[])


cs = {"dim64": contender(64), "dim128": contender(128)}
for turn in range(args.turns):
    for name, s in cs.items():
        c = s["ctx"]
        c0 = c.counters()
        c.set_kernel_timing(True)
        t0 = time.perf_counter()
        for _ in range(args.launches):
            s["call"]()
        c.synchronize()
        s["host_ms"].append((time.perf_counter() - t0) * 1e3 / args.launches)
        c.set_kernel_timing(False)
        c1 = c.counters()
        s["pass_ms"].append((c1.sum_match_kernel_ms - c0.sum_match_kernel_ms) / (c1.n_match_kernel_launches - c0.n_match_kernel_launches))
y, n = cs["dim128"], cs["dim64"]
spread = max(y["pass_ms"]) - min(y["pass_ms"])
out = {"lib": os.path.relpath(capi.LIB_PATH, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")),
       "rows": n["rows"], "queries": args.queries, "k": args.k, "launches_per_turn": args.launches,
       "yardstick": "todhip_match_l2_device over 128 x f32 rows, same shape, same process, alternating turns",
       "dim64_pass_ms_turns": n["pass_ms"], "dim64_host_ms_per_call_turns": n["host_ms"],
       "dim128_pass_ms_turns": y["pass_ms"], "dim128_host_ms_per_call_turns": y["host_ms"],
       "dim64_pass_ms_mean": float(np.mean(n["pass_ms"])), "dim128_pass_ms_mean": float(np.mean(y["pass_ms"])),
       "pass_ratio_64_over_128": float(np.mean(n["pass_ms"]) / np.mean(y["pass_ms"])),
       "host_ratio_64_over_128": float(np.mean(n["host_ms"]) / np.mean(y["host_ms"])),
       "yardstick_spread_ms": spread,
       "acceptance": {"rule": "mean 64-wide pass <= mean 128-wide pass + spread of the 128-wide pass's turns",
                      "passes": bool(np.mean(n["pass_ms"]) <= np.mean(y["pass_ms"]) + spread)},
       "not_measured": ["16 frames per call", "the sharded exchange on several devices", "real SURF or KAZE data"]}
for s in cs.values():
    s["ctx"].close()
print(json.dumps(out))
if args.out:
    json.dump(out, open(args.out, "w"), indent=1)
