"""Times todhip_cross_check_device (tod_amd/csrc/cross_check.hip) on the C3 step -- 32 frames x 1000 queries, k = 5, radius 35, 1M rows
-- between two events on the context's stream, beside the DB pass's kernel time of the same run (todhip_set_kernel_timing), and the
whole todhip_match_device call with todhip_set_cross_check off and on, alternating turns. Independent-bit descriptors put no row inside
radius 35 of a random query, so the filter would have nothing to test: the DB here is 200 000 base rows in 5 variants each (0-8 flipped
bits) and every query is a DB row with 0-20 flipped bits, 400 distinct base rows per frame, so that lists are full and several
keypoints of a frame claim the same rows. Prints one JSON object and writes it to --out.

The data-chained measurements DESIGN 6m asks for (share of matches kept, objects per frame that reach RANSAC, the verifier's stage
time, frames/s and poses recovered with the filter off and on) are NOT taken by this script; the JSON says so.

    timeout 600 python tools/time_cross_check.py --out profiles/cross_check.json"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from tod_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--bases", type=int, default=200000)
ap.add_argument("--frames", type=int, default=32)
ap.add_argument("--queries", type=int, default=1000, help="per frame")
ap.add_argument("--radius", type=int, default=35)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--launches", type=int, default=20, help="timed launches per turn")
ap.add_argument("--turns", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
K, VARIANTS = 5, 5
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
c.set_matcher_engine("mfma")
c.db_load(desc, pts, off)
d_q = torch.from_numpy(q).cuda()
cnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
mm = torch.zeros((nq * K, 4), dtype=torch.int32, device="cuda")
xx = torch.zeros((nq * K, 3), device="cuda")
torch.cuda.synchronize()
out_ptrs = (cnt.data_ptr(), mm.data_ptr(), xx.data_ptr())
st = torch.cuda.ExternalStream(c.stream)


def match():
    c.match_device(d_q.data_ptr(), nq, K, args.radius, *out_ptrs)


def cross():
    c.cross_check_device(d_q.data_ptr(), nq, Q, K, *out_ptrs)


for _ in range(args.warmup):
    match()
    cross()
c.synchronize()
match()
c.synchronize()
kept_before = int(cnt.sum())
cross()
c.synchronize()
kept_after = int(cnt.sum())

filter_ms, pass_ms, call_off_ms, call_on_ms = [], [], [], []
for turn in range(args.turns):
    # the filter alone between two events (each launch on a fresh unfiltered output), the DB pass's kernel time from the same launches
    c0 = c.counters()
    c.set_kernel_timing(True)
    t = 0.0
    with torch.cuda.stream(st):
        for _ in range(args.launches):
            match()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            cross()
            e1.record()
            e1.synchronize()
            t += e0.elapsed_time(e1)
    c.synchronize()
    c.set_kernel_timing(False)
    c1 = c.counters()
    filter_ms.append(t / args.launches)
    pass_ms.append((c1.sum_match_kernel_ms - c0.sum_match_kernel_ms) / (c1.n_match_kernel_launches - c0.n_match_kernel_launches))
    for setting, sink in ((0, call_off_ms), (Q, call_on_ms)):             # the whole call, option off and on
        c.set_cross_check(setting)
        with torch.cuda.stream(st):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                match()
            e1.record()
            e1.synchronize()
            sink.append(e0.elapsed_time(e1) / args.launches)
    c.set_cross_check(0)
c.close()

NOT = "not measured"
out = {"what": "todhip_cross_check_device on the C3 step: %d frames x %d queries, k = %d, radius %d, %d rows (%d base rows x %d variants, "
               "queries = rows with 0-20 flipped bits, 400 base rows per frame)" % (F, Q, K, args.radius, rows, args.bases, VARIANTS),
       "matches_before": kept_before, "matches_after": kept_after, "share_kept": kept_after / max(kept_before, 1),
       "pairs_tested_upper_bound": kept_before * Q,
       "filter_ms": float(np.mean(filter_ms)), "filter_ms_turns": filter_ms,
       "db_pass_kernel_ms": float(np.mean(pass_ms)), "db_pass_kernel_ms_turns": pass_ms,
       "filter_over_db_pass": float(np.mean(filter_ms) / np.mean(pass_ms)),
       "match_device_call_ms": {"cross_check_off": float(np.mean(call_off_ms)), "cross_check_on": float(np.mean(call_on_ms)),
                                "off_turns": call_off_ms, "on_turns": call_on_ms},
       "data_chained_workload": {"share_of_matches_kept": NOT, "objects_per_frame_reaching_ransac": NOT, "stage_ms_per_step_verify": NOT,
                                 "frames_per_s": NOT, "poses_recovered": NOT,
                                 "why": "this script does not drive the chained workload; no effect on the verifier is claimed"}}
print(json.dumps(out))
if args.out:
    json.dump(out, open(args.out, "w"), indent=1)
