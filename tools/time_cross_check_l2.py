"""Times todhip_cross_check_l2_device (tod_amd/csrc/cross_check_l2.hip) and the float ratio test on the C4 shape -- synth.make_sift_db,
500k rows; 1000 queries per frame, k = 2 -- once for a single frame and once for 16 frames per call. A frame's queries are about 400
distinct DB rows plus noise (several queries per row), so that lists are full and rows are contested. Modelled on
tools/time_cross_check.py. Per shape:
  * the filter alone between two events on the context's stream, each launch on a fresh unfiltered output;
  * the whole todhip_match_l2_device call with todhip_set_l2_cross_check off and on, the two settings alternating in one process,
    warm-up and three turns, every turn reported. The yardstick is the call with the setting OFF (code this filter does not touch),
    never the filter's own earlier run;
  * the same alternation for todhip_set_l2_ratio_test off / 0.8 (it adds no launch);
  * the achieved share of the vector roof: kept matches x valid queries x 384 lane-operations over SURVEY 8(d)'s 78.6 T lane-op/s. The
    early exit skips work, so this is the rate at which the DEFINITION's pairs are disposed of, not the kernel's share of peak.
Prints one JSON object and writes it to --out.

    timeout 900 python tools/time_cross_check_l2.py --out profiles/cross_check_l2.json"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from tod_amd import capi, synth

ap = argparse.ArgumentParser()
ap.add_argument("--objects", type=int, default=100, help="of 5000 rows each")
ap.add_argument("--queries", type=int, default=1000, help="per frame")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--launches", type=int, default=20, help="timed launches per turn")
ap.add_argument("--turns", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
K, RADIUS, DISTINCT, NOISE, ROOF = 2, 1.0e9, 400, 6.0, 78.6e12
rng = np.random.default_rng(4)

desc, pts, off = synth.make_sift_db(args.objects, per_object=5000)
Q = args.queries
c = capi.Context(0)
c.db_load(desc, pts, off)
st = torch.cuda.ExternalStream(c.stream)


def timed(fn, launches):
    """ms per launch of `launches` back-to-back calls between two events"""
    with torch.cuda.stream(st):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
    return e0.elapsed_time(e1) / launches


def shape(F):
    nq = F * Q
    pick = np.concatenate([rng.choice(rng.choice(len(desc), DISTINCT, replace=False), Q) for _ in range(F)])
    q = (desc[pick] + rng.normal(0, NOISE, (nq, 128))).astype(np.float32)
    d_q = torch.from_numpy(q).cuda()
    cnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
    mm = torch.zeros((nq * K, 4), dtype=torch.int32, device="cuda")
    xx = torch.zeros((nq * K, 3), device="cuda")
    torch.cuda.synchronize()
    ptrs = (cnt.data_ptr(), mm.data_ptr(), xx.data_ptr())

    def match():
        c.match_l2_device(d_q.data_ptr(), nq, K, RADIUS, *ptrs)

    def cross():
        c.cross_check_l2_device(d_q.data_ptr(), nq, Q, K, *ptrs)

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

    filter_ms, off_ms, on_ms, r_off_ms, r_on_ms = [], [], [], [], []
    for turn in range(args.turns):
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
        filter_ms.append(t / args.launches)
        for setting, sink in ((0, off_ms), (Q, on_ms)):
            c.set_l2_cross_check(setting)
            sink.append(timed(match, args.launches))
        c.set_l2_cross_check(0)
        for setting, sink in ((0.0, r_off_ms), (0.8, r_on_ms)):
            c.set_l2_ratio_test(setting)
            sink.append(timed(match, args.launches))
        c.set_l2_ratio_test(0.0)
    pairs = kept_before * Q
    f_ms, call_ms = float(np.mean(filter_ms)), float(np.mean(off_ms))
    return {"frames": F, "queries_per_frame": Q, "k": K, "matches_before": kept_before, "matches_after": kept_after,
            "share_kept": kept_after / max(kept_before, 1), "pairs_by_definition": pairs,
            "filter_ms": f_ms, "filter_ms_turns": filter_ms,
            "match_l2_device_call_ms": {"cross_check_off": call_ms, "cross_check_on": float(np.mean(on_ms)), "off_turns": off_ms, "on_turns": on_ms},
            "filter_over_call_with_setting_off": f_ms / call_ms,
            "definition_pairs_share_of_vector_roof": pairs * 384 / (f_ms * 1e-3) / ROOF,
            "ratio_test_call_ms": {"off": float(np.mean(r_off_ms)), "on_0.8": float(np.mean(r_on_ms)), "off_turns": r_off_ms, "on_turns": r_on_ms}}


out = {"what": "todhip_cross_check_l2_device and todhip_set_l2_ratio_test on the C4 shape: %d rows (synth.make_sift_db), %d queries per "
               "frame = %d distinct rows + N(0, %g) noise, k = %d" % (len(desc), Q, DISTINCT, NOISE, K),
       "roof_lane_ops_per_s": ROOF, "roof_source": "SURVEY 8(d)",
       "note": "definition_pairs_share_of_vector_roof counts the pairs the definition names, 384 lane-operations each; the kernel's early "
               "exit skips part of them, so it is not the kernel's share of peak",
       "shapes": [shape(1), shape(16)]}
c.close()
print(json.dumps(out))
if args.out:
    json.dump(out, open(args.out, "w"), indent=1)
