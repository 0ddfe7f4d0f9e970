"""Times todhip_match_l2_radius_device (tod_amd/csrc/l2_radius.h) against the yardstick of DESIGN 6l in the same process:
todhip_match_l2_device at k = 5 with the same radius on the same rows and queries, alternating turns. Per turn and call: the host
clock around `--launches` calls that end in a synchronise, and the HIP-event time of the pass over the DB (todhip_set_kernel_timing:
the one GEMM pass of the radius call, pass 2 of the k-NN call -- the same kernel; the k-NN call's seed GEMM is outside its bracket and
shows in the whole-call time only).

Three inputs at BASELINE configs[3]'s shape (1000 queries x 500k rows of synth's SIFT-like DB):
  sparse   the radius admits the planted row of a query and nothing else
  dense    100 planted clusters of 300 near copies: every query lies in one and has ~300 rows in range, none overflows
  scan     the same, and a tenth of the queries lie in one cluster of 3000 near copies: their candidate lists overflow and the
           ordered scan answers them (one read of the f32 DB per such query)
--knn-only times the yardstick on the sparse input alone; with TODHIP_LIB_PATH naming another build of the library this is the
A/B of the unchanged call against the parent commit, each build a process of its own. Prints one JSON object and writes it to --out.

    timeout 600 python tools/time_match_l2_radius.py --out profiles/match_l2_radius.json"""
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
ap.add_argument("--max-per-query", type=int, default=64)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--launches", type=int, default=20, help="timed calls per turn")
ap.add_argument("--turns", type=int, default=3)
ap.add_argument("--knn-only", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
K = 5


def measure(desc, pts, off, q, radius, what):
    nq, mpq = len(q), args.max_per_query
    c = capi.Context(0)
    c.db_load(desc, pts, off)
    d_q = torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda()
    cnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
    inr = torch.zeros(nq, dtype=torch.int32, device="cuda")
    mm = torch.zeros((nq * mpq, 4), dtype=torch.int32, device="cuda")
    xx = torch.zeros((nq * mpq, 3), device="cuda")
    torch.cuda.synchronize()
    calls = {"knn": lambda: c.match_l2_device(d_q.data_ptr(), nq, K, radius, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr())}
    if not args.knn_only:
        calls["radius"] = lambda: c.match_l2_radius_device(d_q.data_ptr(), nq, radius, mpq, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr(),
                                                           inr.data_ptr())
    for call in calls.values():
        for _ in range(args.warmup):
            call()
        c.synchronize()
    pass_ms, host_ms = {n: [] for n in calls}, {n: [] for n in calls}
    for turn in range(args.turns):
        for name, call in calls.items():
            c0 = c.counters()
            c.set_kernel_timing(True)
            t0 = time.perf_counter()
            for _ in range(args.launches):
                call()
            c.synchronize()
            host_ms[name].append((time.perf_counter() - t0) * 1e3 / args.launches)
            c.set_kernel_timing(False)
            c1 = c.counters()
            pass_ms[name].append((c1.sum_match_kernel_ms - c0.sum_match_kernel_ms) / (c1.n_match_kernel_launches - c0.n_match_kernel_launches))
    out = {"what": what, "rows": int(off[-1]), "queries": nq, "radius": radius,
           "yardstick": "todhip_match_l2_device k = 5, same radius",
           "yardstick_pass_ms_turns": pass_ms["knn"], "yardstick_host_ms_per_call_turns": host_ms["knn"]}
    if not args.knn_only:
        c.synchronize()
        n_in = inr.cpu().numpy().astype(np.int64)
        out.update({"max_per_query": mpq, "pass_ms_turns": pass_ms["radius"], "host_ms_per_call_turns": host_ms["radius"],
                    "in_radius": {"mean": float(n_in.mean()), "median": float(np.median(n_in)), "max": int(n_in.max()),
                                  "queries_with_more_than_2048": int((n_in > 2048).sum())}})
    c.close()
    return out


desc, pts, off = synth.make_sift_db(args.objects)
q, _ = synth.make_sift_queries(desc, args.queries, frame=1)
out = {"lib": capi.LIB_PATH, "launches_per_turn": args.launches,
       "sparse": measure(desc, pts, off, q, 200.0, "synth's SIFT-like DB and queries: planted rows at ~136, the others beyond 300")}
if not args.knn_only:
    s = out["sparse"]
    spread = max(s["yardstick_host_ms_per_call_turns"]) - min(s["yardstick_host_ms_per_call_turns"])
    s["acceptance"] = {"rule": "the radius call's slower turn <= the yardstick's slower turn + the spread of the yardstick's turns (host ms per call)",
                       "radius_slower_turn": max(s["host_ms_per_call_turns"]), "bound": max(s["yardstick_host_ms_per_call_turns"]) + spread,
                       "passes": bool(max(s["host_ms_per_call_turns"]) <= max(s["yardstick_host_ms_per_call_turns"]) + spread)}
    rng = np.random.default_rng(3)
    n = len(desc)
    where = rng.permutation(n)
    centres = desc[where[:101]].copy()                                   # the rows themselves stay in the DB
    dense = desc.copy()
    for j in range(100):
        dense[where[1000 + 300 * j:1300 + 300 * j]] = centres[j][None, :] + rng.normal(0, 1.0, (300, 128)).astype(np.float32)
    qd = (centres[np.arange(args.queries) % 100] + rng.normal(0, 1.0, (args.queries, 128))).astype(np.float32)
    out["dense"] = measure(dense, pts, off, qd, 40.0, "100 clusters of 300 near copies (sigma 1: ~16 apart); every query in one of them")
    dense[where[40000:43000]] = centres[100][None, :] + rng.normal(0, 1.0, (3000, 128)).astype(np.float32)
    qd[::10] = (centres[100][None, :] + rng.normal(0, 1.0, (len(qd[::10]), 128))).astype(np.float32)
    out["scan"] = measure(dense, pts, off, qd, 40.0, "the dense input, and every tenth query in a cluster of 3000 near copies: the ordered scan")
    n_scan = out["scan"]["in_radius"]["queries_with_more_than_2048"]
    # the flagged queries' scans run side by side, one workgroup each: the first figure is roughly ONE scan's duration
    added = float(np.mean(out["scan"]["host_ms_per_call_turns"]) - np.mean(out["dense"]["host_ms_per_call_turns"]))
    out["scan"]["ms_per_call_added_to_the_dense_input"] = added
    out["scan"]["added_ms_per_flagged_query"] = added / max(n_scan, 1)
    out["scan"]["f32_db_bytes_read_per_flagged_query"] = n * 512
print(json.dumps(out))
if args.out:
    json.dump(out, open(args.out, "w"), indent=1)
