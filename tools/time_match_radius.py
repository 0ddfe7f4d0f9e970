"""Times the DB pass of todhip_match_radius_device (radius_collect_mfma, tod_amd/csrc/match_radius.hip) with the context's kernel timing
at a chosen shape, against the yardstick of DESIGN 6g in the same process: todhip_match_device at k = 5 with whole blocks
(todhip_set_matcher_block_split 0) on the same rows and queries, alternating turns. Independent-bit rows and queries by default;
--dense adds the `chained` block's trained DB (scenes.train_db: this library's ORB descriptors of rendered views, the DB
tests/golden/chained_frames.npz was matched against) with the ORB descriptors of rendered detection views as queries, where hundreds of
rows lie inside the radius of a query and the pass's atomics and the ordered rescan do real work. Also event-times the whole call.
Prints one JSON object and writes it to --out.

    timeout 600 python tools/time_match_radius.py --out profiles/match_radius.json
    timeout 900 python tools/time_match_radius.py --dense --out profiles/match_radius.json"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from tod_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1000000)
ap.add_argument("--queries", type=int, default=32000)
ap.add_argument("--radius", type=int, default=35)
ap.add_argument("--max-per-query", type=int, default=64)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--launches", type=int, default=20, help="timed launches per turn")
ap.add_argument("--turns", type=int, default=3)
ap.add_argument("--dense", action="store_true", help="also the chained block's trained DB (takes a few minutes to train)")
ap.add_argument("--dense-objects", type=int, default=200)
ap.add_argument("--out", default=None)
args = ap.parse_args()
K = 5


def measure(desc, pts, off, d_q, nq, what):
    """{radius pass, yardstick, ratio, whole call, how many queries overflowed} on one DB and one device-resident query set"""
    mpq, radius = args.max_per_query, args.radius
    c = capi.Context(0)
    c.set_matcher_engine("mfma")
    c.set_matcher_block_split(0)
    c.db_load(desc, pts, off)
    cnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
    inr = torch.zeros(nq, dtype=torch.int32, device="cuda")
    mm = torch.zeros((nq * mpq, 4), dtype=torch.int32, device="cuda")
    xx = torch.zeros((nq * mpq, 3), device="cuda")
    torch.cuda.synchronize()
    calls = {"radius": lambda: c.match_radius_device(d_q.data_ptr(), nq, radius, mpq, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr(), inr.data_ptr()),
             "knn": lambda: c.match_device(d_q.data_ptr(), nq, K, radius, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr())}
    ms = {name: [] for name in calls}
    for name, call in calls.items():
        for _ in range(args.warmup):
            call()
        c.synchronize()
    for turn in range(args.turns):
        for name, call in calls.items():
            c0 = c.counters()
            c.set_kernel_timing(True)
            for _ in range(args.launches):
                call()
            c.synchronize()
            c.set_kernel_timing(False)
            c1 = c.counters()
            ms[name].append((c1.sum_match_kernel_ms - c0.sum_match_kernel_ms) / (c1.n_match_kernel_launches - c0.n_match_kernel_launches))
    st = torch.cuda.ExternalStream(c.stream)
    whole = {}
    with torch.cuda.stream(st):
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                call()
            e1.record()
            e1.synchronize()
            whole[name] = e0.elapsed_time(e1) / args.launches
    calls["radius"]()
    c.synchronize()
    n_in = inr.cpu().numpy().astype(np.int64)
    c.close()
    r, k = float(np.mean(ms["radius"])), float(np.mean(ms["knn"]))
    return {"what": what, "rows": int(off[-1]), "queries": nq, "radius": radius, "max_per_query": mpq, "buffer_keys": capi.radius_capacity(mpq),
            "collect_pass_ms": r, "collect_pass_ms_turns": ms["radius"],
            "yardstick": "todhip_match_device k = 5, matrix-core engine, whole blocks (block split 0), DB-pass kernel",
            "yardstick_ms": k, "yardstick_ms_turns": ms["knn"], "ratio": r / k,
            "whole_call_ms": {"match_radius_device": whole["radius"], "match_device_k5": whole["knn"]},
            "in_radius": {"mean": float(n_in.mean()), "median": float(np.median(n_in)), "max": int(n_in.max()),
                          "queries_beyond_the_buffer": int((n_in > capi.radius_capacity(mpq)).sum())}}


out = {}
rng = np.random.default_rng(1)
desc = rng.integers(0, 256, (args.rows, 32), dtype=np.uint8)
pts = rng.standard_normal((args.rows, 3)).astype(np.float32)
off = np.linspace(0, args.rows, 201).astype(np.uint32)
d_q = torch.from_numpy(rng.integers(0, 256, (args.queries, 32), dtype=np.uint8)).cuda()
out["independent_bits"] = measure(desc, pts, off, d_q, args.queries, "independent-bit rows and queries")
if args.dense:
    from tod_amd import scenes
    NQ, FRAMES = 1000, 32
    tex = scenes.make_textures(args.dense_objects)
    tctx = capi.Context(0)
    desc, pts, off = scenes.train_db(tctx, tex, rows_per_object=5000)
    bts = scenes.make_detection_batches(tex, FRAMES // 16, 16)
    d_q = torch.zeros((FRAMES, NQ, 32), dtype=torch.uint8, device="cuda")
    kp = torch.zeros((16, NQ, 2), device="cuda")
    aux = torch.zeros((16, NQ, 4), device="cuda")
    for b, bt in enumerate(bts):
        tctx.orb_batch_device(bt["images"].data_ptr(), 16, scenes.H * scenes.W, scenes.H, scenes.W, scenes.W, NQ, 3, 1.2, kp.data_ptr(),
                              aux.data_ptr(), d_q[16 * b:].data_ptr(), NQ)
    tctx.synchronize()
    tctx.close()
    out["chained_db"] = measure(desc, pts, off, d_q, FRAMES * NQ, "the chained block's trained DB, ORB descriptors of 32 rendered views as queries")
print(json.dumps(out))
if args.out:
    json.dump(out, open(args.out, "w"), indent=1)
