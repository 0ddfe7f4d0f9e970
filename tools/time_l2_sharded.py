"""Times the float searches over a sharded DB (todhip_match_l2_shard_device + todhip_merge_l2_shards_device and the radius pair,
DESIGN 6n) on one device that rehearses one rank of a world of 8 at BASELINE configs[3]'s shape: synth.make_sift_db's 500 000 rows in
200 objects, so that shard 0 of 8 is 62 500 rows, and 8 x 1000 gathered queries (synth.make_sift_queries, 30 % planted neighbours).
HIP events around `--launches` calls, alternating turns.

  (a) the shard call (k = 2) against todhip_match_l2_device on an unsharded context loaded with the same 62 500 rows, same 8000
      queries: the whole call, and the DB pass alone from todhip_set_kernel_timing. The DB pass is the same kernels; the whole call
      differs by SK against l2_finalize_kernel. The same for the radius pair (radius 200, 64 per query), SR against LE.
  (b) the merges of the 8 shards' key sets for 1000 and for 32 000 queries, k = 2 and 5 and the radius form at 64 per query, against
      todhip_merge_shards_device / todhip_merge_radius_shards_device on Hamming keys of the same shape (a 500 000-row binary DB in 8
      shards, synth.make_frame queries, radius 35).
Prints one JSON object and writes it to --out.

    timeout 900 python tools/time_l2_sharded.py --out profiles/l2_sharded.json"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from tod_amd import capi, synth

ap = argparse.ArgumentParser()
ap.add_argument("--world", type=int, default=8)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--launches", type=int, default=20, help="timed launches per turn")
ap.add_argument("--turns", type=int, default=3)
ap.add_argument("--merge-queries", type=int, nargs="+", default=[1000, 32000])
ap.add_argument("--out", default=None)
args = ap.parse_args()
WORLD, K, MPQ, RADIUS, R_RADIUS, H_RADIUS = args.world, 2, 64, 400.0, 200.0, 35
NQ = WORLD * 1000
NQ_MAX = max(args.merge_queries + [NQ])
assert NQ_MAX % 1000 == 0


def timed(stream, call):
    """ms per call over --launches calls between two events on `stream`"""
    with torch.cuda.stream(stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            call()
        e1.record()
        e1.synchronize()
    return e0.elapsed_time(e1) / args.launches


def turns(streams, calls):
    """{name: [ms per turn]}, the calls alternating; streams: {name: the stream its call runs on}"""
    for call in calls.values():
        for _ in range(args.warmup):
            call()
    torch.cuda.synchronize()
    ms = {name: [] for name in calls}
    for _ in range(args.turns):
        for name, call in calls.items():
            ms[name].append(timed(streams[name], call))
    return ms


def db_pass(ctxs, calls):
    """{name: [ms per turn]} of the bracketed DB pass alone, from the context's kernel timing"""
    ms = {name: [] for name in calls}
    for _ in range(args.turns):
        for name, call in calls.items():
            c = ctxs[name]
            k0 = c.counters()
            c.set_kernel_timing(True)
            for _ in range(args.launches):
                call()
            c.synchronize()
            c.set_kernel_timing(False)
            k1 = c.counters()
            ms[name].append((k1.sum_match_kernel_ms - k0.sum_match_kernel_ms) / (k1.n_match_kernel_launches - k0.n_match_kernel_launches))
    return ms


def say(what):
    print(what, file=sys.stderr, flush=True)


def stats(v):
    return {"ms": float(np.mean(v)), "ms_turns": v, "spread": float((max(v) - min(v)) / np.mean(v))}


def pair(ms, a, b):
    return {a: stats(ms[a]), b: stats(ms[b]), "ratio": float(np.mean(ms[a]) / np.mean(ms[b]))}


desc, pts, off = synth.make_sift_db(200, per_object=2500)
q = np.concatenate([synth.make_sift_queries(desc, 1000, frame=f)[0] for f in range(NQ_MAX // 1000)])
d_q = torch.from_numpy(q).cuda()
shards = []
for r in range(WORLD):
    c = capi.Context(0)
    c.db_load(desc, pts, off, shard_rank=r, shard_count=WORLD)
    shards.append(c)
c0 = shards[0]
info = c0.db_info()
one = capi.Context(0)                                       # unsharded, the same rows as shard 0
lo, hi = int(info["shard_first"]), int(info["shard_first"] + info["shard_rows"])
n_obj0 = int(np.searchsorted(off, hi))
one.db_load(desc[lo:hi], pts[lo:hi], off[:n_obj0 + 1])
assert one.db_info()["total_rows"] == info["shard_rows"]
say("float DB and queries are resident: shard 0 holds %d rows" % info["shard_rows"])
st = {"shard": torch.cuda.ExternalStream(c0.stream), "device": torch.cuda.ExternalStream(one.stream)}
ctx_of = {"shard": c0, "device": one}

# ---- (a) a rank's call against the unsharded call on the same rows
keys = torch.zeros((NQ, MPQ + 1), dtype=torch.int64, device="cuda")
cnt = torch.zeros(NQ_MAX, dtype=torch.int32, device="cuda")
inr = torch.zeros(NQ_MAX, dtype=torch.int32, device="cuda")
mm = torch.zeros((NQ_MAX * MPQ, 4), dtype=torch.int32, device="cuda")
xx = torch.zeros((NQ_MAX * MPQ, 3), device="cuda")
torch.cuda.synchronize()
knn = {"shard": lambda: c0.match_l2_shard_device(d_q.data_ptr(), NQ, K, keys.data_ptr()),
       "device": lambda: one.match_l2_device(d_q.data_ptr(), NQ, K, RADIUS, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr())}
rad = {"shard": lambda: c0.match_l2_radius_shard_device(d_q.data_ptr(), NQ, R_RADIUS, MPQ, keys.data_ptr()),
       "device": lambda: one.match_l2_radius_device(d_q.data_ptr(), NQ, R_RADIUS, MPQ, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr(), inr.data_ptr())}
a = {"what": "shard 0 of %d: %d rows of %d, %d queries; against an unsharded context with the same rows" % (WORLD, info["shard_rows"], len(desc), NQ)}
for name, calls, what in (("knn_k2", knn, "k = 2, radius %g" % RADIUS), ("radius_64", rad, "radius %g, max_per_query %d" % (R_RADIUS, MPQ))):
    whole, passes = turns(st, calls), db_pass(ctx_of, calls)
    a[name] = {"what": what, "whole_call": pair(whole, "shard", "device"), "db_pass": pair(passes, "shard", "device")}
    say("(a) %s done" % name)
one.synchronize()
n_in = inr[:NQ].cpu().numpy().astype(np.int64)
a["radius_64"]["in_radius"] = {"mean": float(n_in.mean()), "max": int(n_in.max()), "queries_with_hits": int((n_in > 0).sum())}
a["one_call_of_1000_queries_for_scale"] = stats(turns(st, {"shard": lambda: c0.match_l2_shard_device(d_q.data_ptr(), 1000, K, keys.data_ptr())})["shard"])

# ---- (b) the merges, against the Hamming merges on keys of the same shape
bdesc, bpts, boff = synth.make_db(100)
bq = np.concatenate([synth.make_frame(bdesc, bpts, boff, 1000, frame=f, visible_object=(17 * f + 3) % 100, H=48, W=64)["q_desc"]
                     for f in range(NQ_MAX // 1000)])
d_bq = torch.from_numpy(bq).cuda()
bshards = []
for r in range(WORLD):
    c = capi.Context(0)
    c.db_load(bdesc, bpts, boff, shard_rank=r, shard_count=WORLD)
    bshards.append(c)
b0 = bshards[0]
stm = {"l2": st["shard"], "hamming": torch.cuda.ExternalStream(b0.stream)}
say("binary DB is resident")
b = {}
for nq in args.merge_queries:
    for form, width in (("knn_k2", 2), ("knn_k5", 5), ("radius_64", MPQ + 1)):
        fk = torch.zeros((WORLD, nq, width), dtype=torch.int64, device="cuda")
        hk = torch.zeros((WORLD, nq, width), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        for r in range(WORLD):
            if form == "radius_64":
                shards[r].match_l2_radius_shard_device(d_q.data_ptr(), nq, R_RADIUS, MPQ, fk[r].data_ptr())
                bshards[r].match_radius_shard_device(d_bq.data_ptr(), nq, H_RADIUS, MPQ, hk[r].data_ptr())
            else:
                shards[r].match_l2_shard_device(d_q.data_ptr(), nq, width, fk[r].data_ptr())
                bshards[r].match_shard_device(d_bq.data_ptr(), nq, width, H_RADIUS, hk[r].data_ptr())
            shards[r].synchronize()
            bshards[r].synchronize()
        if form == "radius_64":
            calls = {"l2": lambda: c0.merge_l2_radius_shards_device(fk.data_ptr(), WORLD, nq, MPQ, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr(), inr.data_ptr()),
                     "hamming": lambda: b0.merge_radius_shards_device(hk.data_ptr(), WORLD, nq, MPQ, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr(), inr.data_ptr())}
        else:
            calls = {"l2": lambda: c0.merge_l2_shards_device(fk.data_ptr(), WORLD, nq, width, RADIUS, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr()),
                     "hamming": lambda: b0.merge_shards_device(hk.data_ptr(), WORLD, nq, width, H_RADIUS, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr())}
        ms = turns(stm, calls)
        torch.cuda.synchronize()
        b["%s_x%d" % (form, nq)] = dict(pair(ms, "l2", "hamming"), what="%d key sets x %d queries x %d keys" % (WORLD, nq, width),
                                        exchange_bytes_per_rank_and_step=WORLD * nq * width * 8)
        say("(b) %s x %d done" % (form, nq))
for c in shards + bshards + [one]:
    c.close()
out = {"measured": True, "device": torch.cuda.get_device_name(0), "launches_per_turn": args.launches, "a_rank_call": a, "b_merge": b,
       "not_measured": "a multi-GPU node: the exchange itself and the 1 -> 8 scaling; real SIFT descriptors"}
print(json.dumps(out))
if args.out:
    json.dump(out, open(args.out, "w"), indent=1)
