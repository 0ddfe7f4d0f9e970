"""Times the radius search over a sharded DB (todhip_match_radius_shard_device + todhip_merge_radius_shards_device) on one
device that rehearses one rank of a world of 8: the synthetic 1M-row DB (synth.make_db(200)), 8 x 4000 queries from
synth.make_frame (30 % planted neighbours), radius 35, max_per_query 64. HIP events around `--launches` calls, alternating turns.

  (a) the shard call against todhip_match_radius_device on the same context (shard 0 of 8) and the same 32 000 queries: the DB pass
      and R2 are the same kernels, S1 stands where R3 stood, so the expected ratio is 1 within the spread of the turns.
  (b) the merge (M1) of the 8 shards' key sets for this rank's 4000 queries, against todhip_merge_shards_device at k = 8 on the same
      shards and queries, and against the collect pass of (a), beside which it runs on the comm stream.
Prints one JSON object and writes it to --out.

    timeout 600 python tools/time_match_radius_sharded.py --out profiles/match_radius_sharded.json"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from tod_amd import capi, synth

ap = argparse.ArgumentParser()
ap.add_argument("--objects", type=int, default=200, help="objects of 5000 rows")
ap.add_argument("--world", type=int, default=8)
ap.add_argument("--queries-per-rank", type=int, default=4000)
ap.add_argument("--radius", type=int, default=35)
ap.add_argument("--max-per-query", type=int, default=64)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--launches", type=int, default=20, help="timed launches per turn")
ap.add_argument("--turns", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
WORLD, NQ_RANK, RADIUS, MPQ, K = args.world, args.queries_per_rank, args.radius, args.max_per_query, 8
NQ = WORLD * NQ_RANK
assert NQ_RANK % 1000 == 0


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


def turns(stream, calls):
    """{name: [ms per turn]}, the calls alternating"""
    for call in calls.values():
        for _ in range(args.warmup):
            call()
    torch.cuda.synchronize()
    ms = {name: [] for name in calls}
    for _ in range(args.turns):
        for name, call in calls.items():
            ms[name].append(timed(stream, call))
    return ms


def say(what):
    print(what, file=sys.stderr, flush=True)


def stats(v):
    return {"ms": float(np.mean(v)), "ms_turns": v, "spread": float((max(v) - min(v)) / np.mean(v))}


desc, pts, off = synth.make_db(args.objects)
# frame f belongs to rank f // (frames per rank); the visible objects are spread over the DB, so every shard meets planted neighbours
n_frames = NQ // 1000
q = np.concatenate([synth.make_frame(desc, pts, off, 1000, frame=f, visible_object=(17 * f + 3) % args.objects, H=48, W=64)["q_desc"]
                    for f in range(n_frames)])
d_q = torch.from_numpy(q).cuda()
shards = []
for r in range(WORLD):
    c = capi.Context(0)
    c.set_matcher_engine("mfma")
    c.db_load(desc, pts, off, shard_rank=r, shard_count=WORLD)
    shards.append(c)
c0 = shards[0]
say("DB and queries are resident")
st0 = torch.cuda.ExternalStream(c0.stream)

# ---- (a) the shard call against the parent's call, shard 0 of WORLD, all NQ queries
keys = torch.zeros((NQ, MPQ + 1), dtype=torch.int64, device="cuda")
cnt = torch.zeros(NQ, dtype=torch.int32, device="cuda")
inr = torch.zeros(NQ, dtype=torch.int32, device="cuda")
mm = torch.zeros((NQ * MPQ, 4), dtype=torch.int32, device="cuda")
xx = torch.zeros((NQ * MPQ, 3), device="cuda")
torch.cuda.synchronize()
calls_a = {"shard": lambda: c0.match_radius_shard_device(d_q.data_ptr(), NQ, RADIUS, MPQ, keys.data_ptr()),
           "device": lambda: c0.match_radius_device(d_q.data_ptr(), NQ, RADIUS, MPQ, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr(), inr.data_ptr())}
whole = turns(st0, calls_a)
passes = {name: [] for name in calls_a}                     # the DB pass alone, from the context's kernel timing
for _ in range(args.turns):
    for name, call in calls_a.items():
        k0 = c0.counters()
        c0.set_kernel_timing(True)
        for _ in range(args.launches):
            call()
        c0.synchronize()
        c0.set_kernel_timing(False)
        k1 = c0.counters()
        passes[name].append((k1.sum_match_kernel_ms - k0.sum_match_kernel_ms) / (k1.n_match_kernel_launches - k0.n_match_kernel_launches))
n_in = inr.cpu().numpy().astype(np.int64)
say("(a) done")
a = {"what": "shard 0 of %d, %d rows of %d, %d queries, radius %d, max_per_query %d" % (WORLD, c0.db_info()["shard_rows"], int(off[-1]), NQ,
                                                                                      RADIUS, MPQ),
     "match_radius_shard_device": stats(whole["shard"]), "match_radius_device": stats(whole["device"]),
     "ratio": float(np.mean(whole["shard"]) / np.mean(whole["device"])),
     "collect_pass": {"shard": stats(passes["shard"]), "device": stats(passes["device"])},
     "in_radius_of_the_shard": {"mean": float(n_in.mean()), "max": int(n_in.max()), "queries_with_hits": int((n_in > 0).sum()),
                                "queries_beyond_the_buffer": int((n_in > capi.radius_capacity(MPQ)).sum())}}

# ---- (b) the merge of WORLD key sets for this rank's queries (the first NQ_RANK)
keys_all = torch.zeros((WORLD, NQ_RANK, MPQ + 1), dtype=torch.int64, device="cuda")
knn_all = torch.zeros((WORLD, NQ_RANK, K), dtype=torch.int64, device="cuda")
torch.cuda.synchronize()
for r, c in enumerate(shards):
    c.match_radius_shard_device(d_q.data_ptr(), NQ_RANK, RADIUS, MPQ, keys_all[r].data_ptr())
    c.match_shard_device(d_q.data_ptr(), NQ_RANK, K, RADIUS, knn_all[r].data_ptr())
    c.synchronize()
calls_b = {"radius_merge": lambda: c0.merge_radius_shards_device(keys_all.data_ptr(), WORLD, NQ_RANK, MPQ, cnt.data_ptr(), mm.data_ptr(),
                                                                  xx.data_ptr(), inr.data_ptr()),
           "knn_merge_k8": lambda: c0.merge_shards_device(knn_all.data_ptr(), WORLD, NQ_RANK, K, RADIUS, cnt.data_ptr(), mm.data_ptr(),
                                                          xx.data_ptr())}
merge = turns(st0, calls_b)
calls_b["radius_merge"]()
c0.synchronize()
m_in = inr[:NQ_RANK].cpu().numpy().astype(np.int64)
b = {"what": "%d key sets x %d queries x (%d + 1) keys" % (WORLD, NQ_RANK, MPQ),
     "merge_radius_shards_device": stats(merge["radius_merge"]), "merge_shards_device_k8": stats(merge["knn_merge_k8"]),
     "ratio_to_knn_merge": float(np.mean(merge["radius_merge"]) / np.mean(merge["knn_merge_k8"])),
     "ratio_to_collect_pass": float(np.mean(merge["radius_merge"]) / np.mean(passes["shard"])),
     "shorter_than_the_pass_it_runs_beside": bool(np.mean(merge["radius_merge"]) < np.mean(passes["shard"])),
     "in_radius": {"mean": float(m_in.mean()), "max": int(m_in.max()), "queries_with_hits": int((m_in > 0).sum())},
     "exchange_bytes_per_rank_and_step": {"radius": WORLD * NQ_RANK * (MPQ + 1) * 8, "knn_k2": WORLD * NQ_RANK * 2 * 8}}
for c in shards:
    c.close()
out = {"measured": True, "device": torch.cuda.get_device_name(0), "launches_per_turn": args.launches, "a_shard_call": a, "b_merge": b}
print(json.dumps(out))
if args.out:
    json.dump(out, open(args.out, "w"), indent=1)
