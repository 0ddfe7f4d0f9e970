"""What todhip_set_db_bit_order does to the matrix-core matcher's DB pass on the data it is meant for: the `chained` block's trained DB
(scenes.train_db: this library's ORB descriptors of rendered views, 200 objects x 5000 rows) with the ORB descriptors of 32 rendered
detection views as queries (32 x 1000, k = 2, radius 35) -- order off against order on IN THE SAME PROCESS, alternating, so that
clocks and neighbours are shared. Per block split (forced 2, 3, 0 = whole blocks, and adaptive): the mean time of the DB-pass kernel
(todhip_set_kernel_timing), the fraction of split blocks that went on to their second part, and, adaptive, the split in use after 100
launches. Also the one-off cost at load and the cost of permuting 32 000 queries. Prints one JSON object (and writes it to --out).

    timeout 900 python tools/bit_order_chained.py --out profiles/bit_order_chained.json"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from tod_amd import capi, scenes

K, RADIUS, NQ, FRAMES = 2, 35, 1000, 32
ap = argparse.ArgumentParser()
ap.add_argument("--objects", type=int, default=200)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--launches", type=int, default=25, help="timed launches per turn; off and on take --turns turns each, alternating")
ap.add_argument("--turns", type=int, default=4)
ap.add_argument("--out", default=None)
args = ap.parse_args()

# ---- the chained block's DB and queries
tex = scenes.make_textures(args.objects)
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
n = FRAMES * NQ
d_c = torch.zeros(n, dtype=torch.int32, device="cuda")
d_m = torch.zeros((n * K, 4), dtype=torch.int32, device="cuda")
d_x = torch.zeros((n * K, 3), device="cuda")
torch.cuda.synchronize()

# ---- two contexts, the same DB; the load is timed on its second run (buffers exist, code objects are loaded)
ctxs, load_ms = {}, {}
for name, mode in (("off", 0), ("on", 1)):
    c = capi.Context(0)
    c.set_db_bit_order(mode)
    c.set_matcher_engine("mfma")
    c.db_load(desc, pts, off)
    ctxs[name] = c
for turn in range(3):
    for name, c in ctxs.items():
        t0 = time.perf_counter()
        c.db_load(desc, pts, off)
        load_ms.setdefault(name, []).append((time.perf_counter() - t0) * 1e3)
order = ctxs["on"].db_bit_order()


def launch(c):
    c.match_device(d_q.data_ptr(), n, K, RADIUS, d_c.data_ptr(), d_m.data_ptr(), d_x.data_ptr())


def result(c):
    c.synchronize()
    return d_c.cpu().numpy().copy(), d_m.cpu().numpy().copy()


launch(ctxs["off"])
want = result(ctxs["off"])
launch(ctxs["on"])
got = result(ctxs["on"])
identical = bool(np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]))   # (slots beyond a query's count are never written: zeros in both)

out = {"what": "hamming_topk_mfma on the chained DB, todhip_set_db_bit_order off against on in one process, alternating turns",
       "rows": int(off[-1]), "queries": n, "k": K, "radius": RADIUS, "results_identical": identical,
       "positions_moved": int((order != np.arange(256)).sum()),
       "load_ms": {k_: min(v[1:]) for k_, v in load_ms.items()}, "splits": {}}
out["load_cost_of_the_order_ms"] = out["load_ms"]["on"] - out["load_ms"]["off"]

for split in (2, 3, 0, -1):
    res = {name: {"ms": [], "blocks": 0, "completed": 0} for name in ctxs}
    for c in ctxs.values():
        c.set_matcher_block_split(split)
        for _ in range(100 if split < 0 else args.warmup):             # adaptive: the controller has settled after 100 launches
            launch(c)
        c.synchronize()
        launch(c)                                                      # reads the report of the launches before it
        c.synchronize()
    if split < 0:
        for name, c in ctxs.items():
            res[name]["last_block_split"] = int(c.counters().last_block_split)
    for turn in range(args.turns):
        for name, c in ctxs.items():
            c0 = c.counters()
            c.set_kernel_timing(True)
            for _ in range(args.launches):
                launch(c)
            c.synchronize()
            c.set_kernel_timing(False)
            launch(c)                                                  # one further launch reads the measured launches' report
            c.synchronize()
            c1 = c.counters()
            res[name]["ms"].append((c1.sum_match_kernel_ms - c0.sum_match_kernel_ms) / (c1.n_match_kernel_launches - c0.n_match_kernel_launches))
            res[name]["blocks"] += int(c1.k4x_half_blocks - c0.k4x_half_blocks)
            res[name]["completed"] += int(c1.k4x_half_blocks_completed - c0.k4x_half_blocks_completed)
    for name, r in res.items():
        r["mean_kernel_ms"] = float(np.mean(r["ms"]))
        r["fraction_completed"] = r["completed"] / r["blocks"] if r["blocks"] else None
        if split < 0:
            r["last_block_split_at_end"] = int(ctxs[name].counters().last_block_split)
    out["splits"]["adaptive" if split < 0 else str(split)] = res

# ---- the query permutation alone: 32 000 queries against a 4096-row DB (the search itself is some ten microseconds there), whole calls
# timed with events on the contexts' shared stream, order on minus order off
st = torch.cuda.Stream()
small = {}
rng = np.random.default_rng(1)
tiny = rng.integers(0, 256, (4096, 32), dtype=np.uint8)
tiny[:, :16] = tiny[0, :16]                                            # constant positions: the order is not the identity
for name, mode in (("off", 0), ("on", 1)):
    c = capi.Context(0, stream=st.cuda_stream)
    c.set_db_bit_order(mode)
    c.set_matcher_engine("mfma")
    c.db_load(tiny, rng.standard_normal((4096, 3)).astype(np.float32), [0, 4096])
    small[name] = c
call_ms = {"off": [], "on": []}
with torch.cuda.stream(st):
    for turn in range(args.turns + 1):
        for name, c in small.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                launch(c)
            e1.record()
            e1.synchronize()
            if turn:                                                   # the first turn warms up
                call_ms[name].append(e0.elapsed_time(e1) / 200.0)
out["query_permutation"] = {"what": "todhip_match_device of 32 000 queries on a 4096-row DB, event-timed whole calls (ms), order on minus off",
                            "call_ms": {k_: float(np.mean(v)) for k_, v in call_ms.items()}, "call_ms_turns": call_ms,
                            "permutation_ms": float(np.mean(call_ms["on"]) - np.mean(call_ms["off"]))}
for c in list(ctxs.values()) + list(small.values()):
    c.close()
print(json.dumps(out))
if args.out:
    json.dump(out, open(args.out, "w"), indent=1)
