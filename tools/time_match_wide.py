"""Times the DB pass of todhip_match_device on a 64-byte DB (hamming_topk_wide, tod_amd/csrc/match_wide.hip) with the context's kernel
timing, against the yardstick of DESIGN 6h in the same process, alternating turns: the 32-byte matrix-core kernel with whole blocks
(todhip_set_matcher_engine mfma, todhip_set_matcher_block_split 0) over twice as many rows at half the radius -- the same number
of descriptor bits and the same number of matrix instructions (32 000 x 500 000 x 8 = 32 000 x 1 000 000 x 4 per 1024 pairs).
Independent-bit rows and queries from synth.make_db. Also event-times both whole calls (DB pass, merge, finalize).
Prints one JSON object and writes it to --out.

    timeout 600 python tools/time_match_wide.py --out profiles/match_wide.json"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from tod_amd import capi, synth

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=500000, help="rows of the 64-byte DB; the 32-byte yardstick gets twice as many")
ap.add_argument("--queries", type=int, default=32000)
ap.add_argument("--k", type=int, default=2)
ap.add_argument("--radius", type=int, default=70, help="of the 64-byte search; the yardstick gets half")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--launches", type=int, default=20, help="timed launches per turn")
ap.add_argument("--turns", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
N_OBJ = 200


def side(desc_bytes, rows, radius, seed):
    """a context with its DB, device-resident queries and output buffers, and the call that is timed"""
    desc, pts, off = synth.make_db(N_OBJ, per_object=rows // N_OBJ, desc_bytes=desc_bytes)
    rng = np.random.default_rng(seed)
    nq, k = args.queries, args.k
    c = capi.Context(0)
    c.set_matcher_engine("mfma")
    c.set_matcher_block_split(0)
    c.db_load(desc, pts, off)
    d_q = torch.from_numpy(rng.integers(0, 256, (nq, desc_bytes), dtype=np.uint8)).cuda()
    cnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
    mm = torch.zeros((nq * k, 4), dtype=torch.int32, device="cuda")
    xx = torch.zeros((nq * k, 3), device="cuda")
    torch.cuda.synchronize()
    keep = (d_q, cnt, mm, xx)
    return c, (lambda: c.match_device(d_q.data_ptr(), nq, k, radius, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr())), keep, int(off[-1])


sides = {"wide": side(64, args.rows, args.radius, 1), "narrow": side(32, 2 * args.rows, args.radius // 2, 2)}
ms = {name: [] for name in sides}
for name, (c, call, _, _) in sides.items():
    for _ in range(args.warmup):
        call()
    c.synchronize()
for turn in range(args.turns):
    for name, (c, call, _, _) in sides.items():
        c0 = c.counters()
        c.set_kernel_timing(True)
        for _ in range(args.launches):
            call()
        c.synchronize()
        c.set_kernel_timing(False)
        c1 = c.counters()
        ms[name].append((c1.sum_match_kernel_ms - c0.sum_match_kernel_ms) / (c1.n_match_kernel_launches - c0.n_match_kernel_launches))
whole, split = {}, {}
for name, (c, call, _, _) in sides.items():
    with torch.cuda.stream(torch.cuda.ExternalStream(c.stream)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            call()
        e1.record()
        e1.synchronize()
        whole[name] = e0.elapsed_time(e1) / args.launches
    split[name] = int(c.counters().last_block_split)
    c.close()
w, n = float(np.mean(ms["wide"])), float(np.mean(ms["narrow"]))
out = {"measured": True,
       "what": "independent-bit rows and queries (synth.make_db), k = %d, matrix-core engine, whole blocks" % args.k,
       "wide": {"desc_bytes": 64, "rows": sides["wide"][3], "queries": args.queries, "radius": args.radius, "db_pass_ms": w,
                "db_pass_ms_turns": ms["wide"], "whole_call_ms": whole["wide"], "last_block_split": split["wide"]},
       "yardstick": {"desc_bytes": 32, "rows": sides["narrow"][3], "queries": args.queries, "radius": args.radius // 2, "db_pass_ms": n,
                     "db_pass_ms_turns": ms["narrow"], "whole_call_ms": whole["narrow"], "last_block_split": split["narrow"],
                     "kernel": "hamming_topk_mfma, whole blocks (todhip_set_matcher_block_split 0)"},
       "ratio": w / n,
       "split_form": "not built: the wide pass has whole blocks only (DESIGN 6h)"}
print(json.dumps(out))
if args.out:
    json.dump(out, open(args.out, "w"), indent=1)
