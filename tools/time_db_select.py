"""What todhip_db_select_objects costs and saves on the headline shape: the synthetic 1M-row DB (200 objects x 5000 rows), 32 000
queries in one todhip_match_device call, k 2, radius 35. For selected shares of 100 % (NULL), 50 %, 10 % and 1 % of the objects:
the wall time of the select call, the DB-pass kernel time (todhip_set_kernel_timing) and the whole match call by HIP events -- each
the median of CALLS calls after WARMUP, repeated REPEATS times in one process; the JSON keeps every repeat's median, so the spread
of repeated runs is there to compare against.

  python tools/time_db_select.py [--parent-lib path/to/libtodhip.so] [--out profiles/db_select.json]

--parent-lib: a build of the parent commit's library. The unrestricted case is then measured again in a fresh process of this same
script with TODHIP_LIB_PATH pointing at it (that library has no selection: nothing else can be measured on it)."""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

N_OBJ, NQ_FRAME, FRAMES, K, RADIUS = 200, 1000, 32, 2, 35
WARMUP, CALLS, REPEATS = 5, 20, 5
SHARES = (("100% (NULL)", None), ("50%", 100), ("10%", 20), ("1%", 2))


def measure(only_null):
    import numpy as np
    import torch
    from tod_amd import capi, synth
    desc, pts, off = synth.make_db(N_OBJ)
    q = np.concatenate([synth.make_frame(desc, pts, off, NQ_FRAME, frame=f, visible_object=(17 * f + 3) % N_OBJ)["q_desc"]
                        for f in range(FRAMES)])
    n = len(q)
    ctx = capi.Context(0)
    ctx.db_load(desc, pts, off)
    ctx.set_kernel_timing(True)
    d_q = torch.from_numpy(q).cuda()
    d_c = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_m = torch.zeros((n * K, 4), dtype=torch.int32, device="cuda")
    d_x = torch.zeros((n * K, 3), device="cuda")
    stream = torch.cuda.ExternalStream(ctx.stream)
    call = lambda: ctx.match_device(d_q.data_ptr(), n, K, RADIUS, d_c.data_ptr(), d_m.data_ptr(), d_x.data_ptr())
    rng = np.random.Generator(np.random.PCG64(1))
    out = []
    for name, n_sel in SHARES:
        if only_null and n_sel is not None:
            continue
        ids = None if n_sel is None else sorted(int(i) for i in rng.permutation(N_OBJ)[:n_sel])
        row = dict(share=name, selected_objects=N_OBJ if ids is None else len(ids), repeats=[])
        for _ in range(REPEATS):
            rep = {}
            if not only_null:
                t_sel = []
                for _ in range(3):                                      # the select call itself: back to all, then the timed one
                    if ids is not None:
                        ctx.select_objects(None)
                    t0 = time.perf_counter()
                    ctx.select_objects(ids)
                    t_sel.append((time.perf_counter() - t0) * 1e3)
                rep["select_ms_median_of_3"] = float(np.median(t_sel))
                row["selected_rows"] = ctx.selection()["rows"]
            for _ in range(WARMUP):
                call()
            ctx.synchronize()
            kern, whole = [], []
            for _ in range(CALLS):
                c0 = ctx.counters()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call()
                e1.record(stream)
                e1.synchronize()
                c1 = ctx.counters()
                whole.append(e0.elapsed_time(e1))
                kern.append(c1.sum_match_kernel_ms - c0.sum_match_kernel_ms)
            rep["db_pass_kernel_ms_median"] = float(np.median(kern))
            rep["match_device_ms_median"] = float(np.median(whole))
            row["repeats"].append(rep)
        for key in row["repeats"][0]:
            v = [r[key] for r in row["repeats"]]
            row[key] = dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
        row["matches"] = int(d_c.sum().item())
        out.append(row)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join("profiles", "db_select.json"))
    ap.add_argument("--only-null", action="store_true", help="the unrestricted case alone (what a library without the call can run)")
    a = ap.parse_args()
    res = dict(workload=dict(db_rows=N_OBJ * 5000, objects=N_OBJ, queries=NQ_FRAME * FRAMES, k=K, radius=RADIUS),
               method=dict(warmup=WARMUP, calls=CALLS, repeats=REPEATS, timing="HIP events around todhip_match_device on the context's stream; "
                           "todhip_set_kernel_timing for the DB pass; time.perf_counter around todhip_db_select_objects"),
               measured=True, this_commit=measure(a.only_null))
    if a.parent_lib:
        tmp = a.out + ".parent.tmp"
        env = dict(os.environ, TODHIP_LIB_PATH=os.path.abspath(a.parent_lib))
        subprocess.run([sys.executable, os.path.abspath(__file__), "--only-null", "--out", tmp], check=True, env=env)
        res["parent_commit_unrestricted"] = json.load(open(tmp))["this_commit"]
        os.remove(tmp)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    for row in res["this_commit"] + res.get("parent_commit_unrestricted", []):
        print({k: v for k, v in row.items() if k != "repeats"})


if __name__ == "__main__":
    main()
