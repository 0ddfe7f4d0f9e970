"""Child process of tests/test_match_radius_sharded_gpu.py (started before anything touches the GPU): torch.distributed on the
"nccl" backend (= RCCL on ROCm) with ONE rank, tod_amd/sharded.py::ShardedMatcher(max_per_query=64) over GpuOps -- the radius pair
behind the same choreography, collectives and event edges as the k-NN form -- for 4 consecutive steps, overlapped and serial, both
exchanges; every step's outputs must equal todhip_match_radius_device on the whole DB, counts and in_radius whole, matches and
points up to counts[q]."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
os.environ.setdefault("MASTER_PORT", "29651")
os.environ["RANK"], os.environ["WORLD_SIZE"], os.environ["LOCAL_RANK"] = "0", "1", "0"
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np
import torch
import torch.distributed as dist

from tod_amd import capi, sharded, synth

MPQ, RADIUS, NQ, B, STEPS = 64, 45, 300, 3, 4

torch.cuda.set_device(0)
dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
assert dist.get_backend() == "nccl" and dist.get_world_size() == 1

desc, pts, off = synth.make_db_ragged([2500, 40, 0, 1900, 3500, 5, 2610], seed=321)
desc[3000:3200] = desc[2999]                                # 201 equal rows: more than max_per_query inside any radius
compute, comm = torch.cuda.Stream(), torch.cuda.Stream()
ctx = capi.Context(0, compute.cuda_stream)                  # this rank's shard: with one rank, every row
ctx.db_load(desc, pts, off, 0, 1)
ref = capi.Context(0)                                       # the unsharded matcher, on a stream of its own
ref.db_load(desc, pts, off)
frames = {(i, b): synth.make_frame(desc, pts, off, NQ, frame=100 * i + b, visible_object=(0, 3, 4, 6)[(i + b) % 4])
          for i in range(STEPS) for b in range(B)}
for i in range(STEPS):
    frames[(i, 0)]["q_desc"][i] = desc[2999]                # one query per step meets them
q_dev = [torch.from_numpy(np.stack([frames[(i, b)]["q_desc"] for b in range(B)])).cuda() for i in range(STEPS)]
torch.cuda.synchronize()
n = B * NQ


def new_out():
    return dict(counts=torch.zeros(n, dtype=torch.int32, device="cuda"), matches=torch.zeros((n * MPQ, 4), dtype=torch.int32, device="cuda"),
                xyz=torch.zeros((n * MPQ, 3), dtype=torch.float32, device="cuda"), in_radius=torch.zeros(n, dtype=torch.int32, device="cuda"))


# the reference result of every step, computed before anything else runs
want = []
for i in range(STEPS):
    o = new_out()
    ref.match_radius_device(q_dev[i].data_ptr(), n, RADIUS, MPQ, o["counts"].data_ptr(), o["matches"].data_ptr(), o["xyz"].data_ptr(),
                            o["in_radius"].data_ptr())
    ref.synchronize()
    want.append({key: v.cpu().numpy().copy() for key, v in o.items()})
assert sum(int(w["counts"].sum()) for w in want) > STEPS * B * 50 and all(int(w["in_radius"].max()) > MPQ for w in want)

n_checked = 0
for exchange in ("all_to_all", "all_gather"):
    for overlap in (True, False):
        ops = sharded.GpuOps(ctx, compute, comm, "nccl", 2, RADIUS, max_per_query=MPQ)
        sm = sharded.ShardedMatcher(ops, 1, 0, B, NQ, 2, exchange=exchange, overlap=overlap, max_per_query=MPQ)
        assert sm.overlap == overlap and sm.keys[0].shape == (n, MPQ + 1)
        outs = [new_out() for _ in range(STEPS)]
        sm.begin(STEPS, lambda i: (q_dev[i], None))
        done = []
        for i in range(STEPS):
            s = sm.step(i, outs[i])
            assert s is (comm if overlap else compute)
            ev = torch.cuda.Event()
            ev.record(s)
            done.append(ev)
        for i in range(STEPS):
            done[i].synchronize()
            got = {key: v.cpu().numpy() for key, v in outs[i].items()}
            assert np.array_equal(got["counts"], want[i]["counts"]), (exchange, overlap, i, "counts")
            assert np.array_equal(got["in_radius"], want[i]["in_radius"]), (exchange, overlap, i, "in_radius")
            keep = (np.arange(MPQ)[None, :] < got["counts"][:, None]).reshape(-1)      # the slots beyond counts[q] are not written
            assert np.array_equal(got["matches"][keep], want[i]["matches"][keep]), (exchange, overlap, i, "matches")
            assert np.array_equal(got["xyz"][keep], want[i]["xyz"][keep]), (exchange, overlap, i, "xyz")
            n_checked += 1
        torch.cuda.synchronize()
dist.destroy_process_group()
ctx.close(); ref.close()
print("ok: %d steps checked" % n_checked)
