"""Child process of tests/test_l2_sharded_gpu.py (started before anything touches the GPU): torch.distributed on the "nccl" backend
(= RCCL on ROCm) with ONE rank, tod_amd/sharded.py::ShardedMatcher(desc_bytes=512) over GpuOps(metric="l2") -- the float pairs behind
the same choreography, collectives and event edges as the Hamming forms -- for 3 consecutive steps of the k-NN form (k = 5) and of
the radius form (64 per query), overlapped and serial; every step's outputs must equal todhip_match_l2_device /
todhip_match_l2_radius_device on the whole DB, counts and in_radius whole, matches and points up to counts[q]."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
os.environ.setdefault("MASTER_PORT", "29652")
os.environ["RANK"], os.environ["WORLD_SIZE"], os.environ["LOCAL_RANK"] = "0", "1", "0"
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np
import torch
import torch.distributed as dist

from tod_amd import capi, sharded

K, MPQ, RADIUS, NQ, B, STEPS = 5, 64, 60.0, 200, 3, 3

torch.cuda.set_device(0)
dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
assert dist.get_backend() == "nccl" and dist.get_world_size() == 1

rng = np.random.Generator(np.random.PCG64(321))
off = np.concatenate([[0], np.cumsum([2500, 40, 0, 1900, 3500, 5, 2610])]).astype(np.uint32)
n_rows = int(off[-1])
desc = (rng.random((n_rows, 128)) * 200).astype(np.float32)
desc[3000:3200] = desc[2999]                                # 201 equal rows: more than max_per_query inside any radius
pts = rng.standard_normal((n_rows, 3)).astype(np.float32)
compute, comm = torch.cuda.Stream(), torch.cuda.Stream()
ctx = capi.Context(0, compute.cuda_stream)                  # this rank's shard: with one rank, every row
ctx.db_load(desc, pts, off, 0, 1)
ref = capi.Context(0)                                       # the unsharded matcher, on a stream of its own
ref.db_load(desc, pts, off)


def frame(i, b):
    """half the queries about 34 from a row (inside the radius: a sigma of 3 over 128 dimensions), the rest random; one meets the equal rows"""
    q = (rng.random((NQ, 128)) * 200).astype(np.float32)
    q[::2] = (desc[rng.integers(0, n_rows, NQ // 2)] + rng.normal(0, 3.0, (NQ // 2, 128))).astype(np.float32)
    if b == 0:
        q[i] = desc[2999]
    return q


q_dev = [torch.from_numpy(np.stack([frame(i, b) for b in range(B)])).cuda() for i in range(STEPS)]
torch.cuda.synchronize()
n = B * NQ


def new_out(width):
    return dict(counts=torch.zeros(n, dtype=torch.int32, device="cuda"), matches=torch.zeros((n * width, 4), dtype=torch.int32, device="cuda"),
                xyz=torch.zeros((n * width, 3), dtype=torch.float32, device="cuda"), in_radius=torch.zeros(n, dtype=torch.int32, device="cuda"))


n_checked = 0
for mpq in (None, MPQ):
    width = K if mpq is None else mpq
    # the reference result of every step, computed before the sharded steps run
    want = []
    for i in range(STEPS):
        o = new_out(width)
        if mpq is None:
            ref.match_l2_device(q_dev[i].data_ptr(), n, K, RADIUS, o["counts"].data_ptr(), o["matches"].data_ptr(), o["xyz"].data_ptr())
        else:
            ref.match_l2_radius_device(q_dev[i].data_ptr(), n, RADIUS, mpq, o["counts"].data_ptr(), o["matches"].data_ptr(), o["xyz"].data_ptr(),
                                       o["in_radius"].data_ptr())
        ref.synchronize()
        want.append({key: v.cpu().numpy().copy() for key, v in o.items()})
    assert all(int(w["counts"].sum()) > n // 2 for w in want) and all(int((w["counts"] == 0).sum()) > n // 4 for w in want)
    assert mpq is None or all(int(w["in_radius"].max()) > mpq for w in want)
    for exchange, overlap in (("all_to_all", True), ("all_gather", False)):
        ops = sharded.GpuOps(ctx, compute, comm, "nccl", K, RADIUS, max_per_query=mpq, metric="l2")
        sm = sharded.ShardedMatcher(ops, 1, 0, B, NQ, K, desc_bytes=512, exchange=exchange, overlap=overlap, max_per_query=mpq)
        assert sm.overlap == overlap and sm.keys[0].shape == (n, K if mpq is None else mpq + 1)
        outs = [new_out(width) for _ in range(STEPS)]
        sm.begin(STEPS, lambda i: (q_dev[i].view(torch.uint8).view(B, NQ, 512), None))      # the queries travel as bytes
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
            assert np.array_equal(got["counts"], want[i]["counts"]), (mpq, exchange, overlap, i, "counts")
            assert np.array_equal(got["in_radius"], want[i]["in_radius"]), (mpq, exchange, overlap, i, "in_radius")   # (zeros in the k-NN form)
            keep = (np.arange(width)[None, :] < got["counts"][:, None]).reshape(-1)      # the slots beyond counts[q] are not written
            assert np.array_equal(got["matches"][keep], want[i]["matches"][keep]), (mpq, exchange, overlap, i, "matches")
            assert np.array_equal(got["xyz"][keep], want[i]["xyz"][keep]), (mpq, exchange, overlap, i, "xyz")
            n_checked += 1
        torch.cuda.synchronize()
dist.destroy_process_group()
ctx.close(); ref.close()
print("ok: %d steps checked" % n_checked)
