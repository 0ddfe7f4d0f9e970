"""Child of tests/test_match_ondemand_bounds_gpu.py (the TODHIP_K4X_* knobs are read once per process). Split 2 forced on the DBs of
tests/ondemand_bounds_cases.py, k 2 and 5, radius 35: the matrix-core answer against the vector engine of the same context and
against the definition computed on the CPU, bit for bit -- counts, matches, xyz -- and the context's counters of split blocks
tested and gone on after one launch. Prints "ok <sha256 of every answer> <tested>:<went on> ..." (one pair per DB and k): the parent
compares the digests and the counters of the forms it starts.

`extras`: the same DB behind todhip_db_select_objects, and as two shards through todhip_match_shard_device +
todhip_merge_shards_device (split 2 by TODHIP_K4X_HALF=2: every context of the process)."""
import hashlib
import os
import sys

import numpy as np

import k4x_children as C
import fastpath_cases as FC
import ondemand_bounds_cases as OC

capi = C.capi
KS = (2, 5)


def check_against_definition(got, want_keys, off, pts, what):
    row_ptr, m, xyz = got
    rows = off[m["imgIdx"]].astype(np.int64) + m["trainIdx"]
    for qi, keys in enumerate(want_keys):
        lo, hi = int(row_ptr[qi]), int(row_ptr[qi + 1])
        assert [(int(d), int(r)) for d, r in zip(m["distance"][lo:hi], rows[lo:hi])] == keys, (what, qi, keys)
        assert np.all(m["queryIdx"][lo:hi] == qi), (what, qi)
    assert np.array_equal(xyz, pts[rows]), what


def run_forms(qt):
    fp4 = int(os.environ["TODHIP_K4X_FP4_ROWS"])
    digest, counters = hashlib.sha256(), []
    for n_rows in OC.ROWS:
        for k in KS:
            desc, pts, off, q, plants = OC.make(n_rows, qt, k, 7 * n_rows + k)
            assert len(FC.tiling(n_rows)[1]) >= 8
            ctx = capi.Context(0)                              # a context per DB: its counters start at zero
            ctx.db_load(desc, pts, off)
            want = C.valu_answer(ctx, q, k, OC.RADIUS)
            check_against_definition(want, OC.knn(desc, q, k, OC.RADIUS), off, pts, (n_rows, k, "valu"))
            ctx.set_matcher_engine("mfma")
            ctx.set_matcher_block_split(2)
            seen = []
            for _ in range(2):                                 # a launch's report is taken when the next launch starts
                got = ctx.match(q, k, OC.RADIUS)
                cnt = ctx.counters()
                assert cnt.last_block_split == 2 and cnt.last_fp4_rows == fp4, (n_rows, k, cnt.last_block_split, cnt.last_fp4_rows)
                assert C.same(got, want), (n_rows, k)
                seen.append((int(cnt.k4x_half_blocks), int(cnt.k4x_half_blocks_completed)))
            assert seen[0] == (0, 0), seen
            counters.append(seen[1])
            digest.update(np.ascontiguousarray(got[0]).tobytes())
            for f in C.FIELDS:
                digest.update(np.ascontiguousarray(got[1][f]).tobytes())
            digest.update(np.ascontiguousarray(got[2]).tobytes())
            ctx.close()
    print("ok %s %s" % (digest.hexdigest(), " ".join("%d:%d" % c for c in counters)))


def run_extras(qt):
    import torch
    assert os.environ.get("TODHIP_K4X_HALF") == "2"
    n_rows, k = OC.ROWS[1], 2
    desc, pts, off, q, plants = OC.make(n_rows, qt, k, 7 * n_rows + k)
    nq = len(q)
    # (1) a selection of objects: the rows searched change, the numbering of the answer does not
    ids = [7, 1, 4, 5, 1]
    rows = np.concatenate([np.arange(off[i], off[i + 1]) for i in sorted(set(ids))])
    ctx = capi.Context(0)
    ctx.db_load(desc, pts, off)
    ctx.select_objects(ids)
    assert ctx.selection()["rows"] == len(rows)
    want = C.valu_answer(ctx, q, k, OC.RADIUS)
    check_against_definition(want, OC.knn(desc, q, k, OC.RADIUS, rows), off, pts, "selection, valu")
    ctx.set_matcher_engine("mfma")
    got = ctx.match(q, k, OC.RADIUS)
    cnt = ctx.counters()
    assert cnt.last_block_split == 2 and cnt.last_fp4_rows == 1
    assert C.same(got, want), "selection"
    ctx.select_objects(None)
    whole = ctx.match(q, k, OC.RADIUS)
    check_against_definition(whole, OC.knn(desc, q, k, OC.RADIUS), off, pts, "whole DB")
    ctx.close()
    # (2) two object-aligned shards, merged on the device
    d_q = torch.from_numpy(q).cuda()
    keys_all = torch.empty((2, nq, k), dtype=torch.int64, device="cuda")
    ctxs = []
    for s in range(2):
        c = capi.Context(0)
        c.set_matcher_engine("mfma")
        c.db_load(desc, pts, off, shard_rank=s, shard_count=2)
        c.match_shard_device(d_q.data_ptr(), nq, k, OC.RADIUS, keys_all[s].data_ptr())
        c.synchronize()
        cnt = c.counters()
        assert cnt.last_block_split == 2 and cnt.last_fp4_rows == 1
        ctxs.append(c)
    counts = torch.empty(nq, dtype=torch.int32, device="cuda")
    m = torch.empty((nq * k, 4), dtype=torch.int32, device="cuda")
    xyz = torch.empty((nq * k, 3), dtype=torch.float32, device="cuda")
    ctxs[0].merge_shards_device(keys_all.data_ptr(), 2, nq, k, OC.RADIUS, counts.data_ptr(), m.data_ptr(), xyz.data_ptr())
    ctxs[0].synchronize()
    for c in ctxs:
        c.close()
    counts = counts.cpu().numpy()
    keep = np.arange(k)[None, :] < counts[:, None]
    m = m.cpu().numpy().view(capi.DMATCH_DTYPE).reshape(nq, k)[keep]
    xyz = xyz.cpu().numpy().reshape(nq, k, 3)[keep]
    assert np.array_equal(np.diff(whole[0].astype(np.int64)), counts)
    assert all(np.array_equal(m[f], whole[1][f]) for f in C.FIELDS) and np.array_equal(xyz, whole[2])
    print("ok extras")


if __name__ == "__main__":
    assert os.environ.get("TODHIP_K4X_QT") in ("4", "6") and os.environ.get("TODHIP_K4X_FP4_ROWS") in ("0", "1")
    if len(sys.argv) > 1 and sys.argv[1] == "extras":
        run_extras(int(os.environ["TODHIP_K4X_QT"]))
    else:
        run_forms(int(os.environ["TODHIP_K4X_QT"]))
