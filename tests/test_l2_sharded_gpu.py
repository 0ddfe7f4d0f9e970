"""todhip_match_l2_shard_device + todhip_merge_l2_shards_device[_on] and todhip_match_l2_radius_shard_device +
todhip_merge_l2_radius_shards_device[_on] on the GPU: one context per shard on device 0 (db_load(shard_rank, shard_count)) plus an
unsharded context. What a shard sends equals the numpy definition (tests/l2_sharded_ref.py) in every slot; what a merge leaves equals
what todhip_match_l2_device / todhip_match_l2_radius_device leave on the unsharded context, byte for byte over whole prefilled
buffers, and the oracle (k-NN) or the numpy definition (radius).

The small DB (l2_sharded_ref.make_db): objects short of, on and past the 32-row tile, an empty one, shards without rows (world 8),
288 copies of one row in every shard, so that equal d2 is ordered by global row across every shard boundary and k and max_per_query
cut inside the tie. Its 1059 rows cannot overflow a query's candidate lists (2048 rows); the larger shapes below do: a cluster that
one shard holds most of, a shard whose Rmax is a thousand times the others', and 70 000 rows that take another path of the search
unsharded (one GEMM), in 2 shards (seed and two GEMMs) and in 8."""
import os
import subprocess
import sys

import numpy as np
import pytest

import l2_sharded_ref as S
import match_l2_radius_ref as R
import oracle_lib as O
from tod_amd import capi, sharded

pytestmark = pytest.mark.gpu

WORLDS = (1, 2, 3, 4, 8)
MPQS = (1, 5, 64, 1024)
FIELDS = ("queryIdx", "trainIdx", "imgIdx", "distance")
SENTINEL = 0x5A5A5A5A
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "l2_sharded_gpu_child.py")


def load(desc, off, pts, rank=0, world=1, stream=None):
    c = capi.Context(0, stream)
    c.db_load(desc, pts, off, shard_rank=rank, shard_count=world)
    return c


def shard_rows(off, world):
    return [np.arange(lo, hi) for _, _, lo, hi in (sharded.shard_bounds(off, r, world) for r in range(world))]


@pytest.fixture(scope="module")
def db():
    desc, off, pts, q = S.make_db()
    return dict(desc=desc, off=off, pts=pts, q=q, dd=R.d2(desc, q), radii=S.radii(desc, q))


@pytest.fixture(scope="module")
def ctxs(db):
    """{world: its shard contexts}; world 1's only context is the unsharded one"""
    out = {w: [load(db["desc"], db["off"], db["pts"], r, w) for r in range(w)] for w in WORLDS}
    yield out
    for cs in out.values():
        for c in cs:
            c.close()


def prefilled(nq, width):
    """(counts, matches, xyz, in_radius), filled so that an unwritten slot shows"""
    import torch
    return (torch.full((nq,), 77, dtype=torch.int32, device="cuda"), torch.full((nq * width, 4), SENTINEL, dtype=torch.int32, device="cuda"),
            torch.full((nq * width, 3), -7.5, dtype=torch.float32, device="cuda"), torch.full((nq,), 78, dtype=torch.int32, device="cuda"))


def to_numpy(bufs):
    return tuple(b.cpu().numpy() for b in bufs)


def dev_q(q):
    import torch
    return torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda()


def unsharded_knn(c, q, k, radius):
    import torch
    d_q, bufs = dev_q(q), prefilled(len(q), k)
    torch.cuda.synchronize()
    c.match_l2_device(d_q.data_ptr(), len(q), k, radius, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr())
    c.synchronize()
    return to_numpy(bufs[:3])


def unsharded_radius(c, q, radius, mpq):
    import torch
    d_q, bufs = dev_q(q), prefilled(len(q), mpq)
    torch.cuda.synchronize()
    c.match_l2_radius_device(d_q.data_ptr(), len(q), radius, mpq, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr())
    c.synchronize()
    return to_numpy(bufs)


def shard_keys_dev(shards, q, k=None, radius=None, mpq=None):
    """the shards' answers as one device tensor i64[n_shards, nq, k or mpq + 1], prefilled so that an unwritten slot shows"""
    import torch
    d_q = dev_q(q)
    keys = torch.full((len(shards), len(q), k if mpq is None else mpq + 1), 0x1234567, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for s, c in enumerate(shards):
        if mpq is None:
            c.match_l2_shard_device(d_q.data_ptr(), len(q), k, keys[s].data_ptr())
        else:
            c.match_l2_radius_shard_device(d_q.data_ptr(), len(q), radius, mpq, keys[s].data_ptr())
    for c in shards:
        c.synchronize()
    return keys


def merged_knn(c, keys, radius, stream=None):
    import torch
    n_shards, nq, k = keys.shape
    bufs = prefilled(nq, k)
    torch.cuda.synchronize()
    c.merge_l2_shards_device(keys.data_ptr(), n_shards, nq, k, radius, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                             stream=None if stream is None else stream.cuda_stream)
    c.synchronize()
    if stream is not None:
        stream.synchronize()
    return to_numpy(bufs[:3])


def merged_radius(c, keys, with_in_radius=True, stream=None):
    import torch
    n_shards, nq, width = keys.shape
    bufs = prefilled(nq, width - 1)
    torch.cuda.synchronize()
    c.merge_l2_radius_shards_device(keys.data_ptr(), n_shards, nq, width - 1, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                                    bufs[3].data_ptr() if with_in_radius else None, stream=None if stream is None else stream.cuda_stream)
    c.synchronize()
    if stream is not None:
        stream.synchronize()
    return to_numpy(bufs)


def unpack(raw, width):
    """whole fixed-stride buffers -> (row_ptr, matches, xyz[, in_radius]); the slots behind counts[q] must hold the prefill"""
    cnt, mm, xx = raw[:3]
    nq = len(cnt)
    cnt = cnt.astype(np.int64)
    keep = np.arange(width)[None, :] < cnt[:, None]
    assert (mm.reshape(nq, width, 4)[~keep] == SENTINEL).all() and (xx.reshape(nq, width, 3)[~keep] == -7.5).all(), "slots behind counts[q] were written"
    return (np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32), mm.view(capi.DMATCH_DTYPE).reshape(nq, width)[keep],
            xx.reshape(nq, width, 3)[keep]) + tuple(r.astype(np.uint32) for r in raw[3:])


def same(got, want, what=""):
    assert len(got) == len(want), what
    assert np.array_equal(got[0], want[0]), what
    for f in FIELDS:
        assert np.array_equal(got[1][f], want[1][f]), (what, f)
    for a, b in zip(got[2:], want[2:]):
        assert np.array_equal(a, b), what


def same_bytes(a, b, what=""):
    assert len(a) == len(b), what
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes(), what


def prefix(want, nq):
    n = int(want[0][nq])
    return (want[0][:nq + 1], want[1][:n], want[2][:n]) + tuple(w[:nq] for w in want[3:])


# ---------------------------------------------------------------------------------------------------- 1. the load
def test_a_float_db_loads_in_shards_and_the_unsharded_calls_refuse_a_shard(db):
    """(the parent refuses the load: TODHIP_EINVAL for desc_bytes == 512 with shard_count > 1)"""
    shards = [load(db["desc"], db["off"], db["pts"], r, 3) for r in range(3)]
    try:
        info = [c.db_info() for c in shards]
        want = [sharded.shard_bounds(db["off"], r, 3) for r in range(3)]
        assert [i["shard_rows"] for i in info] == [hi - lo for _, _, lo, hi in want] and sum(i["shard_rows"] for i in info) == 1059
        assert [i["shard_first"] for i in info] == [lo for _, _, lo, _ in want]
        assert all(i["total_rows"] == 1059 and i["n_objs"] == 10 for i in info) and all(c.desc_bytes() == 512 for c in shards)
        for c in shards:
            for call in (lambda: c.match_l2(db["q"], 2, 100.0), lambda: c.match_l2_radius(db["q"], 100.0, 5)):
                with pytest.raises(capi.TodError) as e:
                    call()
                assert e.value.status == capi.EINVAL
    finally:
        for c in shards:
            c.close()


# ---------------------------------------------------------------------------------------------------- 2. the small DB, k-NN
_ORACLE = {}


def oracle_knn(db, k, radius):
    if (k, radius) not in _ORACLE:
        rc, rp, m, xyz = O.l2_match(db["desc"], db["off"], db["pts"], db["q"], k, radius)
        assert rc == 0
        _ORACLE[(k, radius)] = (rp, m, xyz)
    return _ORACLE[(k, radius)]


@pytest.mark.parametrize("world", WORLDS)
def test_knn_shard_keys_and_merge_equal_the_definition_and_the_unsharded_call(ctxs, db, world):
    one, q = ctxs[1][0], db["q"]
    rows = shard_rows(db["off"], world)
    n_cut = 0
    for k in range(1, 9):
        for nq in ((1, 33) if k in (2, 5) else (33,)):
            keys = shard_keys_dev(ctxs[world], q[:nq], k=k)
            want_keys = np.stack([S.shard_keys_knn(db["desc"], db["off"], q, k, r, db["dd"]) for r in rows])[:, :nq]
            assert np.array_equal(keys.cpu().numpy().view(np.uint64), want_keys), (world, k, nq)      # every slot: keys and padding
            for radius in db["radii"]:
                what = (world, k, nq, radius)
                got = merged_knn(ctxs[world][-1], keys, radius)
                same_bytes(got, unsharded_knn(one, q[:nq], k, radius), what)
                same(unpack(got, k), prefix(oracle_knn(db, k, radius), nq), what)
                n_cut += int((got[0] < k).sum())
        if world > 1 and k > 1:                                  # query 0 is the tie's row: d2 = 0 in the lists of several shards
            assert ((want_keys[:, 0, 0] >> np.uint64(32)) == 0).sum() > 1
    assert n_cut > 0


# ---------------------------------------------------------------------------------------------------- 3. the small DB, radius pair
_WANT = {}


def want_radius(db, radius, mpq):
    if (radius, mpq) not in _WANT:
        _WANT[(radius, mpq)] = R.match_l2_radius(db["desc"], db["off"], db["pts"], db["q"], radius, mpq, db["dd"])
    return _WANT[(radius, mpq)]


@pytest.mark.parametrize("world", WORLDS)
def test_radius_shard_keys_and_merge_equal_the_definition_and_the_unsharded_call(ctxs, db, world):
    one, q = ctxs[1][0], db["q"]
    rows = shard_rows(db["off"], world)
    n_over = n_under = 0
    for radius in db["radii"][1:]:                              # the whole tie inside, then more and more rows
        for mpq in MPQS:
            what = (world, radius, mpq)
            want = want_radius(db, radius, mpq)
            keys = shard_keys_dev(ctxs[world], q, radius=radius, mpq=mpq)
            want_keys = np.stack([S.shard_keys_radius(db["desc"], db["off"], q, radius, mpq, r, db["dd"]) for r in rows])
            assert np.array_equal(keys.cpu().numpy().view(np.uint64), want_keys), what      # every slot: keys, padding, count
            got = merged_radius(ctxs[world][-1], keys)
            same_bytes(got, unsharded_radius(one, q, radius, mpq), what)
            same(unpack(got, mpq), want, what)
            n_over += int((want[3] > mpq).sum())
            n_under += int((want[3] < mpq).sum())
    assert n_over > 0 and n_under > 0
    assert (want_radius(db, db["radii"][1], 64)[3][0::6] == len(S.TIE_ROWS) + 1).all()      # in_radius > max_per_query: the tie is cut


def test_in_radius_may_be_null_and_one_query(ctxs, db):
    keys = shard_keys_dev(ctxs[3], db["q"], radius=900.0, mpq=5)
    got = merged_radius(ctxs[3][0], keys, with_in_radius=False)
    assert (got[3] == 78).all()
    same_bytes(got[:3], merged_radius(ctxs[3][0], keys)[:3])
    keys = shard_keys_dev(ctxs[3], db["q"][:1], radius=900.0, mpq=5)
    same_bytes(merged_radius(ctxs[3][1], keys), unsharded_radius(ctxs[1][0], db["q"][:1], 900.0, 5))


def test_counters_and_kernel_timing(ctxs, db):
    import torch
    c = ctxs[2][0]
    d_q = dev_q(db["q"])
    keys = torch.zeros((33, 65), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    c.set_kernel_timing(True)
    try:
        before = c.counters().n_match_kernel_launches
        c.match_l2_shard_device(d_q.data_ptr(), 33, 5, keys.data_ptr())
        c.synchronize()
        cnt = c.counters()
        assert cnt.last_nq == 33 and cnt.last_k == 5 and cnt.n_match_kernel_launches == before + 1 and cnt.last_match_kernel_ms > 0
        c.match_l2_radius_shard_device(d_q.data_ptr(), 20, 900.0, 64, keys.data_ptr())
        c.synchronize()
        cnt = c.counters()
        assert cnt.last_nq == 20 and cnt.last_k == 64 and cnt.n_match_kernel_launches == before + 2
    finally:
        c.set_kernel_timing(False)


# ---------------------------------------------------------------------------------------------------- 4. larger shapes: the paths
def all_forms_equal_unsharded(desc, off, pts, q, worlds, knn, radius_cases, merge_rank=0):
    """per world: the merged bytes of every case equal the unsharded context's. Returns the unsharded outputs and the last world's keys."""
    one = load(desc, off, pts)
    try:
        want_knn = {c: unsharded_knn(one, q, *c) for c in knn}
        want_rad = {c: unsharded_radius(one, q, *c) for c in radius_cases}
    finally:
        one.close()
    keys_rad = {}
    for world in worlds:
        shards = [load(desc, off, pts, r, world) for r in range(world)]
        try:
            for k, radius in knn:
                keys = shard_keys_dev(shards, q, k=k)
                same_bytes(merged_knn(shards[merge_rank % world], keys, radius), want_knn[(k, radius)], (world, k, radius))
            for radius, mpq in radius_cases:
                keys = shard_keys_dev(shards, q, radius=radius, mpq=mpq)
                same_bytes(merged_radius(shards[merge_rank % world], keys), want_rad[(radius, mpq)], (world, radius, mpq))
                keys_rad[(world, radius, mpq)] = keys.cpu().numpy().view(np.uint64)
        finally:
            for c in shards:
                c.close()
    return want_knn, want_rad, keys_rad


def test_the_three_paths_70000_rows():
    """70 000 random rows x 100 queries: unsharded the one-GEMM path (>= 64k rows), in 2 shards the seed and two GEMMs, in 8 shards
    about 8.7k rows each; k 2 and 5 and the radius form at 64 per query; the oracle on 16 of the queries"""
    rng = np.random.Generator(np.random.PCG64(5))
    n, nq = 70000, 100
    desc = rng.integers(0, 256, (n, 128)).astype(np.float32)
    pts = rng.standard_normal((n, 3)).astype(np.float32)
    off = np.arange(0, n + 1, 1000, dtype=np.uint32)
    q = rng.integers(0, 256, (nq, 128)).astype(np.float32)
    q[::3] = desc[rng.integers(0, n, len(q[::3]))]               # a third of the queries are rows, one component moved
    q[::3, 5] += 3
    want_knn, want_rad, keys = all_forms_equal_unsharded(desc, off, pts, q, (2, 8), ((2, 930.0), (5, 1.0e9)), ((1000.0, 64),), merge_rank=3)
    for k, radius in ((2, 930.0), (5, 1.0e9)):
        rc, rp, m, xyz = O.l2_match(desc, off, pts, q[:16], k, radius)
        assert rc == 0
        same(prefix(unpack(want_knn[(k, radius)], k), 16), (rp, m, xyz), k)
    rc, rp, m, xyz = O.l2_match(desc, off, pts, q[:16], 64, 1000.0)
    assert rc == 0
    same(prefix(unpack(want_rad[(1000.0, 64)], 64), 16)[:3], (rp, m, xyz))
    in_radius = want_rad[(1000.0, 64)][3]
    assert in_radius[::3].min() >= 1 and in_radius.max() > 8
    assert np.array_equal(keys[(8, 1000.0, 64)][:, :, 64].sum(axis=0), in_radius.astype(np.uint64))


def test_one_shard_overflows_into_the_ordered_scan_and_the_other_does_not():
    """5 000 rows; rows 0 .. 2999 a tight cluster of near ties. In 2 shards the first holds 2 500 of them -- more than a query's
    candidate lists hold, so a query inside the cluster takes the exact scan (k-NN) or the ordered scan (radius) there -- and the second
    holds 500, which fit."""
    rng = np.random.Generator(np.random.PCG64(77))
    base = rng.random(128, dtype=np.float32) * 100
    desc = (rng.random((5000, 128)) * 100).astype(np.float32)
    desc[:3000] = (base[None, :] + rng.normal(0, 0.05, (3000, 128))).astype(np.float32)
    pts = rng.random((5000, 3)).astype(np.float32)
    off = np.array([0, 1234, 2500, 5000], np.uint32)
    q = (desc[3000:3040] + rng.normal(0, 0.05, (40, 128))).astype(np.float32)
    q[::4] = (base[None, :] + rng.normal(0, 0.05, (10, 128))).astype(np.float32)
    assert [len(r) for r in shard_rows(off, 2)] == [2500, 2500]
    _, want_rad, keys = all_forms_equal_unsharded(desc, off, pts, q, (2,), ((5, 2.0), (8, 1.0e9)), ((2.0, 5), (2.0, 1024)))
    want = R.match_l2_radius(desc, off, pts, q, 2.0, 1024)
    same(unpack(want_rad[(2.0, 1024)], 1024), want)
    counts = keys[(2, 2.0, 1024)][:, :, 1024]
    assert (counts[0, ::4] == 2500).all() and (counts[1, ::4] == 500).all() and (want[3][::4] == 3000).all()


def test_a_shard_whose_rmax_is_a_thousand_times_the_others():
    """Three objects of 2 500 rows, one per shard; the middle one's rows are a cluster scaled by 1e3, so that shard's Rmax and eps(q) are a
    thousand times the others' and the queries near its rows have the whole shard inside the radius and the filter's band (the scans).
    Unsharded, the one Rmax is the large one for every row, so the queries beside the unscaled rows overflow too, while in their own
    shards the filter leaves them one candidate. The merged bytes are the same."""
    rng = np.random.Generator(np.random.PCG64(78))
    desc = (rng.random((7500, 128)) * 200).astype(np.float32)
    base = (rng.random(128) * 200).astype(np.float32)
    desc[2500:5000] = ((base[None, :] + rng.normal(0, 0.5, (2500, 128))) * 1.0e3).astype(np.float32)
    pts = rng.random((7500, 3)).astype(np.float32)
    off = np.array([0, 2500, 5000, 7500], np.uint32)
    q = (rng.random((12, 128)) * 200).astype(np.float32)
    q[0:4] = (desc[2500:2504] + rng.normal(0, 300.0, (4, 128))).astype(np.float32)           # near ties of the scaled shard
    q[4:8] = (desc[[10, 2499, 5000, 7499]] + rng.normal(0, 1.0, (4, 128))).astype(np.float32)
    assert [len(r) for r in shard_rows(off, 3)] == [2500] * 3
    # the scaled rows are 8 700 +- 550 from queries 0 .. 3 (128 dimensions of 2 x 500^2 + 300^2): all inside a radius of 12 000
    want_knn, want_rad, _ = all_forms_equal_unsharded(desc, off, pts, q, (3,), ((5, 1.2e4), (8, 1.0e9)), ((100.0, 64), (1.2e4, 64)), merge_rank=1)
    rc, rp, m, xyz = O.l2_match(desc, off, pts, q, 5, 1.2e4)
    assert rc == 0
    same(unpack(want_knn[(5, 1.2e4)], 5), (rp, m, xyz))
    same(unpack(want_rad[(1.2e4, 64)], 64), R.match_l2_radius(desc, off, pts, q, 1.2e4, 64))
    same(unpack(want_rad[(100.0, 64)], 64), R.match_l2_radius(desc, off, pts, q, 100.0, 64))
    assert (want_rad[(1.2e4, 64)][3][0:4] == 2500).all() and (want_rad[(1.2e4, 64)][3][4:] == 5000).all()
    assert not want_rad[(100.0, 64)][3][0:4].any() and (want_rad[(100.0, 64)][3][4:8] == 1).all()


# ---------------------------------------------------------------------------------------------------- 5. repeatability
def test_merges_on_a_second_stream_equal_the_plain_forms(db):
    import torch
    compute, comm = torch.cuda.Stream(), torch.cuda.Stream()
    shards = [load(db["desc"], db["off"], db["pts"], r, 2, stream=compute.cuda_stream) for r in range(2)]
    q = db["q"]
    try:
        d_q = dev_q(q)
        for k, radius, mpq in ((5, 900.0, None), (None, 900.0, 5), (None, 1.0e9, 1024)):
            width = k if mpq is None else mpq + 1
            keys = torch.zeros((2, len(q), width), dtype=torch.int64, device="cuda")
            bufs = prefilled(len(q), k if mpq is None else mpq)
            torch.cuda.synchronize()
            for s, c in enumerate(shards):
                if mpq is None:
                    c.match_l2_shard_device(d_q.data_ptr(), len(q), k, keys[s].data_ptr())
                else:
                    c.match_l2_radius_shard_device(d_q.data_ptr(), len(q), radius, mpq, keys[s].data_ptr())
            ev = torch.cuda.Event()
            ev.record(compute)
            comm.wait_event(ev)
            if mpq is None:
                shards[0].merge_l2_shards_device(keys.data_ptr(), 2, len(q), k, radius, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                                                 stream=comm.cuda_stream)
                comm.synchronize()
                same_bytes(to_numpy(bufs[:3]), merged_knn(shards[1], keys, radius), (k, radius))
                same(unpack(to_numpy(bufs[:3]), k), oracle_knn(db, k, radius))
            else:
                shards[0].merge_l2_radius_shards_device(keys.data_ptr(), 2, len(q), mpq, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                                                        bufs[3].data_ptr(), stream=comm.cuda_stream)
                comm.synchronize()
                same_bytes(to_numpy(bufs), merged_radius(shards[1], keys), (radius, mpq))
                same(unpack(to_numpy(bufs), mpq), want_radius(db, radius, mpq))
    finally:
        for c in shards:
            c.close()


def test_three_runs_are_byte_identical(ctxs, db):
    q = db["q"]
    for world, k, radius, mpq in ((2, 8, 900.0, None), (8, 2, 1.0e9, None), (4, None, 1.0e9, 1024), (8, None, 900.0, 64)):
        runs = []
        for _ in range(3):
            if mpq is None:
                keys = shard_keys_dev(ctxs[world], q, k=k)
                runs.append((keys.cpu().numpy(),) + merged_knn(ctxs[world][0], keys, radius))
            else:
                keys = shard_keys_dev(ctxs[world], q, radius=radius, mpq=mpq)
                runs.append((keys.cpu().numpy(),) + merged_radius(ctxs[world][0], keys))
        for other in runs[1:]:
            same_bytes(runs[0], other, (world, k, radius, mpq))


# ---------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_outputs_untouched(ctxs, db):
    import torch
    L = capi.lib()
    nq, k, mpq = 8, 4, 4
    one = ctxs[1][0]
    d_q = dev_q(db["q"][:nq])
    kk = torch.full((2, nq, k), 0x1234567, dtype=torch.int64, device="cuda")          # the k-NN pair's keys
    kr = torch.full((2, nq, mpq + 1), 0x1234567, dtype=torch.int64, device="cuda")    # the radius pair's
    cnt, mm, xx, inr = prefilled(nq, mpq)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    inf, nan = float("inf"), float("nan")

    def shard(h=one._h, q_=d_q.data_ptr(), nq_=nq, k_=k, out=kk.data_ptr()):
        return L.todhip_match_l2_shard_device(h, q_, nq_, k_, out)

    def merge(h=one._h, in_=kk.data_ptr(), s_=2, nq_=nq, k_=k, radius=900.0, c_=cnt.data_ptr(), m_=mm.data_ptr(), x_=xx.data_ptr()):
        return L.todhip_merge_l2_shards_device(h, in_, s_, nq_, k_, radius, c_, m_, x_)

    def merge_on(h=one._h, st_=stream.cuda_stream, in_=kk.data_ptr(), s_=2, nq_=nq, k_=k, radius=900.0, c_=cnt.data_ptr(), m_=mm.data_ptr(),
                 x_=xx.data_ptr()):
        return L.todhip_merge_l2_shards_device_on(h, st_, in_, s_, nq_, k_, radius, c_, m_, x_)

    def rshard(h=one._h, q_=d_q.data_ptr(), nq_=nq, radius=900.0, mpq_=mpq, out=kr.data_ptr()):
        return L.todhip_match_l2_radius_shard_device(h, q_, nq_, radius, mpq_, out)

    def rmerge(h=one._h, in_=kr.data_ptr(), s_=2, nq_=nq, mpq_=mpq, c_=cnt.data_ptr(), m_=mm.data_ptr(), x_=xx.data_ptr(), inr_=inr.data_ptr()):
        return L.todhip_merge_l2_radius_shards_device(h, in_, s_, nq_, mpq_, c_, m_, x_, inr_)

    def rmerge_on(h=one._h, st_=stream.cuda_stream, in_=kr.data_ptr(), s_=2, nq_=nq, mpq_=mpq, c_=cnt.data_ptr(), m_=mm.data_ptr(),
                  x_=xx.data_ptr(), inr_=inr.data_ptr()):
        return L.todhip_merge_l2_radius_shards_device_on(h, st_, in_, s_, nq_, mpq_, c_, m_, x_, inr_)

    empty = capi.Context(0)
    rng = np.random.Generator(np.random.PCG64(5))
    binary = capi.Context(0)
    binary.db_load(rng.integers(0, 256, (40, 32), dtype=np.uint8), db["pts"][:40], np.array([0, 10, 40]))
    wide = capi.Context(0)
    wide.db_load(rng.integers(0, 256, (40, 64), dtype=np.uint8), db["pts"][:40], np.array([0, 10, 40]))
    try:
        common = [dict(h=None), dict(nq_=0)]
        for bad in common + [dict(q_=None), dict(out=None), dict(k_=0), dict(k_=9)]:
            assert shard(**bad) == capi.EINVAL, bad
        for bad in common + [dict(q_=None), dict(out=None), dict(mpq_=0), dict(mpq_=1025)] + [dict(radius=r) for r in (0.0, -1.0, inf, nan)]:
            assert rshard(**bad) == capi.EINVAL, bad
        merges = [dict(in_=None), dict(c_=None), dict(m_=None), dict(x_=None), dict(s_=0), dict(s_=65)]
        for bad in common + merges + [dict(k_=0), dict(k_=9)] + [dict(radius=r) for r in (0.0, -1.0, nan)]:
            assert merge(**bad) == capi.EINVAL, bad
            assert merge_on(**bad) == capi.EINVAL, bad
        for bad in common + merges + [dict(mpq_=0), dict(mpq_=1025)]:
            assert rmerge(**bad) == capi.EINVAL, bad
            assert rmerge_on(**bad) == capi.EINVAL, bad
        assert merge_on(st_=None) == capi.EINVAL and rmerge_on(st_=None) == capi.EINVAL
        for fn in (shard, merge, merge_on, rshard, rmerge, rmerge_on):
            assert fn(h=empty._h) == capi.ENODB, fn.__name__
            assert fn(h=binary._h) == capi.EINVAL and fn(h=wide._h) == capi.EINVAL, fn.__name__
        torch.cuda.synchronize()
        assert (kk == 0x1234567).all() and (kr == 0x1234567).all() and (cnt == 77).all() and (mm == SENTINEL).all() and (xx == -7.5).all() and (inr == 78).all()
        # and the same arguments without the fault are served (an infinite radius cuts nothing in the k-NN merge)
        assert shard() == capi.OK
        one.synchronize()
        kk[1] = -1                                                       # a second shard without rows
        torch.cuda.synchronize()
        assert merge() == capi.OK and merge(radius=inf) == capi.OK and merge_on() == capi.OK
        assert rshard() == capi.OK
        one.synchronize()
        kr[1, :, :mpq] = -1
        kr[1, :, mpq] = 0
        torch.cuda.synchronize()
        assert rmerge() == capi.OK and rmerge(inr_=None) == capi.OK and rmerge_on() == capi.OK and rmerge_on(inr_=None) == capi.OK
        one.synchronize()
        stream.synchronize()
    finally:
        for c in (empty, binary, wide):
            c.close()


# ---------------------------------------------------------------------------------------------------- 7. the choreography
def test_sharded_matcher_float_on_rccl_one_rank():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29652", HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, CHILD], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "ok: 12 steps checked" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
