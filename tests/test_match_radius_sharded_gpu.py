"""todhip_match_radius_shard_device + todhip_merge_radius_shards_device[_on] on the GPU: one context per shard on device 0
(db_load(shard_rank, shard_count)) plus an unsharded context. What a shard sends equals the numpy definition
(tests/sharded_radius_ref.py) in every slot; what the merge leaves equals what todhip_match_radius_device leaves on the unsharded
context, byte for byte over whole prefilled buffers, and the numpy definition.

The DB (sharded_radius_ref.make_db) is the smallest on which the pair can go wrong: objects short of, on and past a 32-row step, an
empty one, shards without rows (world 8), 300 copies of one row across the boundary at row 590 (195 + 105: more than a shard's
candidate buffer holds at max_per_query <= 32 / 64, so the keys come out of the ordered rescan). Worlds 4 and 8 at max_per_query
1024 are 4096 keys per query (the merge's staged form, full) and 8192 (its global form); max_per_query 1 and 5 put up to 256 and
25 queries into one workgroup, with a ragged last one at 33 queries and 3 x 5 elements that do not divide 256."""
import os
import subprocess
import sys

import numpy as np
import pytest

import match_radius_ref as R
import sharded_radius_ref as S
from tod_amd import capi, sharded

pytestmark = pytest.mark.gpu

WORLDS = (1, 2, 3, 4, 8)
RADII = (1, 35, 127, 128, 256, 1000)
MPQS = (1, 5, 64, 1024)
FIELDS = ("queryIdx", "trainIdx", "imgIdx", "distance")
SENTINEL = 0x5A5A5A5A
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sharded_radius_gpu_child.py")


def load(desc, off, pts, rank=0, world=1, stream=None, bit_order=False):
    c = capi.Context(0, stream)
    if bit_order:
        c.set_db_bit_order(1)
    c.db_load(desc, pts, off, shard_rank=rank, shard_count=world)
    return c


@pytest.fixture(scope="module")
def db():
    return S.make_db()


@pytest.fixture(scope="module")
def ctxs(db):
    """{world: its shard contexts}; world 1's only context is the unsharded one"""
    desc, off, pts, _ = db
    out = {w: [load(desc, off, pts, r, w) for r in range(w)] for w in WORLDS}
    for w in WORLDS:
        assert [c.db_info()["shard_rows"] for c in out[w]] == [hi - lo for _, _, lo, hi in (sharded.shard_bounds(off, r, w) for r in range(w))]
    yield out
    for cs in out.values():
        for c in cs:
            c.close()


def shard_rows(off, world, sel=None):
    """per shard: the searched rows (under a selection of objects, when given)"""
    keep = np.ones(int(off[-1]), bool)
    if sel is not None:
        keep[:] = False
        for o in sel:
            keep[int(off[o]):int(off[o + 1])] = True
    return [np.arange(lo, hi)[keep[lo:hi]] for _, _, lo, hi in (sharded.shard_bounds(off, r, world) for r in range(world))]


def prefilled(nq, mpq):
    import torch
    return (torch.full((nq,), 77, dtype=torch.int32, device="cuda"), torch.full((nq * mpq, 4), SENTINEL, dtype=torch.int32, device="cuda"),
            torch.full((nq * mpq, 3), -7.5, dtype=torch.float32, device="cuda"), torch.full((nq,), 78, dtype=torch.int32, device="cuda"))


def to_numpy(bufs):
    return tuple(b.cpu().numpy() for b in bufs)


def unsharded_raw(c, q, radius, mpq):
    import torch
    d_q = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    bufs = prefilled(len(q), mpq)
    torch.cuda.synchronize()
    c.match_radius_device(d_q.data_ptr(), len(q), radius, mpq, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr())
    c.synchronize()
    return to_numpy(bufs)


def shard_keys_dev(shards, q, radius, mpq):
    """the shards' answers as one device tensor i64[n_shards, nq, mpq + 1], prefilled so that an unwritten slot shows"""
    import torch
    d_q = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    keys = torch.full((len(shards), len(q), mpq + 1), 0x1234567, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for s, c in enumerate(shards):
        c.match_radius_shard_device(d_q.data_ptr(), len(q), radius, mpq, keys[s].data_ptr())
    for c in shards:
        c.synchronize()
    return keys


def merged_raw(c, keys, mpq, with_in_radius=True):
    n_shards, nq, _ = keys.shape
    bufs = prefilled(nq, mpq)
    import torch
    torch.cuda.synchronize()
    c.merge_radius_shards_device(keys.data_ptr(), n_shards, nq, mpq, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
                                 bufs[3].data_ptr() if with_in_radius else None)
    c.synchronize()
    return to_numpy(bufs)


def unpack(raw, mpq):
    """whole fixed-stride buffers -> (row_ptr, matches, xyz, in_radius); the slots behind counts[q] must hold the prefill"""
    cnt, mm, xx, inr = raw
    nq = len(cnt)
    cnt = cnt.astype(np.int64)
    keep = np.arange(mpq)[None, :] < cnt[:, None]
    assert (mm.reshape(nq, mpq, 4)[~keep] == SENTINEL).all() and (xx.reshape(nq, mpq, 3)[~keep] == -7.5).all(), "slots behind counts[q] were written"
    return (np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32), mm.view(capi.DMATCH_DTYPE).reshape(nq, mpq)[keep],
            xx.reshape(nq, mpq, 3)[keep], inr.astype(np.uint32))


def same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), what
    for f in FIELDS:
        assert np.array_equal(got[1][f], want[1][f]), (what, f)
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), what


def same_bytes(a, b, what=""):
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes(), what


def prefix(want, nq):
    n = int(want[0][nq])
    return want[0][:nq + 1], want[1][:n], want[2][:n], want[3][:nq]


_WANT = {}


def want_of(db, world, radius, mpq):
    """the numpy definition for all 33 queries, once per case: (the shards' keys, the unsharded answer); every nq is a prefix"""
    key = (world, radius, mpq)
    if key not in _WANT:
        desc, off, pts, q = db
        if (radius, mpq) not in _WANT:
            _WANT[(radius, mpq)] = R.match_radius(desc, off, pts, q, radius, mpq)
        _WANT[key] = (np.stack([S.shard_keys(desc, off, pts, q, radius, mpq, r) for r in shard_rows(off, world)]), _WANT[(radius, mpq)])
    return _WANT[key]


@pytest.mark.parametrize("nq", [1, 32, 33])
@pytest.mark.parametrize("world", WORLDS)
def test_shard_keys_and_merge_equal_the_definition_and_the_unsharded_call(ctxs, db, world, nq):
    q = db[3][:nq]
    one = ctxs[1][0]
    n_over = n_rescan = 0
    for radius in RADII:
        for mpq in MPQS:
            what = (world, nq, radius, mpq)
            want_keys, want = want_of(db, world, radius, mpq)
            keys = shard_keys_dev(ctxs[world], q, radius, mpq)
            assert np.array_equal(keys.cpu().numpy().view(np.uint64), want_keys[:, :nq]), what      # every slot: keys, padding, count
            got = merged_raw(ctxs[world][-1], keys, mpq)
            same_bytes(got, unsharded_raw(one, q, radius, mpq), what)
            same(unpack(got, mpq), prefix(want, nq), what)
            n_over += int((want[3][:nq] > mpq).sum())
            n_rescan += int((want_keys[:, :nq, mpq] > capi.radius_capacity(mpq)).sum())
    assert n_over > 0 and n_rescan > 0


def test_in_radius_may_be_null(ctxs, db):
    q = db[3]
    keys = shard_keys_dev(ctxs[3], q, 35, 5)
    got = merged_raw(ctxs[3][0], keys, 5, with_in_radius=False)
    assert (got[3] == 78).all()
    same_bytes(got[:3], merged_raw(ctxs[3][0], keys, 5)[:3])


def test_merge_on_a_second_stream_equals_the_plain_form(db):
    import torch
    desc, off, pts, q = db
    compute, comm = torch.cuda.Stream(), torch.cuda.Stream()
    shards = [load(desc, off, pts, r, 2, stream=compute.cuda_stream) for r in range(2)]
    try:
        for radius, mpq in ((35, 5), (256, 1024)):
            d_q = torch.from_numpy(q).cuda()
            keys = torch.zeros((2, len(q), mpq + 1), dtype=torch.int64, device="cuda")
            bufs = prefilled(len(q), mpq)
            torch.cuda.synchronize()
            for s, c in enumerate(shards):
                c.match_radius_shard_device(d_q.data_ptr(), len(q), radius, mpq, keys[s].data_ptr())
            ev = torch.cuda.Event()
            ev.record(compute)
            comm.wait_event(ev)
            shards[0].merge_radius_shards_device_on(comm.cuda_stream, keys.data_ptr(), 2, len(q), mpq, bufs[0].data_ptr(), bufs[1].data_ptr(),
                                                    bufs[2].data_ptr(), bufs[3].data_ptr())
            comm.synchronize()
            same_bytes(to_numpy(bufs), merged_raw(shards[1], keys, mpq), (radius, mpq))
            same(unpack(to_numpy(bufs), mpq), R.match_radius(desc, off, pts, q, radius, mpq), (radius, mpq))
    finally:
        for c in shards:
            c.close()


def test_three_runs_are_byte_identical(ctxs, db):
    q = db[3]
    for world, radius, mpq in ((2, 1, 5), (4, 256, 1024), (8, 128, 64)):
        runs = []
        for _ in range(3):
            keys = shard_keys_dev(ctxs[world], q, radius, mpq)
            runs.append((keys.cpu().numpy(),) + merged_raw(ctxs[world][0], keys, mpq))
        for other in runs[1:]:
            same_bytes(runs[0], other, (world, radius, mpq))


@pytest.mark.parametrize("sel", [[7, 3, 0], []], ids=["three-objects", "nothing"])
def test_selection_on_every_shard(ctxs, db, sel):
    desc, off, pts, q = db
    one = ctxs[1][0]
    try:
        for world in (2, 3, 8):
            for c in ctxs[world] + [one]:
                c.select_objects(sel)
            rows = shard_rows(off, world, sel)
            for radius, mpq in ((35, 5), (256, 64), (256, 1024)):
                keys = shard_keys_dev(ctxs[world], q, radius, mpq)
                want_keys = np.stack([S.shard_keys(desc, off, pts, q, radius, mpq, r) for r in rows])
                assert np.array_equal(keys.cpu().numpy().view(np.uint64), want_keys), (world, radius, mpq)
                got = merged_raw(ctxs[world][0], keys, mpq)
                same_bytes(got, unsharded_raw(one, q, radius, mpq), (world, radius, mpq))
                want = R.match_radius(desc, off, pts, q, radius, mpq, rows=np.concatenate(rows))
                same(unpack(got, mpq), want, (world, radius, mpq))
                if not sel:
                    assert not got[0].any() and not got[3].any() and (want_keys[:, :, :mpq] == S.PAD).all()
    finally:
        for cs in ctxs.values():
            for c in cs:
                c.select_objects(None)


def test_bit_order_ratio_test_and_lsh_change_nothing(ctxs, db):
    desc, off, pts, q = db
    desc = desc.copy()
    desc[:, :8] &= np.random.Generator(np.random.PCG64(3)).integers(0, 256, (len(desc), 8), dtype=np.uint8)   # biased leading bits
    desc[S.TIE_ROWS] = desc[100]
    q = S.make_queries(desc, S.NQ, 8)
    shards = [load(desc, off, pts, r, 3, bit_order=True) for r in range(3)]
    one = load(desc, off, pts)
    try:
        assert any(not np.array_equal(c.db_bit_order(), np.arange(256)) for c in shards)
        cases = ((35, 5), (100, 64), (256, 1024))
        first = {}
        for k in cases:
            keys = shard_keys_dev(shards, q, *k)
            first[k] = (keys.cpu().numpy(),) + merged_raw(shards[0], keys, k[1])
            same_bytes(first[k][1:], unsharded_raw(one, q, *k), ("bit order", k))
            same(unpack(first[k][1:], k[1]), R.match_radius(desc, off, pts, q, *k), ("bit order", k))
        for c in shards:
            c.set_ratio_test(0.8)
            c.set_lsh(10, 16, 1)
        for k in cases:
            keys = shard_keys_dev(shards, q, *k)
            same_bytes((keys.cpu().numpy(),) + merged_raw(shards[0], keys, k[1]), first[k], ("ratio + lsh", k))
    finally:
        for c in shards + [one]:
            c.close()


def test_many_tiles_many_queries_eight_shards():
    """70 000 random rows x 1 100 queries, radius 100, 64 per query, world 8: several tiles per shard and six query blocks per wave in
    the DB pass, 275 workgroups in the merge; against the unsharded context"""
    rng = np.random.Generator(np.random.PCG64(5))
    n, nq, radius, mpq = 70000, 1100, 100, 64
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    pts = rng.standard_normal((n, 3)).astype(np.float32)
    off = np.arange(0, n + 1, 1000, dtype=np.uint32)
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    q[::3] = desc[rng.integers(0, n, len(q[::3]))]
    q[::3, 5] ^= 0x81
    shards = [load(desc, off, pts, r, 8) for r in range(8)]
    one = load(desc, off, pts)
    try:
        keys = shard_keys_dev(shards, q, radius, mpq)
        got = merged_raw(shards[3], keys, mpq)
        want = unsharded_raw(one, q, radius, mpq)
    finally:
        for c in shards + [one]:
            c.close()
    same_bytes(got, want)
    k = keys.cpu().numpy().view(np.uint64)
    assert np.array_equal(k[:, :, mpq].sum(axis=0), want[3].astype(np.uint64)) and want[3][::3].min() >= 1 and want[3].max() > 8
    real = k[:, :, :mpq] != S.PAD
    assert np.array_equal(real.sum(axis=2), np.minimum(k[:, :, mpq], mpq)) and (np.diff(k[:, :, :mpq].astype(np.float64), axis=2) >= 0).all()


def test_refusals(ctxs, db):
    import torch
    L = capi.lib()
    desc, off, pts, q = db
    nq, mpq = 8, 4
    one = ctxs[1][0]
    d_q = torch.from_numpy(np.ascontiguousarray(q[:nq])).cuda()
    keys = torch.zeros((2, nq, mpq + 1), dtype=torch.int64, device="cuda")
    cnt, mm, xx, inr = prefilled(nq, mpq)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()

    def shard(h=one._h, q_=d_q.data_ptr(), nq_=nq, radius=35, mpq_=mpq, k_=keys.data_ptr()):
        return L.todhip_match_radius_shard_device(h, q_, nq_, radius, mpq_, k_)

    def merge(h=one._h, k_=keys.data_ptr(), s_=2, nq_=nq, mpq_=mpq, c_=cnt.data_ptr(), m_=mm.data_ptr(), x_=xx.data_ptr(), in_=inr.data_ptr()):
        return L.todhip_merge_radius_shards_device(h, k_, s_, nq_, mpq_, c_, m_, x_, in_)

    def merge_on(h=one._h, st_=stream.cuda_stream, k_=keys.data_ptr(), s_=2, nq_=nq, mpq_=mpq, c_=cnt.data_ptr(), m_=mm.data_ptr(),
                 x_=xx.data_ptr(), in_=inr.data_ptr()):
        return L.todhip_merge_radius_shards_device_on(h, st_, k_, s_, nq_, mpq_, c_, m_, x_, in_)

    assert shard() == capi.OK and shard(k_=keys[1].data_ptr()) == capi.OK
    one.synchronize()
    keys[1, :, :mpq] = -1                                               # a second shard without rows
    keys[1, :, mpq] = 0
    torch.cuda.synchronize()
    assert merge() == capi.OK and merge(in_=None) == capi.OK and merge_on() == capi.OK and merge_on(in_=None) == capi.OK
    one.synchronize()
    stream.synchronize()
    for bad in (dict(h=None), dict(q_=None), dict(k_=None), dict(nq_=0), dict(radius=0), dict(mpq_=0), dict(mpq_=1025)):
        assert shard(**bad) == capi.EINVAL, bad
    for bad in (dict(h=None), dict(k_=None), dict(c_=None), dict(m_=None), dict(x_=None), dict(nq_=0), dict(s_=0), dict(s_=65), dict(mpq_=0),
                dict(mpq_=1025)):
        assert merge(**bad) == capi.EINVAL, bad
        assert merge_on(**bad) == capi.EINVAL, bad
    assert merge_on(st_=None) == capi.EINVAL
    empty = capi.Context(0)
    assert shard(h=empty._h) == capi.ENODB and merge(h=empty._h) == capi.ENODB and merge_on(h=empty._h) == capi.ENODB
    empty.close()
    rng = np.random.Generator(np.random.PCG64(5))
    fl = capi.Context(0)
    fl.db_load(rng.standard_normal((40, 128)).astype(np.float32), pts[:40], np.array([0, 10, 40]))
    wide = capi.Context(0)
    wide.db_load(rng.integers(0, 256, (40, 64), dtype=np.uint8), pts[:40], np.array([0, 10, 40]))
    for c in (fl, wide):
        assert shard(h=c._h) == capi.EINVAL and merge(h=c._h) == capi.EINVAL and merge_on(h=c._h) == capi.EINVAL
        c.close()


def test_sharded_matcher_radius_on_rccl_one_rank():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29651", HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, CHILD], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "ok: 16 steps checked" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
