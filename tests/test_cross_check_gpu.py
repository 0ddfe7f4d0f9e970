"""todhip_cross_check_device and todhip_set_cross_check on the GPU. Every comparison is bit for bit against the numpy definition
(tests/cross_check_ref.py) applied to the library's OWN unfiltered output; tests/test_cross_check_cpu.py pins the same inputs on the
reference alone (the filter removes some and keeps some, the index tie decides some), so nothing here passes vacuously."""
import ctypes as C

import numpy as np
import pytest

import cross_check_cases as CC
import cross_check_ref as R

pytestmark = pytest.mark.gpu


class Env:
    def __init__(self):
        import torch
        from tod_amd import capi
        self.torch, self.capi = torch, capi
        self.ctx = {}
        for w in CC.WIDTHS:
            db = CC.make_db(w)
            self.ctx[w] = capi.Context(0)
            self.ctx[w].db_load(db["desc"], db["pts"], db["off"])

    def close(self):
        for c in self.ctx.values():
            c.close()

    def outputs(self, nq, stride):
        """sentinel-filled output tensors (counts, matches, xyz)"""
        t = self.torch
        return (t.full((nq,), 0x5A5A5A5A, dtype=t.int32, device="cuda"), t.full((nq * stride, 4), 0x5A5A5A5A, dtype=t.int32, device="cuda"),
                t.full((nq * stride, 3), 0x5A5A5A5A, dtype=t.int32, device="cuda"))

    def image(self, ctx, out):
        """the three outputs on the host: counts u32, matches DMATCH, xyz as raw u32 [n, 3] (compared as bits)"""
        ctx.synchronize()
        c, m, x = (o.cpu().numpy() for o in out)
        return c.view(np.uint32).copy(), m.view(self.capi.DMATCH_DTYPE).reshape(-1).copy(), x.view(np.uint32).copy()

    def upload(self, a):
        d = self.torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.torch.cuda.synchronize()
        return d


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


def same_filtered(got, before, ref, stride):
    """got: the image after the filter; before: the unfiltered image; ref: R.cross_check's result on `before`"""
    counts, m, x = got
    c0, m0, x0 = before
    assert np.array_equal(counts, ref["counts"])
    slot = np.tile(np.arange(stride), len(counts))
    front = slot < np.repeat(counts, stride)
    assert np.array_equal(m[front], ref["matches"][front]) and np.array_equal(x[front], ref["xyz"].view(np.uint32)[front])
    behind = slot >= np.repeat(np.minimum(c0, stride), stride)           # at or behind the old counts: never written
    assert np.array_equal(m[behind], m0[behind]) and np.array_equal(x[behind], x0[behind])


def filter_and_check(env, ctx, db, q, d_q, Q, stride, out, frame_nq=None):
    """`out` holds an unfiltered output of the library for the queries q: filter it twice, compare with the reference"""
    before = env.image(ctx, out)
    assert before[0].max() <= stride
    ref = R.cross_check(before[0], before[1], before[2].view(np.float32), q, db["desc"], db["off"], Q, stride, frame_nq)
    ptrs = [o.data_ptr() for o in out]
    ctx.cross_check_device(d_q.data_ptr(), len(q), Q, stride, *ptrs, frame_nq=frame_nq)
    once = env.image(ctx, out)
    same_filtered(once, before, ref, stride)
    ctx.cross_check_device(d_q.data_ptr(), len(q), Q, stride, *ptrs, frame_nq=frame_nq)
    twice = env.image(ctx, out)
    assert np.array_equal(twice[0], once[0])                             # idempotent
    same_filtered(twice, before, ref, stride)
    return ref


@pytest.mark.parametrize("Q", CC.SINGLE_FRAMES)
@pytest.mark.parametrize("width", CC.WIDTHS)
def test_single_frame_every_k(env, width, Q):
    ctx, db = env.ctx[width], CC.make_db(width)
    q = CC.make_queries(width, Q)
    d_q = env.upload(q)
    for k in CC.KS:
        out = env.outputs(Q, k)
        ctx.match_device(d_q.data_ptr(), Q, k, CC.RADIUS, *[o.data_ptr() for o in out])
        want = CC.search_ref(db, q, k, CC.RADIUS)
        got = env.image(ctx, out)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])       # the pinned inputs are the library's output
        ref = filter_and_check(env, ctx, db, q, d_q, Q, k, out)
        assert (ref["removed"] > 0) == (Q > 1) and ref["removed"] < ref["total"]


@pytest.mark.parametrize("width", CC.WIDTHS)
def test_frames_and_frame_nq(env, width):
    ctx, db = env.ctx[width], CC.make_db(width)
    f3 = CC.FRAMES3
    q = CC.make_frames3(width)
    d_q = env.upload(q)
    for k in (1, 5):
        out = env.outputs(len(q), k)
        ctx.match_device(d_q.data_ptr(), len(q), k, CC.RADIUS, *[o.data_ptr() for o in out])
        ref = filter_and_check(env, ctx, db, q, d_q, f3["Q"], k, out, f3["frame_nq"])
        assert ref["counts"][33:66].sum() == 0 and ref["counts"][73:].sum() == 0 and ref["counts"][66:73].sum() > 0
    # frames without a frame_nq, a short last frame (33 + 33 + 4); more frames than travel as a kernel argument (70 frames of 1 with a
    # frame_nq, 35 frames of 2 without)
    q = CC.make_queries(width, 70)
    d_q = env.upload(q)
    for Q, frame_nq in ((33, None), (33, [40, 5, 3]), (1, [i % 3 != 1 for i in range(70)]), (2, None), (2, [2, 1, 0] * 11 + [2, 2])):
        out = env.outputs(70, 5)
        ctx.match_device(d_q.data_ptr(), 70, 5, CC.RADIUS, *[o.data_ptr() for o in out])
        filter_and_check(env, ctx, db, q, d_q, Q, 5, out, None if frame_nq is None else np.asarray(frame_nq, np.uint32))


@pytest.mark.parametrize("stride", [64, 1024])
def test_radius_search_strides(env, stride):
    ctx, db = env.ctx[32], CC.make_db(32)
    q = CC.make_queries(32, 70)
    d_q = env.upload(q)
    out = env.outputs(70, stride)
    ctx.match_radius_device(d_q.data_ptr(), 70, CC.RADIUS, stride, *[o.data_ptr() for o in out])
    c0 = env.image(ctx, out)[0]
    assert (c0 == 64).any() if stride == 64 else c0.max() > 64           # a count that equals the stride; more than one compaction chunk
    ref = filter_and_check(env, ctx, db, q, d_q, 70, stride, out)
    assert 0 < ref["removed"] < ref["total"]
    out = env.outputs(70, stride)
    ctx.match_radius_device(d_q.data_ptr(), 70, CC.RADIUS, stride, *[o.data_ptr() for o in out])
    filter_and_check(env, ctx, db, q, d_q, 33, stride, out, np.array([33, 0, 4], np.uint32))


@pytest.mark.parametrize("width", CC.WIDTHS)
def test_setter_equals_match_then_filter(env, width):
    capi, db = env.capi, CC.make_db(width)
    ctx = env.ctx[width]
    q = CC.make_queries(width, 70)
    d_q = env.upload(q)
    plain = capi.Context(0)                                              # a context that never hears of the option
    plain.db_load(db["desc"], db["pts"], db["off"])
    try:
        for k, Q in ((5, 70), (1, 33), (8, 2)):
            out0 = env.outputs(70, k)
            plain.match_device(d_q.data_ptr(), 70, k, CC.RADIUS, *[o.data_ptr() for o in out0])
            before = env.image(plain, out0)
            ref = R.cross_check(before[0], before[1], before[2].view(np.float32), q, db["desc"], db["off"], Q, k)
            assert 0 < ref["removed"] < ref["total"]
            ctx.set_cross_check(Q)
            out = env.outputs(70, k)
            ctx.match_device(d_q.data_ptr(), 70, k, CC.RADIUS, *[o.data_ptr() for o in out])
            same_filtered(env.image(ctx, out), before, ref, k)
            row_ptr, m, xyz = ctx.match(q, k, CC.RADIUS)                 # the host form packs its CSR from the filtered counts
            w_ptr, w_m, w_xyz = R.csr(ref["counts"], ref["matches"], ref["xyz"], k)
            assert np.array_equal(row_ptr, w_ptr) and np.array_equal(m, w_m) and np.array_equal(xyz.view(np.uint32), w_xyz.view(np.uint32))
            ctx.set_cross_check(0)                                       # off again: byte for byte the plain context's outputs
            out = env.outputs(70, k)
            ctx.match_device(d_q.data_ptr(), 70, k, CC.RADIUS, *[o.data_ptr() for o in out])
            for a, b in zip(env.image(ctx, out), before):
                assert np.array_equal(a, b)
            p_ptr, p_m, p_xyz = plain.match(q, k, CC.RADIUS)
            row_ptr, m, xyz = ctx.match(q, k, CC.RADIUS)
            assert np.array_equal(row_ptr, p_ptr) and np.array_equal(m, p_m) and np.array_equal(xyz.view(np.uint32), p_xyz.view(np.uint32))
    finally:
        ctx.set_cross_check(0)
        plain.close()


def test_behind_the_ratio_test_lsh_and_a_selection(env):
    ctx, db = env.ctx[32], CC.make_db(32)
    q = CC.make_queries(32, 70)
    d_q = env.upload(q)

    def run(k=5):
        out = env.outputs(70, k)
        ctx.match_device(d_q.data_ptr(), 70, k, CC.RADIUS, *[o.data_ptr() for o in out])
        ref = filter_and_check(env, ctx, db, q, d_q, 70, k, out)
        assert ref["total"] > 0
        return ref
    try:
        plain = run()
        ctx.set_ratio_test(0.8)
        ratio = run()
        assert ratio["total"] < plain["total"]                           # the filter saw what the ratio test left
        ctx.set_ratio_test(0.0)
        ctx.set_lsh(10, 16, 1)
        run()
        ctx.set_lsh(0)
        ctx.select_objects([3, 4])                                       # the matches name rows of the full DB; the filter reads those
        sel = run()
        assert 0 < sel["total"] < plain["total"]
        ctx.select_objects(None)
    finally:
        ctx.set_ratio_test(0.0)
        ctx.set_lsh(0)
        ctx.select_objects(None)
    # a selection on the 64-byte DB too
    c64, db64 = env.ctx[64], CC.make_db(64)
    q64 = CC.make_queries(64, 70)
    d_q64 = env.upload(q64)
    try:
        c64.select_objects([4, 1])
        out = env.outputs(70, 5)
        c64.match_device(d_q64.data_ptr(), 70, 5, CC.RADIUS, *[o.data_ptr() for o in out])
        assert filter_and_check(env, c64, db64, q64, d_q64, 70, 5, out)["total"] > 0
    finally:
        c64.select_objects(None)


def test_with_a_bit_order_and_on_a_merged_sharded_output(env):
    capi, db = env.capi, CC.make_db(32)
    q = CC.make_queries(32, 70)
    d_q = env.upload(q)
    ordered = capi.Context(0)
    shards = [capi.Context(0) for _ in range(4)]             # object-aligned quarters: ranks 0 and 1 hold the rows, 2 and 3 none
    try:
        ordered.set_db_bit_order(1)
        ordered.db_load(db["desc"], db["pts"], db["off"])
        assert not np.array_equal(ordered.db_bit_order(), np.arange(256))            # the stored rows ARE permuted
        out = env.outputs(70, 5)
        ordered.match_device(d_q.data_ptr(), 70, 5, CC.RADIUS, *[o.data_ptr() for o in out])
        ref = filter_and_check(env, ordered, db, q, d_q, 70, 5, out)
        assert 0 < ref["removed"] < ref["total"]
        ordered.set_cross_check(33)                                                  # and through the setter
        out2 = env.outputs(70, 5)
        ordered.match_device(d_q.data_ptr(), 70, 5, CC.RADIUS, *[o.data_ptr() for o in out2])
        want = CC.search_ref(db, q, 5, CC.RADIUS)
        ref33 = R.cross_check(want[0], want[1], want[2], q, db["desc"], db["off"], 33, 5)
        got = env.image(ordered, out2)
        assert np.array_equal(got[0], ref33["counts"])
        # the two shards that hold rows (and two empty ones), merged on the device, filtered on the context that holds the whole DB
        keys = env.torch.zeros((4, 70, 5), dtype=env.torch.int64, device="cuda")
        for r, c in enumerate(shards):
            c.db_load(db["desc"], db["pts"], db["off"], shard_rank=r, shard_count=4)
            assert (0 < c.db_info()["shard_rows"] < CC.N_ROWS) == (r < 2)
            c.match_shard_device(d_q.data_ptr(), 70, 5, CC.RADIUS, keys[r].data_ptr())
            c.synchronize()
        out = env.outputs(70, 5)
        shards[0].merge_shards_device(keys.data_ptr(), 4, 70, 5, CC.RADIUS, *[o.data_ptr() for o in out])
        shards[0].synchronize()
        merged = env.image(shards[0], out)
        assert np.array_equal(merged[0], want[0]) and np.array_equal(merged[1], want[1])
        # ... which a shard's own context refuses to filter, outputs untouched
        L = capi.lib()
        assert L.todhip_cross_check_device(shards[0]._h, d_q.data_ptr(), 70, 70, None, 5, *[o.data_ptr() for o in out]) == capi.EINVAL
        assert L.todhip_set_cross_check(shards[1]._h, 70) == capi.EINVAL
        for a, b in zip(env.image(shards[0], out), merged):
            assert np.array_equal(a, b)
        ref = filter_and_check(env, env.ctx[32], db, q, d_q, 70, 5, out)
        assert 0 < ref["removed"] < ref["total"]
    finally:
        ordered.close()
        for c in shards:
            c.close()


def test_refusals_leave_the_outputs_untouched(env):
    capi, L = env.capi, env.capi.lib()
    ctx, db = env.ctx[32], CC.make_db(32)
    q = CC.make_queries(32, 33)
    d_q = env.upload(q)
    out = env.outputs(33, 5)
    ctx.match_device(d_q.data_ptr(), 33, 5, CC.RADIUS, *[o.data_ptr() for o in out])
    before = env.image(ctx, out)
    p = [o.data_ptr() for o in out]

    def call(h=ctx._h, dq=d_q.data_ptr(), nq=33, Q=33, stride=5, c=p[0], m=p[1], x=p[2]):
        return L.todhip_cross_check_device(h, dq, nq, Q, None, stride, c, m, x)
    for bad in (dict(h=None), dict(dq=None), dict(c=None), dict(m=None), dict(x=None), dict(nq=0), dict(Q=0), dict(stride=0), dict(stride=1025)):
        assert call(**bad) == capi.EINVAL, bad
    empty = capi.Context(0)
    flt = capi.Context(0)
    try:
        assert call(h=empty._h) == capi.ENODB
        assert L.todhip_set_cross_check(empty._h, 33) == capi.OK                       # nothing loaded yet: nothing to object to
        rng = np.random.Generator(np.random.PCG64(3))
        flt.db_load(rng.standard_normal((40, 128)).astype(np.float32), db["pts"][:40], np.array([0, 40], np.uint32))
        assert call(h=flt._h) == capi.EINVAL                                            # a float DB
        assert L.todhip_set_cross_check(flt._h, 33) == capi.EINVAL and L.todhip_set_cross_check(flt._h, 0) == capi.OK
        # the refused setter changed nothing: set 33, reload as one shard of four (refused: 7), reload whole -- frames of 33 still
        c = empty
        c.db_load(db["desc"], db["pts"], db["off"], shard_rank=1, shard_count=4)
        assert 0 < c.db_info()["shard_rows"] < CC.N_ROWS
        assert L.todhip_set_cross_check(c._h, 7) == capi.EINVAL
        c.db_load(db["desc"], db["pts"], db["off"])
        out2 = env.outputs(33, 5)
        c.match_device(d_q.data_ptr(), 33, 5, CC.RADIUS, *[o.data_ptr() for o in out2])
        ref = R.cross_check(before[0], before[1], before[2].view(np.float32), q, db["desc"], db["off"], 33, 5)
        ref7 = R.cross_check(before[0], before[1], before[2].view(np.float32), q, db["desc"], db["off"], 7, 5)
        assert not np.array_equal(ref["counts"], ref7["counts"])
        assert np.array_equal(env.image(c, out2)[0], ref["counts"])
    finally:
        empty.close()
        flt.close()
    for a, b in zip(env.image(ctx, out), before):
        assert np.array_equal(a, b)
