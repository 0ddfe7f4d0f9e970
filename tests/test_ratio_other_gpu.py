"""todhip_other_object_min_device, todhip_ratio_other_apply_device, todhip_ratio_other_device and todhip_set_ratio_test_other on the
GPU. Every comparison is bit for bit against the numpy definition (tests/ratio_other_ref.py) -- the filter's on the library's OWN
unfiltered output; tests/test_ratio_other_cpu.py pins the same inputs on the reference alone (the planted equalities, confusers at
lo - 1 and hi, duplicates at lo and hi - 1, ratios that drop some and keep some), so nothing here passes vacuously."""
import numpy as np
import pytest

import cross_check_ref as XR
import ratio_other_cases as RC
import ratio_other_ref as R

pytestmark = pytest.mark.gpu

NONE = R.NONE
_tables = {}


def table(width, nq):
    """(queries, their complete distance table), computed once"""
    if (width, nq) not in _tables:
        q = RC.make_queries(width, nq)
        _tables[(width, nq)] = (q, R.hamming(q, RC.make_db(width)["desc"]))
    return _tables[(width, nq)]


class Env:
    def __init__(self):
        import torch
        from tod_amd import capi
        self.torch, self.capi = torch, capi
        self.ctx = {}
        for w in RC.WIDTHS:
            self.ctx[w] = self.context(w)

    def context(self, width, db=None, **load):
        db = db or RC.make_db(width)
        c = self.capi.Context(0)
        c.db_load(db["desc"], db["pts"], db["off"], **load)
        return c

    def close(self):
        for c in self.ctx.values():
            c.close()

    def outputs(self, nq, stride):
        """sentinel-filled output tensors (counts, matches, xyz)"""
        t = self.torch
        return (t.full((nq,), RC.SENTINEL, dtype=t.int32, device="cuda"), t.full((nq * stride, 4), RC.SENTINEL, dtype=t.int32, device="cuda"),
                t.full((nq * stride, 3), RC.SENTINEL, dtype=t.int32, device="cuda"))

    def words(self, n, fill=RC.SENTINEL):
        return self.torch.full((n,), fill, dtype=self.torch.int32, device="cuda")

    def image(self, ctx, out):
        """the three outputs on the host: counts u32, matches DMATCH, xyz as raw u32 [n, 3] (compared as bits)"""
        ctx.synchronize()
        c, m, x = (o.cpu().numpy() for o in out)
        return c.view(np.uint32).copy(), m.view(self.capi.DMATCH_DTYPE).reshape(-1).copy(), x.view(np.uint32).copy()

    def upload(self, a):
        a = np.ascontiguousarray(a)
        d = self.torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
        self.torch.cuda.synchronize()
        return d

    def other_min(self, ctx, d_q, nq, excl, limit=None, cap=NONE):
        """the primitive on a sentinel-filled output, back on the host"""
        d_excl = self.upload(np.asarray(excl, np.int64).astype(np.uint32))
        d_lim = None if limit is None else self.upload(np.asarray(limit, np.uint32))
        d_min = self.words(nq + 8)                                        # eight words behind the output: never written
        ctx.other_object_min_device(d_q.data_ptr(), nq, d_excl.data_ptr(), d_min.data_ptr(), None if d_lim is None else d_lim.data_ptr(), cap)
        ctx.synchronize()
        got = d_min.cpu().numpy().view(np.uint32)
        assert (got[nq:] == RC.SENTINEL).all()
        return got[:nq].copy()


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


def nearest_object(D, off):
    """the object of every query's nearest row in the order (distance, row)"""
    return R.row_objects(off)[np.argmin(D, axis=1)]


# ---------------------------------------------------------------- the primitive

@pytest.mark.parametrize("nq", RC.NQS)
@pytest.mark.parametrize("width", RC.WIDTHS)
def test_primitive_exact_minimum(env, width, nq):
    """d_limit NULL, cap NONE: the exact minimum, the form for thresholds of either sign"""
    ctx, db = env.ctx[width], RC.make_db(width)
    q, D = table(width, nq)
    d_q = env.upload(q)
    own = nearest_object(D, db["off"])
    mixed = np.where(np.arange(nq) % 3 == 0, NONE, np.where(np.arange(nq) % 3 == 1, own, (np.arange(nq) * 5) % 8))
    for excl in (own, mixed, np.full(nq, NONE), np.full(nq, 5), np.full(nq, 0), np.full(nq, 1000)):   # 0: the empty object; 1000: none
        want = R.other_min(D, db["off"], excl)
        assert (want != NONE).all()
        assert np.array_equal(env.other_min(ctx, d_q, nq, excl), want)
    assert np.array_equal(R.other_min(D, db["off"], np.full(nq, 0)), D.min(axis=1))


@pytest.mark.parametrize("width", RC.WIDTHS)
def test_primitive_limits_and_caps(env, width):
    ctx, db, bits = env.ctx[width], RC.make_db(width), 8 * width
    nq = 70
    q, D = table(width, nq)
    d_q = env.upload(q)
    own = nearest_object(D, db["off"])
    exact = R.other(D, db["off"], own).astype(np.int64)
    i = np.arange(nq)
    # per-query limits on both sides of the true value, at it, one beside it, 0 and none
    lim = np.select([i % 6 == 0, i % 6 == 1, i % 6 == 2, i % 6 == 3, i % 6 == 4], [exact + 3, np.maximum(exact, 2) - 2, exact, exact + 1, 0], NONE)
    want = R.other_min(D, db["off"], own, lim)
    assert (want < exact).any() and (want == exact).any() and (want == 0).any()
    for cap in (NONE, bits // 2, bits // 2 + 1, 6, 0):                   # bits / 2: the last cap of the non-negative-threshold form
        assert np.array_equal(env.other_min(ctx, d_q, nq, own, lim, cap), R.other_min(D, db["off"], own, lim, cap)), cap
        assert np.array_equal(env.other_min(ctx, d_q, nq, own, None, cap), R.other_min(D, db["off"], own, None, cap)), cap
    # a cap that cuts: queries of the cluster without a confuser have their other object ~bits / 2 away
    far = R.other_min(D, db["off"], np.full(nq, 3))
    assert (far > 12).any() and np.array_equal(env.other_min(ctx, d_q, nq, np.full(nq, 3), None, 12), np.minimum(far, 12))


@pytest.mark.parametrize("width", RC.WIDTHS)
def test_primitive_under_selections(env, width):
    ctx, db, bits = env.ctx[width], RC.make_db(width), 8 * width
    nq = 70
    q, D = table(width, nq)
    d_q = env.upload(q)
    own = nearest_object(D, db["off"])
    try:
        # the two tiny objects: 6 random-looking rows, minima above bits / 2 for the queries that exclude the nearer one
        for sel, excls in (([1, 6], (np.full(nq, 6), np.full(nq, 1), own, np.full(nq, NONE))),     # own: mostly objects that are not selected
                           ([5], (np.full(nq, 5), np.full(nq, 2))),                                   # one object: NONE when it is excluded
                           ([0], (own,)), ([], (own,)),                                               # the empty object; nothing
                           ([7, 2, 4], (own, np.full(nq, 4)))):
            ctx.select_objects(sel)
            mask = R.searched_mask(db["off"], selection=sel)
            for excl in excls:
                want = R.other_min(D, db["off"], excl, searched=mask)
                assert np.array_equal(env.other_min(ctx, d_q, nq, excl), want), sel
                lim = np.where(np.arange(nq) % 2 == 0, 7, NONE)
                assert np.array_equal(env.other_min(ctx, d_q, nq, excl, lim, bits // 2), R.other_min(D, db["off"], excl, lim, bits // 2, mask)), sel
        ctx.select_objects([1, 6])
        big = env.other_min(ctx, d_q, nq, np.full(nq, 6))
        assert (big > bits // 2).any()                                    # a distance only the form for negative thresholds finds
        ctx.select_objects([5])
        assert (env.other_min(ctx, d_q, nq, np.full(nq, 5)) == NONE).all()
        ctx.select_objects([])
        assert (env.other_min(ctx, d_q, nq, own) == NONE).all()
    finally:
        ctx.select_objects(None)
    assert np.array_equal(env.other_min(ctx, d_q, nq, own), R.other(D, db["off"], own))


# ---------------------------------------------------------------- the filter

def filter_and_check(env, ctx, q, d_q, stride, out, ratio, D, off, searched=None):
    """`out` holds an unfiltered output of the library: filter it, compare the counts with the reference; nothing else may change"""
    before = env.image(ctx, out)
    assert before[0].max() <= stride
    ref = R.ratio_other(before[0], before[1], stride, ratio, D, off, searched)
    ctx.ratio_other_device(d_q.data_ptr(), len(q), ratio, stride, out[0].data_ptr(), out[1].data_ptr())
    got = env.image(ctx, out)
    assert np.array_equal(got[0], ref["counts"])
    assert np.array_equal(got[1], before[1]) and np.array_equal(got[2], before[2])       # matches and xyz: not a byte
    return ref, before


@pytest.mark.parametrize("nq", RC.NQS)
@pytest.mark.parametrize("width", RC.WIDTHS)
def test_filter_every_ratio(env, width, nq):
    ctx, db = env.ctx[width], RC.make_db(width)
    q, D = table(width, nq)
    d_q = env.upload(q)
    want = RC.search_ref(db, q, 2, 35, D=D)
    for ratio in RC.RATIOS:
        out = env.outputs(nq, 2)
        ctx.match_device(d_q.data_ptr(), nq, 2, 35, *[o.data_ptr() for o in out])
        ref, before = filter_and_check(env, ctx, q, d_q, 2, out, ratio, D, db["off"])
        assert np.array_equal(before[0], want[0])                                         # the pinned inputs are the library's output
        if nq >= 33:
            assert ref["dropped"] > 0 and ref["kept"] > 0
            d1 = before[1].reshape(nq, 2)[:, 0]["distance"]
            assert (d1[0], ref["other"][0]) == (4, 8) and (d1[1], ref["other"][1]) == (4, 9) and (d1[2], ref["other"][2]) == (6, 8)
            assert (ref["counts"][0] > 0) == (ratio > 0.5) and ref["counts"][1] > 0 and (ref["counts"][2] > 0) == (ratio > 0.75)


@pytest.mark.parametrize("width", RC.WIDTHS)
def test_single_object_db_everything_survives(env, width):
    one = RC.single_object_db(width)
    ctx = env.context(width, one)
    try:
        q, _ = table(width, 70)
        d_q = env.upload(q)
        out = env.outputs(70, 2)
        ctx.match_device(d_q.data_ptr(), 70, 2, 8 * width, *[o.data_ptr() for o in out])
        before = env.image(ctx, out)
        assert (before[0] == 2).all()
        ctx.ratio_other_device(d_q.data_ptr(), 70, 0.5, 2, out[0].data_ptr(), out[1].data_ptr())
        for a, b in zip(env.image(ctx, out), before):
            assert np.array_equal(a, b)
        assert (env.other_min(ctx, d_q, 70, np.zeros(70)) == NONE).all()
    finally:
        ctx.close()


@pytest.mark.parametrize("width", RC.WIDTHS)
def test_behind_match_device_and_the_radius_search(env, width):
    ctx, db, bits = env.ctx[width], RC.make_db(width), 8 * width
    nq = 70
    q, D = table(width, nq)
    d_q = env.upload(q)
    for k in (1, 2, 8):
        for radius in (35, bits):
            out = env.outputs(nq, k)
            ctx.match_device(d_q.data_ptr(), nq, k, radius, *[o.data_ptr() for o in out])
            ref, _ = filter_and_check(env, ctx, q, d_q, k, out, 0.8, D, db["off"])
            assert ref["dropped"] > 0 and ref["kept"] > 0
    if width == 32:                                                                       # the radius search serves 32-byte rows
        for mpq in (5, 64):
            out = env.outputs(nq, mpq)
            ctx.match_radius_device(d_q.data_ptr(), nq, 35, mpq, *[o.data_ptr() for o in out])
            ref, _ = filter_and_check(env, ctx, q, d_q, mpq, out, 0.75, D, db["off"])
            assert ref["dropped"] > 0 and ref["kept"] > 0
    # a query without a kept match is left alone (radius 2: most queries keep nothing), a count above 0 with an empty... stays a count
    out = env.outputs(nq, 2)
    ctx.match_device(d_q.data_ptr(), nq, 2, 2, *[o.data_ptr() for o in out])
    ref, before = filter_and_check(env, ctx, q, d_q, 2, out, 0.5, D, db["off"])
    assert (before[0] == 0).any() and ref["kept"] > 0


def same_image(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("width", RC.WIDTHS)
def test_setter_order_host_form_and_off(env, width):
    capi, db = env.capi, RC.make_db(width)
    ctx = env.ctx[width]
    nq = 70
    q, D = table(width, nq)
    d_q = env.upload(q)
    plain = env.context(width)                                           # a context that never hears of the setter
    try:
        for k, radius, classic, Q in ((2, 35, 0.0, 0), (1, 35, 0.0, 0), (8, 8 * width, 0.0, 0), (5, 35, 0.9, 0), (5, 35, 0.0, 70), (2, 35, 0.9, 33)):
            plain.set_ratio_test(classic)
            ctx.set_ratio_test(classic)
            out0 = env.outputs(nq, k)
            plain.match_device(d_q.data_ptr(), nq, k, radius, *[o.data_ptr() for o in out0])
            before = env.image(plain, out0)
            ref = R.ratio_other(before[0], before[1], k, 0.8, D, db["off"])
            assert ref["dropped"] > 0 and ref["kept"] > 0
            want = (ref["counts"], before[1], before[2])
            if Q:                                                        # the cross-check sees what this filter left, not the reverse
                x = XR.cross_check(ref["counts"], before[1], before[2].view(np.float32), q, db["desc"], db["off"], Q, k)
                assert 0 < x["removed"] and x["counts"].sum() > 0
                want = (x["counts"], x["matches"], x["xyz"].view(np.uint32))
            ctx.set_ratio_test_other(0.8)
            ctx.set_cross_check(Q)
            out = env.outputs(nq, k)
            ctx.match_device(d_q.data_ptr(), nq, k, radius, *[o.data_ptr() for o in out])
            got = env.image(ctx, out)
            assert np.array_equal(got[0], want[0])
            slot = np.tile(np.arange(k), nq)
            front = slot < np.repeat(got[0], k)
            assert np.array_equal(got[1][front], want[1][front]) and np.array_equal(got[2][front], want[2][front])
            behind = slot >= np.repeat(np.minimum(before[0], k), k)      # at or behind the old counts: the sentinel still
            assert np.array_equal(got[1][behind], before[1][behind]) and np.array_equal(got[2][behind], before[2][behind])
            assert (got[1][behind].view(np.uint32) == RC.SENTINEL).all()
            row_ptr, m, xyz = ctx.match(q, k, radius)                    # the host form packs its CSR from the filtered counts
            w_ptr, w_m, w_xyz = XR.csr(want[0], want[1], want[2].view(np.float32), k)
            assert np.array_equal(row_ptr, w_ptr) and np.array_equal(m, w_m) and np.array_equal(xyz.view(np.uint32), w_xyz.view(np.uint32))
            ctx.set_ratio_test_other(0.0)                                # off again: byte for byte the plain context's outputs
            ctx.set_cross_check(0)
            out = env.outputs(nq, k)
            ctx.match_device(d_q.data_ptr(), nq, k, radius, *[o.data_ptr() for o in out])
            same_image(env.image(ctx, out), before)
            p_ptr, p_m, p_xyz = plain.match(q, k, radius)
            row_ptr, m, xyz = ctx.match(q, k, radius)
            assert np.array_equal(row_ptr, p_ptr) and np.array_equal(m, p_m) and np.array_equal(xyz.view(np.uint32), p_xyz.view(np.uint32))
    finally:
        ctx.set_ratio_test_other(0.0)
        ctx.set_cross_check(0)
        ctx.set_ratio_test(0.0)
        plain.close()


@pytest.mark.parametrize("width", RC.WIDTHS)
def test_filter_under_selections(env, width):
    ctx, db = env.ctx[width], RC.make_db(width)
    nq = 70
    q, D = table(width, nq)
    d_q = env.upload(q)
    try:
        for sel in ([2, 5, 7], [5], [], [1, 2, 3]):
            ctx.select_objects(sel)
            mask = R.searched_mask(db["off"], selection=sel)
            out = env.outputs(nq, 2)
            ctx.match_device(d_q.data_ptr(), nq, 2, 35, *[o.data_ptr() for o in out])
            ref, before = filter_and_check(env, ctx, q, d_q, 2, out, 0.75, D, db["off"], mask)
            if sel == [5]:                                               # no other selected object: everything survives
                assert ref["dropped"] == 0 and ref["kept"] > 0
            if sel == []:
                assert before[0].sum() == 0
            if len(sel) == 3:
                assert ref["kept"] > 0
        ctx.select_objects(None)                                         # all objects again: the whole DB's answer
        out = env.outputs(nq, 2)
        ctx.match_device(d_q.data_ptr(), nq, 2, 35, *[o.data_ptr() for o in out])
        whole, _ = filter_and_check(env, ctx, q, d_q, 2, out, 0.75, D, db["off"])
        assert whole["dropped"] > 0
    finally:
        ctx.select_objects(None)


def test_with_a_bit_order(env):
    db = RC.make_db(32)
    nq = 70
    q, D = table(32, nq)
    d_q = env.upload(q)
    ordered = env.capi.Context(0)
    try:
        ordered.set_db_bit_order(1)
        ordered.db_load(db["desc"], db["pts"], db["off"])
        assert not np.array_equal(ordered.db_bit_order(), np.arange(256))                 # the stored rows ARE permuted
        own = nearest_object(D, db["off"])
        assert np.array_equal(env.other_min(ordered, d_q, nq, own), R.other(D, db["off"], own))
        out = env.outputs(nq, 2)
        ordered.match_device(d_q.data_ptr(), nq, 2, 35, *[o.data_ptr() for o in out])
        ref, before = filter_and_check(env, ordered, q, d_q, 2, out, 0.8, D, db["off"])
        assert ref["dropped"] > 0 and ref["kept"] > 0
        ordered.set_ratio_test_other(0.8)
        out = env.outputs(nq, 2)
        ordered.match_device(d_q.data_ptr(), nq, 2, 35, *[o.data_ptr() for o in out])
        assert np.array_equal(env.image(ordered, out)[0], ref["counts"])
    finally:
        ordered.close()


# ---------------------------------------------------------------- shards

@pytest.mark.parametrize("shard_count", [2, 3])
@pytest.mark.parametrize("width", RC.WIDTHS)
def test_shards_minimum_over_ranks_then_apply(env, width, shard_count):
    """per-shard primitive -> torch.minimum over the shards -> apply == ratio_other_device on the unsharded context, byte for byte"""
    torch, capi, db = env.torch, env.capi, RC.make_db(width)
    whole = env.ctx[width]
    nq, k, ratio = 70, 2, 0.8
    q, D = table(width, nq)
    d_q = env.upload(q)
    shards = [env.context(width, shard_rank=r, shard_count=shard_count) for r in range(shard_count)]
    try:
        out = env.outputs(nq, k)
        whole.match_device(d_q.data_ptr(), nq, k, 35, *[o.data_ptr() for o in out])
        before = env.image(whole, out)
        mine = tuple(o.clone() for o in out)
        ref, _ = filter_and_check(env, whole, q, d_q, k, out, ratio, D, db["off"])
        want = env.image(whole, out)
        excl, lim = R.limits_of(before[0], before[1], k, ratio)
        d_excl, d_lim = env.upload(excl), env.upload(lim)
        cap = int(R.limit(8 * width, ratio))
        per_rank, covered = [], 0
        for r, c in enumerate(shards):
            info = c.db_info()
            covered += info["shard_rows"]
            d_min = env.words(nq)
            c.other_object_min_device(d_q.data_ptr(), nq, d_excl.data_ptr(), d_min.data_ptr(), d_lim.data_ptr(), cap)
            c.synchronize()
            mask = R.searched_mask(db["off"], shard=(info["shard_first"], info["shard_rows"]))
            assert np.array_equal(d_min.cpu().numpy().view(np.uint32), R.other_min(D, db["off"], excl, lim, cap, mask)), r
            # ... and the exact per-shard minimum: NONE on a shard that holds only the excluded object's rows, or none at all
            exact = env.other_min(c, d_q, nq, excl)
            assert np.array_equal(exact, R.other_min(D, db["off"], excl, searched=mask)), r
            per_rank.append(d_min)
            if info["shard_rows"] != RC.N_ROWS:                          # (of two object-aligned halves the first holds every object here)
                assert capi.lib().todhip_ratio_other_device(c._h, d_q.data_ptr(), nq, ratio, k, mine[0].data_ptr(), mine[1].data_ptr()) == capi.EINVAL
                assert capi.lib().todhip_set_ratio_test_other(c._h, ratio) == capi.EINVAL
            assert capi.lib().todhip_set_ratio_test_other(c._h, 0.0) == capi.OK
        assert covered == RC.N_ROWS
        # unsigned minimum: the words are below 2^31 or NONE (-1 as int32), so compare as int64 of the unsigned value
        u = [t.to(torch.int64) & 0xFFFFFFFF for t in per_rank]
        total = u[0]
        for t in u[1:]:
            total = torch.minimum(total, t)
        d_total = env.upload(total.cpu().numpy().astype(np.uint32))
        assert np.array_equal(total.cpu().numpy().astype(np.uint32), R.other_min(D, db["off"], excl, lim, cap))
        shards[-1].ratio_other_apply_device(ratio, nq, k, d_total.data_ptr(), mine[0].data_ptr(), mine[1].data_ptr())   # any rank's context
        same_image(env.image(shards[-1], mine), want)
        assert ref["dropped"] > 0 and ref["kept"] > 0
    finally:
        for c in shards:
            c.close()


# ---------------------------------------------------------------- refusals

def test_refusals_leave_the_outputs_untouched(env):
    capi, L = env.capi, env.capi.lib()
    ctx, db = env.ctx[32], RC.make_db(32)
    nq = 33
    q, D = table(32, nq)
    d_q = env.upload(q)
    out = env.outputs(nq, 2)
    ctx.match_device(d_q.data_ptr(), nq, 2, 35, *[o.data_ptr() for o in out])
    before = env.image(ctx, out)
    p = [o.data_ptr() for o in out]
    d_excl, d_min = env.upload(np.zeros(nq, np.uint32)), env.words(nq)

    def whole(h=ctx._h, dq=d_q.data_ptr(), n=nq, ratio=0.8, stride=2, c=p[0], m=p[1]):
        return L.todhip_ratio_other_device(h, dq, n, ratio, stride, c, m)

    def apply(h=ctx._h, ratio=0.8, n=nq, stride=2, o=d_min.data_ptr(), c=p[0], m=p[1]):
        return L.todhip_ratio_other_apply_device(h, ratio, n, stride, o, c, m)

    def prim(h=ctx._h, dq=d_q.data_ptr(), n=nq, e=d_excl.data_ptr(), lim=None, cap=NONE, o=d_min.data_ptr()):
        return L.todhip_other_object_min_device(h, dq, n, e, lim, cap, o)
    nan = float("nan")
    for bad in (dict(h=None), dict(dq=None), dict(c=None), dict(m=None), dict(n=0), dict(ratio=0.0), dict(ratio=-0.5), dict(ratio=1.5),
                dict(ratio=nan), dict(stride=0), dict(stride=1025)):
        assert whole(**bad) == capi.EINVAL, bad
    for bad in (dict(h=None), dict(o=None), dict(c=None), dict(m=None), dict(n=0), dict(ratio=0.0), dict(ratio=1.0001), dict(ratio=nan),
                dict(stride=0), dict(stride=1025)):
        assert apply(**bad) == capi.EINVAL, bad
    for bad in (dict(h=None), dict(dq=None), dict(e=None), dict(o=None), dict(n=0)):
        assert prim(**bad) == capi.EINVAL, bad
    for bad in (-0.1, 1.5, nan):
        assert L.todhip_set_ratio_test_other(ctx._h, bad) == capi.EINVAL
    assert (d_min.cpu().numpy().view(np.uint32) == RC.SENTINEL).all()
    empty, flt = capi.Context(0), capi.Context(0)
    try:
        assert whole(h=empty._h) == capi.ENODB and apply(h=empty._h) == capi.ENODB and prim(h=empty._h) == capi.ENODB
        assert L.todhip_set_ratio_test_other(empty._h, 0.8) == capi.OK                   # nothing loaded yet: nothing to object to
        rng = np.random.Generator(np.random.PCG64(3))
        flt.db_load(rng.standard_normal((40, 128)).astype(np.float32), db["pts"][:40], np.array([0, 40], np.uint32))
        assert whole(h=flt._h) == capi.EINVAL and apply(h=flt._h) == capi.EINVAL and prim(h=flt._h) == capi.EINVAL
        assert L.todhip_set_ratio_test_other(flt._h, 0.8) == capi.EINVAL and L.todhip_set_ratio_test_other(flt._h, 0.0) == capi.OK
        # the refused setter changed nothing: 0.8 set above, a reload as one shard of three refuses 0.5, a whole reload still filters at 0.8
        c = empty
        c.db_load(db["desc"], db["pts"], db["off"], shard_rank=1, shard_count=3)
        assert 0 < c.db_info()["shard_rows"] < RC.N_ROWS
        assert L.todhip_set_ratio_test_other(c._h, 0.5) == capi.EINVAL
        c.db_load(db["desc"], db["pts"], db["off"])
        out2 = env.outputs(nq, 2)
        c.match_device(d_q.data_ptr(), nq, 2, 35, *[o.data_ptr() for o in out2])
        ref8 = R.ratio_other(before[0], before[1], 2, 0.8, D, db["off"])
        ref5 = R.ratio_other(before[0], before[1], 2, 0.5, D, db["off"])
        assert not np.array_equal(ref8["counts"], ref5["counts"])
        assert np.array_equal(env.image(c, out2)[0], ref8["counts"])
    finally:
        empty.close()
        flt.close()
    same_image(env.image(ctx, out), before)
