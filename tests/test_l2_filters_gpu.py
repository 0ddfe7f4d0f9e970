"""todhip_set_l2_ratio_test, todhip_cross_check_l2_device and todhip_set_l2_cross_check on the GPU. Every comparison is bit for bit
against the numpy definitions (tests/l2_filters_ref.py), the cross-check on the library's OWN unfiltered output taken just before;
tests/test_l2_filters_cpu.py pins the same inputs on the reference alone (the filters remove some and keep some, the index tie and
the summation order decide some), so nothing here passes vacuously."""
import numpy as np
import pytest

import cross_check_ref as R
import l2_filters_cases as LC
import l2_filters_ref as F
import l2_radius_cases as RC
from match_l2_radius_ref import d2

pytestmark = pytest.mark.gpu


class Env:
    def __init__(self):
        import torch
        from tod_amd import capi
        self.torch, self.capi = torch, capi
        self.made = []
        self.ctx = self.context(LC.make_db())

    def context(self, db, **shard):
        c = self.capi.Context(0)
        self.made.append(c)
        c.db_load(db["desc"], db["pts"], db["off"], **shard)
        return c

    def close(self):
        for c in self.made:
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

    def match(self, ctx, d_q, nq, k, radius):
        out = self.outputs(nq, k)
        ctx.match_l2_device(d_q.data_ptr(), nq, k, radius, *[o.data_ptr() for o in out])
        return out


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


def same_front(got, want_counts, want_m, want_x, stride):
    """counts equal, and the first counts[q] slots of every query equal bit for bit"""
    counts, m, x = got
    assert np.array_equal(counts, want_counts)
    front = np.tile(np.arange(stride), len(counts)) < np.repeat(counts, stride)
    assert np.array_equal(m[front], want_m[front]) and np.array_equal(x[front], np.ascontiguousarray(want_x, np.float32).view(np.uint32)[front])


def same_filtered(got, before, ref, stride):
    """got: the image after the filter; before: the unfiltered image; ref: F.cross_check_l2's result on `before`"""
    same_front(got, ref["counts"], ref["matches"], ref["xyz"], stride)
    slot = np.tile(np.arange(stride), len(got[0]))
    behind = slot >= np.repeat(np.minimum(before[0], stride), stride)    # at or behind the old counts: never written
    assert np.array_equal(got[1][behind], before[1][behind]) and np.array_equal(got[2][behind], before[2][behind])


def filter_and_check(env, ctx, db, q, d_q, Q, stride, out, frame_nq=None):
    """`out` holds an unfiltered output of the library for the queries q: filter it twice, compare with the reference"""
    before = env.image(ctx, out)
    assert before[0].max() <= stride
    ref = F.cross_check_l2(before[0], before[1], before[2].view(np.float32), q, db["desc"], db["off"], Q, stride, frame_nq)
    ptrs = [o.data_ptr() for o in out]
    ctx.cross_check_l2_device(d_q.data_ptr(), len(q), Q, stride, *ptrs, frame_nq=frame_nq)
    once = env.image(ctx, out)
    same_filtered(once, before, ref, stride)
    ctx.cross_check_l2_device(d_q.data_ptr(), len(q), Q, stride, *ptrs, frame_nq=frame_nq)
    twice = env.image(ctx, out)
    assert np.array_equal(twice[0], once[0])                             # idempotent
    same_filtered(twice, before, ref, stride)
    return ref


# ------------------------------------------------------------------------------------------------ the filter entry point
@pytest.mark.parametrize("Q", LC.SINGLE_FRAMES)
def test_single_frame_every_k(env, Q):
    ctx, db = env.ctx, LC.make_db()
    q = LC.make_queries(Q)
    d_q = env.upload(q)
    dd = d2(db["desc"], q)
    for k in LC.KS:
        out = env.match(ctx, d_q, Q, k, LC.RADIUS)
        want = LC.search_ref(db, q, k, LC.RADIUS, dd)
        same_front(env.image(ctx, out), *want, k)                        # the pinned inputs are the library's output
        ref = filter_and_check(env, ctx, db, q, d_q, Q, k, out)
        assert (ref["removed"] > 0) == (Q > 1) and ref["removed"] < ref["total"]


def test_frames_and_frame_nq(env):
    ctx, db = env.ctx, LC.make_db()
    f3 = LC.FRAMES3
    q = LC.make_frames3()
    d_q = env.upload(q)
    for k in (1, 5):
        out = env.match(ctx, d_q, len(q), k, LC.RADIUS)
        ref = filter_and_check(env, ctx, db, q, d_q, f3["Q"], k, out, f3["frame_nq"])
        assert ref["counts"][33:66].sum() == 0 and ref["counts"][73:].sum() == 0 and ref["counts"][66:73].sum() > 0
    # frames without a frame_nq and a short last frame (33 + 33 + 4); frame_nq beyond a frame; 70 frames: frame_nq in device memory
    q = LC.make_queries(70)
    d_q = env.upload(q)
    for Q, frame_nq in ((33, None), (33, [40, 5, 3]), (1, [i % 3 != 1 for i in range(70)])):
        out = env.match(ctx, d_q, 70, 5, LC.RADIUS)
        filter_and_check(env, ctx, db, q, d_q, Q, 5, out, None if frame_nq is None else np.asarray(frame_nq, np.uint32))
    q, frame_nq = LC.make_frames70()
    d_q = env.upload(q)
    out = env.match(ctx, d_q, len(q), 2, LC.RADIUS)
    ref = filter_and_check(env, ctx, db, q, d_q, 2, 2, out, frame_nq)
    assert 0 < ref["removed"] < ref["total"] == 280 and ref["tie_decided"] > 0


@pytest.mark.parametrize("stride", [64, 1024])
def test_radius_search_strides(env, stride):
    ctx, db = env.ctx, LC.make_db()
    q = LC.make_queries(70)
    d_q = env.upload(q)
    for Q, frame_nq in ((70, None), (33, np.array([33, 0, 4], np.uint32))):
        out = env.outputs(70, stride)
        ctx.match_l2_radius_device(d_q.data_ptr(), 70, LC.RADIUS, stride, *[o.data_ptr() for o in out])
        c0 = env.image(ctx, out)[0]
        assert (c0 == 64).any() if stride == 64 else c0.max() > 64       # a count that equals the stride; more than one compaction chunk
        ref = filter_and_check(env, ctx, db, q, d_q, Q, stride, out, frame_nq)
        assert 0 < ref["removed"] < ref["total"]


def test_summation_order_decides_and_the_gpu_gives_the_sequential_answer(env):
    db, q = LC.order_frame()
    ctx = env.context(db)
    d_q = env.upload(q)
    out = env.match(ctx, d_q, 80, 1, 1.0e9)
    ref = filter_and_check(env, ctx, db, q, d_q, 80, 1, out)
    assert ref["removed"] == 40
    before = LC.search_ref(db, q, 1, 1e9)
    alt = F.cross_check_l2(*before, q, db["desc"], db["off"], 80, 1, dist=LC.pairwise_bits)
    assert not np.array_equal(alt["counts"], ref["counts"])              # (another order of the sum would have shown)


def test_early_exit_trap(env):
    db, q, at = LC.trap()
    ctx = env.context(db)
    d_q = env.upload(q)
    for Q, k in ((len(q), 1), (len(q), 2)):
        out = env.match(ctx, d_q, len(q), k, 1.0e9)
        ref = filter_and_check(env, ctx, db, q, d_q, Q, k, out)
        got = env.image(ctx, out)
        named_row0 = [(got[1]["imgIdx"][i * k:i * k + got[0][i]] == 0).any() for i in at]
        assert named_row0 == [True, False, False] and ref["tie_decided"] >= 3


def test_on_a_merged_sharded_output_with_an_empty_shard(env):
    capi, db = env.capi, LC.make_db()
    q = LC.make_queries(70)
    d_q = env.upload(q)
    shards = [env.context(db, shard_rank=r, shard_count=4) for r in range(4)]   # object-aligned quarters: ranks 0 and 1 hold the rows
    rows = [c.db_info()["shard_rows"] for c in shards]
    assert sum(rows) == LC.N_ROWS and [0 < n < LC.N_ROWS for n in rows] == [True, True, False, False]
    keys = env.torch.zeros((4, 70, 5), dtype=env.torch.int64, device="cuda")
    for r, c in enumerate(shards):
        c.match_l2_shard_device(d_q.data_ptr(), 70, 5, keys[r].data_ptr())
        c.synchronize()
    assert (keys[2:] == -1).all().item()                                 # a shard without rows sends padding only
    out = env.outputs(70, 5)
    shards[0].merge_l2_shards_device(keys.data_ptr(), 4, 70, 5, LC.RADIUS, *[o.data_ptr() for o in out])
    merged = env.image(shards[0], out)
    plain = env.image(env.ctx, env.match(env.ctx, d_q, 70, 5, LC.RADIUS))
    same_front(merged, plain[0], plain[1], plain[2].view(np.float32), 5)
    # a shard's own context refuses to filter, outputs untouched
    L = capi.lib()
    assert L.todhip_cross_check_l2_device(shards[0]._h, d_q.data_ptr(), 70, 70, None, 5, *[o.data_ptr() for o in out]) == capi.EINVAL
    assert L.todhip_set_l2_cross_check(shards[1]._h, 70) == capi.EINVAL
    for a, b in zip(env.image(shards[0], out), merged):
        assert np.array_equal(a, b)
    ref = filter_and_check(env, env.ctx, db, q, d_q, 70, 5, out)
    assert 0 < ref["removed"] < ref["total"]


# ------------------------------------------------------------------------------------------------ the setter
def test_setter_equals_match_then_filter_and_follows_the_ratio_test(env):
    db = LC.make_db()
    ctx = env.ctx
    q = LC.make_queries(70)
    d_q = env.upload(q)
    dd = d2(db["desc"], q)
    plain = env.context(db)                                              # a context that never hears of the options
    try:
        for k, Q, ratio in ((5, 70, 0.0), (1, 33, 0.0), (8, 2, 0.0), (5, 70, 0.7), (1, 70, 0.7)):
            before = env.image(plain, env.match(plain, d_q, 70, k, LC.RADIUS))
            if ratio:                                                    # ratio -> radius -> cross-check
                before = F.ratio_filter(dd, k, LC.RADIUS, ratio, db["off"], db["pts"], LC.SENTINEL)
                before = (before[0], before[1], before[2].view(np.uint32))
                assert 0 < (before[0] > 0).sum() < 70
            ref = F.cross_check_l2(before[0], before[1], before[2].view(np.float32), q, db["desc"], db["off"], Q, k)
            assert 0 < ref["removed"] < ref["total"]
            ctx.set_l2_ratio_test(ratio)
            ctx.set_l2_cross_check(Q)
            same_front(env.image(ctx, env.match(ctx, d_q, 70, k, LC.RADIUS)), ref["counts"], ref["matches"], ref["xyz"], k)
            row_ptr, m, xyz = ctx.match_l2(q, k, LC.RADIUS)              # the host form packs its CSR from the filtered counts
            w_ptr, w_m, w_xyz = R.csr(ref["counts"], ref["matches"], ref["xyz"], k)
            assert np.array_equal(row_ptr, w_ptr) and np.array_equal(m, w_m) and np.array_equal(xyz.view(np.uint32), w_xyz.view(np.uint32))
            ctx.set_l2_ratio_test(0.0)
            ctx.set_l2_cross_check(0)                                    # off again: byte for byte the plain context's outputs
            for a, b in zip(env.image(ctx, env.match(ctx, d_q, 70, k, LC.RADIUS)), env.image(plain, env.match(plain, d_q, 70, k, LC.RADIUS))):
                assert np.array_equal(a, b)
            p_ptr, p_m, p_xyz = plain.match_l2(q, k, LC.RADIUS)
            row_ptr, m, xyz = ctx.match_l2(q, k, LC.RADIUS)
            assert np.array_equal(row_ptr, p_ptr) and np.array_equal(m, p_m) and np.array_equal(xyz.view(np.uint32), p_xyz.view(np.uint32))
    finally:
        ctx.set_l2_ratio_test(0.0)
        ctx.set_l2_cross_check(0)


# ------------------------------------------------------------------------------------------------ the ratio test
def ratio_sweep(env, ctx, db, q, radii, ks=(1, 2, 5, 8), ratios=(0.5, 0.8, 1.0), dd=None):
    """match_l2_device and match_l2 with the ratio test on against the definition; returns how many queries were dropped in all"""
    d_q = env.upload(q)
    dd = d2(db["desc"], q) if dd is None else dd
    dropped = 0
    try:
        for ratio in ratios:
            ctx.set_l2_ratio_test(ratio)
            keep = F.ratio_passes(dd, ratio)
            dropped += int((~keep).sum())
            for radius in radii:
                two = None
                for k in sorted(ks, reverse=True):
                    want = F.ratio_filter(dd, k, radius, ratio, db["off"], db["pts"])
                    got = env.image(ctx, env.match(ctx, d_q, len(q), k, radius))
                    same_front(got, *want, k)
                    assert (got[0][~keep] == 0).all()
                    if k == 2:
                        two = got
                    if k == 1 and two is not None:                       # k = 1 on returns the first match of k = 2 on
                        assert np.array_equal(got[0], np.minimum(two[0], 1))
                        has = got[0] == 1
                        assert np.array_equal(got[1][has], two[1][0::2][has]) and np.array_equal(got[2][has], two[2][0::2][has])
                row_ptr, m, xyz = ctx.match_l2(q, ks[0], radius)
                want = F.ratio_filter(dd, ks[0], radius, ratio, db["off"], db["pts"])
                w_ptr, w_m, w_xyz = R.csr(*want, ks[0])
                assert np.array_equal(row_ptr, w_ptr) and np.array_equal(m, w_m) and np.array_equal(xyz.view(np.uint32), w_xyz.view(np.uint32))
    finally:
        ctx.set_l2_ratio_test(0.0)
    return dropped


def test_ratio_sweep_on_the_small_db_and_the_planted_rows(env):
    big = RC.Db(nq=70)
    db = dict(desc=big.desc, pts=big.pts, off=big.off)
    ctx = env.context(db)
    assert ratio_sweep(env, ctx, db, big.q, (150.0, 1.0e4)) == 20
    db, q = LC.ratio_planted()
    ctx = env.context(db)
    d_q = env.upload(q)
    try:
        for col, ratio in enumerate((0.5, 0.8, 1.0)):
            ctx.set_l2_ratio_test(ratio)
            got = env.image(ctx, env.match(ctx, d_q, len(q), 2, LC.RATIO_RADIUS))
            assert [c > 0 for c in got[0]] == [LC.RATIO_WANT[name][col] for name in LC.RATIO_SCENARIOS], ratio
    finally:
        ctx.set_l2_ratio_test(0.0)
    assert ratio_sweep(env, ctx, db, q, (LC.RATIO_RADIUS, 1.0e5)) > 0
    # a one-row DB passes
    one = dict(desc=db["desc"][:1], pts=db["pts"][:1], off=np.array([0, 1], np.uint32))
    ctx1 = env.context(one)
    assert ratio_sweep(env, ctx1, one, q, (1.0e9,), ks=(1, 2), ratios=(0.5,)) == 0


def test_ratio_on_the_one_gemm_path_and_through_the_exact_scan(env):
    """65 536 rows select the one-GEMM path (tod_amd/csrc/l2_plan.h: 2048 tiles; tests/test_l2_gpu.py's switch_db sizes); 1500
    near-copies of one vector overflow the candidate lists of the queries beside it, which the exact scan then answers
    (test_one_gemm_path_with_overflowing_candidate_lists's construction)."""
    rng = np.random.Generator(np.random.PCG64(123))
    n = 65536
    desc = (rng.random((n, 128)) * 200).astype(np.float32)
    base = (rng.random(128) * 200).astype(np.float32)
    desc[rng.choice(n, 1500, replace=False)] = base[None, :] + rng.normal(0, 0.02, (1500, 128)).astype(np.float32)
    q = np.concatenate([base[None, :] + rng.normal(0, 0.02, (4, 128)).astype(np.float32),       # overflow -> exact scan
                        desc[rng.integers(0, n, 8)] + rng.normal(0, 3.0, (8, 128)).astype(np.float32),
                        (rng.random((4, 128)) * 200).astype(np.float32)]).astype(np.float32)
    db = dict(desc=desc, pts=rng.random((n, 3)).astype(np.float32), off=np.array([0, 20011, 20011, n], np.uint32))
    ctx = env.context(db)
    dropped = ratio_sweep(env, ctx, db, q, (1.0e9,), ks=(1, 2, 8), ratios=(0.8,))
    assert 0 < dropped < len(q)


def test_sixteen_frames_in_one_call_equal_their_single_frame_calls(env):
    ctx, db = env.ctx, LC.make_db()
    frames = [LC.make_queries(33, seed) for seed in range(16)]
    q = np.concatenate(frames)
    d_q = env.upload(q)
    try:
        ctx.set_l2_ratio_test(0.9)
        ctx.set_l2_cross_check(33)
        whole = env.image(ctx, env.match(ctx, d_q, len(q), 2, LC.RADIUS))
        assert 0 < (whole[0] > 0).sum() < len(q)
        for f in (0, 7, 15):
            d_f = env.upload(frames[f])
            alone = env.image(ctx, env.match(ctx, d_f, 33, 2, LC.RADIUS))
            part = (whole[0][33 * f:33 * f + 33], whole[1][66 * f:66 * f + 66].copy(), whole[2][66 * f:66 * f + 66])
            part[1]["queryIdx"] -= 33 * f
            same_front(part, alone[0], alone[1], alone[2].view(np.float32), 2)
    finally:
        ctx.set_l2_ratio_test(0.0)
        ctx.set_l2_cross_check(0)


def test_sharded_pair_with_the_ratio_test_and_the_radius_forms_without(env):
    capi, db = env.capi, LC.make_db()
    L = capi.lib()
    q = LC.make_queries(70)
    d_q = env.upload(q)
    dd = d2(db["desc"], q)
    shards = [env.context(db, shard_rank=r, shard_count=3) for r in range(3)]
    assert sum(c.db_info()["shard_rows"] for c in shards) == LC.N_ROWS
    ctx = env.ctx
    plain_radius = env.outputs(70, 64)
    ctx.match_l2_radius_device(d_q.data_ptr(), 70, LC.RADIUS, 64, *[o.data_ptr() for o in plain_radius])
    plain_radius = env.image(ctx, plain_radius)
    try:
        for c in shards + [ctx]:
            c.set_l2_ratio_test(0.7)
        ctx.set_l2_cross_check(70)
        for k in (2, 5):
            keys = env.torch.zeros((3, 70, k), dtype=env.torch.int64, device="cuda")
            for r, c in enumerate(shards):
                c.match_l2_shard_device(d_q.data_ptr(), 70, k, keys[r].data_ptr())
                c.synchronize()
            out = env.outputs(70, k)
            shards[1].merge_l2_shards_device(keys.data_ptr(), 3, 70, k, LC.RADIUS, *[o.data_ptr() for o in out])
            want = F.ratio_filter(dd, k, LC.RADIUS, 0.7, db["off"], db["pts"])
            assert 0 < (want[0] > 0).sum() < 70
            same_front(env.image(shards[1], out), *want, k)
        # k = 1 is refused while the test is on, by both steps; nothing is written
        keys = env.torch.full((3, 70, 1), 7, dtype=env.torch.int64, device="cuda")
        out = env.outputs(70, 1)
        assert L.todhip_match_l2_shard_device(shards[0]._h, d_q.data_ptr(), 70, 1, keys.data_ptr()) == capi.EINVAL
        assert L.todhip_merge_l2_shards_device(shards[0]._h, keys.data_ptr(), 3, 70, 1, LC.RADIUS, *[o.data_ptr() for o in out]) == capi.EINVAL
        shards[0].synchronize()
        assert (keys == 7).all().item() and (env.image(shards[0], out)[0] == 0x5A5A5A5A).all()
        # the radius forms are unchanged by both settings
        got = env.outputs(70, 64)
        ctx.match_l2_radius_device(d_q.data_ptr(), 70, LC.RADIUS, 64, *[o.data_ptr() for o in got])
        for a, b in zip(env.image(ctx, got), plain_radius):
            assert np.array_equal(a, b)
        rkeys = env.torch.zeros((3, 70, 65), dtype=env.torch.int64, device="cuda")
        for r, c in enumerate(shards):
            c.match_l2_radius_shard_device(d_q.data_ptr(), 70, LC.RADIUS, 64, rkeys[r].data_ptr())
            c.synchronize()
        got = env.outputs(70, 64)
        shards[2].merge_l2_radius_shards_device(rkeys.data_ptr(), 3, 70, 64, *[o.data_ptr() for o in got])
        got = env.image(shards[2], got)
        same_front(got, plain_radius[0], plain_radius[1], plain_radius[2].view(np.float32), 64)
    finally:
        for c in shards + [ctx]:
            c.set_l2_ratio_test(0.0)
        ctx.set_l2_cross_check(0)


# ------------------------------------------------------------------------------------------------ refusals, and nothing changes while off
def test_refusals_leave_settings_and_outputs_untouched(env):
    capi, L = env.capi, env.capi.lib()
    ctx, db = env.ctx, LC.make_db()
    q = LC.make_queries(33)
    d_q = env.upload(q)
    out = env.match(ctx, d_q, 33, 5, LC.RADIUS)
    before = env.image(ctx, out)
    p = [o.data_ptr() for o in out]

    def call(h=ctx._h, dq=d_q.data_ptr(), nq=33, Q=33, stride=5, c=p[0], m=p[1], x=p[2]):
        return L.todhip_cross_check_l2_device(h, dq, nq, Q, None, stride, c, m, x)
    for bad in (dict(h=None), dict(dq=None), dict(c=None), dict(m=None), dict(x=None), dict(nq=0), dict(Q=0), dict(stride=0), dict(stride=1025),
                dict(nq=1 << 21, stride=1024)):
        assert call(**bad) == capi.EINVAL, bad
    import cross_check_cases as CC
    empty = capi.Context(0)
    env.made.append(empty)
    assert call(h=empty._h) == capi.ENODB
    assert L.todhip_set_l2_cross_check(empty._h, 33) == capi.OK and L.todhip_set_l2_cross_check(empty._h, 0) == capi.OK
    for width in CC.WIDTHS:                                              # 32-byte and 64-byte binary DBs
        b = CC.make_db(width)
        binary = env.context(b)
        assert call(h=binary._h) == capi.EINVAL
        assert L.todhip_set_l2_cross_check(binary._h, 33) == capi.EINVAL and L.todhip_set_l2_cross_check(binary._h, 0) == capi.OK
        assert L.todhip_set_l2_ratio_test(binary._h, 0.8) == capi.OK     # with any DB or none
        bq = env.upload(CC.make_queries(width, 33))
        a = env.outputs(33, 5)
        binary.match_device(bq.data_ptr(), 33, 5, CC.RADIUS, *[o.data_ptr() for o in a])
        want = CC.search_ref(b, CC.make_queries(width, 33), 5, CC.RADIUS)
        got = env.image(binary, a)
        assert np.array_equal(got[0], want[0])                           # ... and the Hamming forms do not hear of it
    # a sharded float context: the setter is refused and leaves the setting -- set 33, reload as a shard (refused: 7), reload whole
    c = empty
    assert L.todhip_set_l2_cross_check(c._h, 33) == capi.OK
    c.db_load(db["desc"], db["pts"], db["off"], shard_rank=1, shard_count=4)
    assert 0 < c.db_info()["shard_rows"] < LC.N_ROWS
    assert L.todhip_set_l2_cross_check(c._h, 7) == capi.EINVAL and call(h=c._h) == capi.EINVAL
    c.db_load(db["desc"], db["pts"], db["off"])
    ref = F.cross_check_l2(before[0], before[1], before[2].view(np.float32), q, db["desc"], db["off"], 33, 5)
    ref7 = F.cross_check_l2(before[0], before[1], before[2].view(np.float32), q, db["desc"], db["off"], 7, 5)
    assert not np.array_equal(ref["counts"], ref7["counts"])
    assert np.array_equal(env.image(c, env.match(c, d_q, 33, 5, LC.RADIUS))[0], ref["counts"])
    c.set_l2_cross_check(0)
    # the ratio setter's domain: a refused value leaves the setting
    c.set_l2_ratio_test(0.7)
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        assert L.todhip_set_l2_ratio_test(c._h, bad) == capi.EINVAL
    want = F.ratio_filter(d2(db["desc"], q), 5, LC.RADIUS, 0.7, db["off"], db["pts"])
    assert 0 < (want[0] > 0).sum() < 33
    same_front(env.image(c, env.match(c, d_q, 33, 5, LC.RADIUS)), *want, 5)
    c.set_l2_ratio_test(0.0)
    for a, b in zip(env.image(ctx, out), before):
        assert np.array_equal(a, b)


def test_nothing_changes_while_both_settings_are_off(env):
    """match_l2[_device] after the setters were switched on and off again is byte for byte what a context gave before they were ever
    called, sentinel bytes behind the counts included; the Hamming setters do not reach the float forms"""
    db = LC.make_db()
    q = LC.make_queries(70)
    d_q = env.upload(q)
    fresh = env.context(db)
    first = {k: env.image(fresh, env.match(fresh, d_q, 70, k, LC.RADIUS)) for k in LC.KS}
    host = {k: fresh.match_l2(q, k, LC.RADIUS) for k in LC.KS}
    fresh.set_l2_ratio_test(0.7)
    fresh.set_l2_cross_check(70)
    assert not np.array_equal(env.image(fresh, env.match(fresh, d_q, 70, 5, LC.RADIUS))[0], first[5][0])
    fresh.set_l2_ratio_test(0.0)
    fresh.set_l2_cross_check(0)
    fresh.set_ratio_test(0.5)                                            # the Hamming forms' setter: not for the float forms
    for k in LC.KS:
        for a, b in zip(env.image(fresh, env.match(fresh, d_q, 70, k, LC.RADIUS)), first[k]):
            assert np.array_equal(a, b)
        for a, b in zip(fresh.match_l2(q, k, LC.RADIUS), host[k]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    fresh.set_ratio_test(0.0)
