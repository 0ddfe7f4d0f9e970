"""todhip_match_l2_radius[_device] on the GPU against its definition (include/todhip.h), bit for bit: the numpy statement of it
(tests/match_l2_radius_ref.py, which tests/test_match_l2_radius_cpu.py pins to the oracle on the first 70 queries of the same
inputs) and the oracle itself where its lists stay short. Shapes are the smallest at which the kernels can go wrong: objects of 0,
1, 31, 32, 33, 257, 5 and 700 rows (the 32-row tile), 1 ... 600 queries (513 crosses the 512-query block), rows planted exactly on
the radius, candidates that spill from a lane's slot into the shared list, lists that overflow (the ordered scan) and ones that do not.

The device form leaves the slots behind counts[q] unwritten; the tests prefill them and look."""
import ctypes as C

import numpy as np
import pytest

import l2_radius_cases as K
import match_l2_radius_ref as R
import oracle_lib as O
from tod_amd import capi, synth

pytestmark = pytest.mark.gpu

NQS = (1, 33, 70, 513, 600)
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def db():
    return K.Db()


@pytest.fixture(scope="module")
def ctx(db):
    c = capi.Context(0)
    c.db_load(db.desc, db.pts, db.off)
    yield c
    c.close()


class Dev:
    """todhip_match_l2_radius_device through torch tensors; the outputs are prefilled so that untouched slots show"""

    def __init__(self):
        import torch
        self.torch = torch

    def raw(self, c, q, radius, mpq, with_in_radius=True):
        torch = self.torch
        nq = len(q)
        d_q = torch.from_numpy(np.ascontiguousarray(q, np.float32)).cuda()
        cnt = torch.full((nq,), 77, dtype=torch.int32, device="cuda")
        inr = torch.full((nq,), 78, dtype=torch.int32, device="cuda")
        mm = torch.full((nq * mpq, 4), SENTINEL, dtype=torch.int32, device="cuda")
        xx = torch.full((nq * mpq, 3), -7.5, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        c.match_l2_radius_device(d_q.data_ptr(), nq, radius, mpq, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr(),
                                 inr.data_ptr() if with_in_radius else None)
        c.synchronize()
        return cnt.cpu().numpy(), mm.cpu().numpy(), xx.cpu().numpy(), inr.cpu().numpy()

    def match(self, c, q, radius, mpq, with_in_radius=True):
        nq = len(q)
        cnt, mm, xx, inr = self.raw(c, q, radius, mpq, with_in_radius)
        cnt = cnt.astype(np.int64)
        keep = np.arange(mpq)[None, :] < cnt[:, None]
        assert (mm.reshape(nq, mpq, 4)[~keep] == SENTINEL).all() and (xx.reshape(nq, mpq, 3)[~keep] == -7.5).all(), "slots behind counts[q] were written"
        if not with_in_radius:
            assert (inr == 78).all()
        m = mm.view(capi.DMATCH_DTYPE).reshape(nq, mpq)[keep]
        return np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32), m, xx.reshape(nq, mpq, 3)[keep], inr.astype(np.uint32)


@pytest.fixture(scope="module")
def dev():
    return Dev()


def same(got, want, what="", in_radius=True):
    assert np.array_equal(got[0], want[0]), what
    for f in K.FIELDS:
        assert np.array_equal(got[1][f], want[1][f]), (what, f)
    assert np.array_equal(got[2], want[2]), what
    if in_radius:
        assert np.array_equal(got[3], want[3]), what


def prefix(want, nq):
    """the answer for the first nq queries of a call"""
    n = int(want[0][nq])
    return want[0][:nq + 1], want[1][:n], want[2][:n], want[3][:nq]


def rows_of(off, m):
    return off[m["imgIdx"]].astype(np.int64) + m["trainIdx"]


def three_runs_identical(dev, c, q, radius, mpq):
    runs = [dev.raw(c, q, radius, mpq) for _ in range(3)]
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert a.tobytes() == b.tobytes(), (radius, mpq)


# ---------------------------------------------------------------------------------------------------- 1. edges of the tiling
@pytest.fixture(scope="module")
def wants(db):
    """the definition for all 600 queries, once per (radius, max_per_query): every nq is a prefix of them"""
    dd = R.d2(db.desc, db.q)
    return {(r, m): R.match_l2_radius(db.desc, db.off, db.pts, db.q, r, m, dd) for r in K.RADII for m in K.MPQS}


@pytest.mark.parametrize("nq", NQS)
def test_host_and_device_forms_equal_the_definition(ctx, dev, db, wants, nq):
    n = len(db.desc)
    for radius in K.RADII:
        for mpq in K.MPQS:
            want = prefix(wants[(radius, mpq)], nq)
            what = (nq, radius, mpq)
            same(ctx.match_l2_radius(db.q[:nq], radius, mpq), want, what)
            same(dev.match(ctx, db.q[:nq], radius, mpq), want, what)
        assert not want[3].any() if radius == K.RADII[0] else (want[3] == n).all() if radius == K.RADII[-1] else 0 < want[3].max() < n
    same(dev.match(ctx, db.q[:nq], 150.0, 5, with_in_radius=False), prefix(wants[(150.0, 5)], nq), in_radius=False)
    cnt = ctx.counters()
    assert cnt.last_nq == nq and cnt.last_k == 5


def test_the_first_queries_equal_the_oracle(ctx, db):
    """the oracle directly, without the numpy statement in between"""
    q = db.q[:33]
    keys = O.l2_knn_keys(db.desc, q, len(db.desc))
    d2 = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    for radius, mpq in ((150.0, 5), (1150.0, 64), (1150.0, 1024)):
        rc, rp, m, xyz = O.l2_match(db.desc, db.off, db.pts, q, mpq, radius)
        assert rc == 0
        same(ctx.match_l2_radius(q, radius, mpq), (rp, m, xyz, (~(np.sqrt(d2) > np.float32(radius))).sum(axis=1)), (radius, mpq))


def test_counters_and_kernel_timing(ctx, db):
    ctx.set_kernel_timing(True)
    try:
        before = ctx.counters().n_match_kernel_launches
        rp, m, _, _ = ctx.match_l2_radius(db.q[:70], 1150.0, 16)        # (16 per query: the binding's buffers fit at once)
        cnt = ctx.counters()
        assert cnt.last_nq == 70 and cnt.last_k == 16 and cnt.last_matches == len(m) == int(rp[-1]) == 70 * 16
        assert cnt.n_match_kernel_launches == before + 1 and cnt.last_match_kernel_ms > 0
    finally:
        ctx.set_kernel_timing(False)


# ---------------------------------------------------------------------------------------------------- 2. the boundary
def test_rows_exactly_on_the_radius_and_one_ulp_beyond(dev):
    """d2 = 3600 against radius 60: inside; against the next float below 60: outside. Query 1 and its rows are shifted by 100 000 in
    every dimension: a norm of 1.1e6, equal to Rmax, where the bf16 scores say nothing and eps(q) is at its largest."""
    desc, off, pts, q, radius = K.boundary()
    c = capi.Context(0)
    try:
        c.db_load(desc, pts, off)
        for r, inside in ((radius, 2), (np.nextafter(radius, np.float32(0)), 1)):
            for mpq in (1, 5):
                want = R.match_l2_radius(desc, off, pts, q, r, mpq)
                assert list(want[3]) == [inside] * 3
                same(c.match_l2_radius(q, float(r), mpq), want, (float(r), mpq))
                same(dev.match(c, q, float(r), mpq), want, (float(r), mpq))
        got = c.match_l2_radius(q, float(radius), 5)
        assert list(rows_of(off, got[1])) == [42, 40, 104, 102, 42, 40] and list(got[1]["distance"][1::2]) == [60.0] * 3
    finally:
        c.close()


def test_a_radius_whose_square_overflows_takes_every_row_and_no_padding_row(ctx, dev, db):
    n = len(db.desc)                                                     # 1059 rows: 29 padding rows behind them
    q = db.q[:33]
    for mpq in (5, 1024):
        want = R.match_l2_radius(db.desc, db.off, db.pts, q, 1.0e20, mpq)
        assert (want[3] == n).all()
        same(ctx.match_l2_radius(q, 1.0e20, mpq), want, mpq)
        got = dev.match(ctx, q, 1.0e20, mpq)
        same(got, want, mpq)
        assert rows_of(db.off, got[1]).max() < n


# ---------------------------------------------------------------------------------------------------- 3. slot spill and ties
@pytest.fixture(scope="module")
def spill():
    """5 000 rows (one 32-row tile per chunk, so a lane half's slot answers for 16 rows of it): rows 1000..1059 are near copies of one
    vector and rows 2000..2039 EXACT copies of row 1500 -- more than 8 candidates per (chunk, lane half), so the shared list is in use,
    and 41 equal distances. Queries: next to the vector, row 1500 itself and next to it, random ones."""
    rng = np.random.Generator(np.random.PCG64(321))
    desc = (rng.random((5000, 128)) * 200).astype(np.float32)
    base = (rng.random(128) * 200).astype(np.float32)
    desc[1000:1060] = base[None, :] + rng.normal(0, 0.02, (60, 128)).astype(np.float32)
    desc[2000:2040] = desc[1500]
    pts = rng.random((5000, 3)).astype(np.float32)
    off = np.array([0, 1010, 2020, 5000], np.uint32)
    q = np.concatenate([base[None, :] + rng.normal(0, 0.02, (6, 128)).astype(np.float32), desc[1500:1501],
                        desc[1500:1501] + rng.normal(0, 0.02, (3, 128)).astype(np.float32),
                        (rng.random((20, 128)) * 200).astype(np.float32)]).astype(np.float32)
    c = capi.Context(0)
    c.db_load(desc, pts, off)
    yield c, desc, pts, off, q
    c.close()


@pytest.mark.parametrize("mpq", [5, 64])
def test_spill_into_the_shared_list_and_equal_distances(spill, dev, mpq):
    c, desc, pts, off, q = spill
    want = R.match_l2_radius(desc, off, pts, q, 1.0, mpq)
    assert (want[3][:6] == 60).all() and (want[3][6:10] == 41).all() and not want[3][10:].any()
    same(c.match_l2_radius(q, 1.0, mpq), want)
    got = dev.match(c, q, 1.0, mpq)
    same(got, want)
    mine = rows_of(off, got[1][got[1]["queryIdx"] == 6])                 # the duplicates: lowest rows first
    assert list(mine) == ([1500] + list(range(2000, 2040)))[:mpq]
    three_runs_identical(dev, c, q, 1.0, mpq)


# ---------------------------------------------------------------------------------------------------- 4. the ordered scan
@pytest.fixture(scope="module")
def cluster():
    """5 000 rows, 3 000 of them a tight cluster of near ties; 40 queries: every fourth inside the cluster (more candidates than a list
    holds: the ordered scan), the others next to rows outside it (one row in range each)"""
    rng = np.random.Generator(np.random.PCG64(77))
    base = rng.random(128, dtype=np.float32) * 100
    desc = (rng.random((5000, 128)) * 100).astype(np.float32)
    where = np.sort(rng.choice(5000, 3000, replace=False))
    desc[where] = (base[None, :] + rng.normal(0, 0.05, (3000, 128))).astype(np.float32)
    outside = np.setdiff1d(np.arange(5000), where)
    pts = rng.random((5000, 3)).astype(np.float32)
    off = np.array([0, 1234, 5000], np.uint32)
    q = (desc[outside[:40]] + rng.normal(0, 0.05, (40, 128))).astype(np.float32)
    q[::4] = (base[None, :] + rng.normal(0, 0.05, (10, 128))).astype(np.float32)
    c = capi.Context(0)
    c.db_load(desc, pts, off)
    yield c, desc, pts, off, q
    c.close()


@pytest.mark.parametrize("mpq", [5, 1024])
def test_overflowing_queries_take_the_ordered_scan(cluster, dev, mpq):
    c, desc, pts, off, q = cluster
    want = R.match_l2_radius(desc, off, pts, q, 2.0, mpq)                # cluster rows are ~0.8 apart
    assert (want[3][::4] == 3000).all() and (want[3][::4] > 2048).all() and (np.delete(want[3], np.arange(0, 40, 4)) == 1).all()
    same(c.match_l2_radius(q, 2.0, mpq), want)
    same(dev.match(c, q, 2.0, mpq), want)
    three_runs_identical(dev, c, q, 2.0, mpq)


# ---------------------------------------------------------------------------------------------------- 5. agreement with the k-NN call
def test_max_per_query_up_to_8_equals_match_l2_and_leaves_it_unchanged(ctx, db):
    q = db.q[:70]
    for radius in (150.0, 1150.0):
        for k in range(1, 9):
            knn = ctx.match_l2(q, k, radius)
            rad = ctx.match_l2_radius(q, radius, k)
            same(rad, knn, (radius, k), in_radius=False)
            assert np.array_equal(np.minimum(rad[3], k), np.diff(rad[0].astype(np.int64)))
            again = ctx.match_l2(q, k, radius)                           # the shared workspace is not disturbed
            same(again, knn, (radius, k), in_radius=False)


# ---------------------------------------------------------------------------------------------------- 6. one larger shape
def test_many_chunks_and_two_query_blocks(dev):
    """20 000 rows x 600 queries: chunks of several tiles, two query blocks, about 60 random rows inside the radius per query"""
    rng = np.random.Generator(np.random.PCG64(5))
    n, nq, radius, mpq = 20000, 600, 1000.0, 64
    desc = rng.integers(0, 256, (n, 128)).astype(np.float32)
    pts = rng.standard_normal((n, 3)).astype(np.float32)
    off = np.array([0, 7000, 7001, 19999, 20000], np.uint32)
    q = rng.integers(0, 256, (nq, 128)).astype(np.float32)
    q[::3] = desc[rng.integers(0, n, len(q[::3]))]                       # a third of the queries are rows: distance 0 somewhere
    q[::3, 5] += 3
    c = capi.Context(0)
    try:
        c.db_load(desc, pts, off)
        host = c.match_l2_radius(q, radius, mpq)
        device = dev.match(c, q, radius, mpq)
    finally:
        c.close()
    want = R.match_l2_radius(desc, off, pts, q, radius, mpq)
    assert want[3][::3].min() >= 1 and (want[3] > mpq).any() and (want[3] < mpq).any()
    same(host, want)
    same(device, want)


# ---------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_and_capacity(ctx, db):
    import torch
    L = capi.lib()
    nq, mpq = 8, 4
    q = np.ascontiguousarray(db.q[:nq])
    rp, inr = np.zeros(nq + 1, np.uint32), np.zeros(nq, np.uint32)
    m, xyz = np.zeros(nq * mpq, capi.DMATCH_DTYPE), np.zeros((nq * mpq, 3), np.float32)
    n = C.c_uint32(nq * mpq)

    def host(h=ctx._h, q_=q.ctypes.data, nq_=nq, radius=150.0, mpq_=mpq, rp_=rp.ctypes.data, m_=m.ctypes.data, x_=xyz.ctypes.data,
             n_=C.addressof(n), in_=inr.ctypes.data):
        return L.todhip_match_l2_radius(h, q_, nq_, radius, mpq_, rp_, m_, x_, n_, in_)

    assert host() == capi.OK and n.value == rp[nq]
    n.value = nq * mpq
    assert host(in_=None) == capi.OK                                     # in_radius may be NULL
    bad_radii = [dict(radius=r) for r in (0.0, -1.0, float("inf"), float("nan"))]
    for bad in [dict(h=None), dict(q_=None), dict(rp_=None), dict(m_=None), dict(x_=None), dict(n_=None), dict(nq_=0), dict(mpq_=0),
                dict(mpq_=1025)] + bad_radii:
        assert host(**bad) == capi.EINVAL, bad
    # capacity: the needed count comes back, row_ptr and in_radius are filled, matches are not
    want = R.match_l2_radius(db.desc, db.off, db.pts, q, 1.0e4, mpq)
    need = int(want[0][-1])
    assert need == nq * mpq
    rp[:] = 0; inr[:] = 0; m[:] = 0
    n.value = need - 1
    assert host(radius=1.0e4) == capi.ECAPACITY and n.value == need
    assert np.array_equal(rp, want[0]) and np.array_equal(inr, want[3]) and not m["distance"].any()
    assert host(radius=1.0e4) == capi.OK and n.value == need and np.array_equal(m["trainIdx"], want[1]["trainIdx"])
    same(ctx.match_l2_radius(db.q[:70], 1.0e4, 64), R.match_l2_radius(db.desc, db.off, db.pts, db.q[:70], 1.0e4, 64))   # the binding grows

    d_q = torch.from_numpy(q).cuda()
    cnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
    mm = torch.zeros((nq * mpq, 4), dtype=torch.int32, device="cuda")
    xx = torch.zeros((nq * mpq, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def device(h=ctx._h, q_=d_q.data_ptr(), nq_=nq, radius=150.0, mpq_=mpq, c_=cnt.data_ptr(), m_=mm.data_ptr(), x_=xx.data_ptr(), in_=None):
        return L.todhip_match_l2_radius_device(h, q_, nq_, radius, mpq_, c_, m_, x_, in_)

    assert device() == capi.OK
    ctx.synchronize()
    for bad in [dict(h=None), dict(q_=None), dict(c_=None), dict(m_=None), dict(x_=None), dict(nq_=0), dict(mpq_=0), dict(mpq_=1025)] + bad_radii:
        assert device(**bad) == capi.EINVAL, bad
    empty = capi.Context(0)
    assert host(h=empty._h) == capi.ENODB and device(h=empty._h) == capi.ENODB
    empty.close()


def test_a_context_reloaded_float_binary_float(db):
    rng = np.random.Generator(np.random.PCG64(9))
    q = db.q[:33]
    want = R.match_l2_radius(db.desc, db.off, db.pts, q, 1150.0, 64)
    c = capi.Context(0)
    try:
        c.db_load(db.desc, db.pts, db.off)
        same(c.match_l2_radius(q, 1150.0, 64), want)
        c.db_load(rng.integers(0, 256, (len(db.desc), 32), dtype=np.uint8), db.pts, db.off)
        with pytest.raises(capi.TodError) as e:
            c.match_l2_radius(q, 1150.0, 64)                             # a DB that is not float
        assert e.value.status == capi.EINVAL
        c.db_load(db.desc[:500], db.pts[:500], np.array([0, 500], np.uint32))
        same(c.match_l2_radius(q, 1150.0, 64), R.match_l2_radius(db.desc[:500], [0, 500], db.pts[:500], q, 1150.0, 64))
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------- 8. end to end
def test_radius_matches_feed_the_verifier():
    """Float descriptors on synth's scene geometry: every model point is four rows (four training views: the same 3D point, descriptors a
    little apart). The radius search's matches go through todhip_verify; the oracle's matcher and verifier run on the same input."""
    bdesc, pts, off = synth.make_db(3, per_object=2000)
    n = len(pts)
    pts = np.ascontiguousarray(pts[(np.arange(n) // 4) * 4])
    fr = synth.make_frame(bdesc, pts, off, 500, frame=0, visible_object=1)
    rng = np.random.Generator(np.random.PCG64(44))
    point = rng.random((n // 4, 128)) * 200
    desc = (point[np.arange(n) // 4] + rng.normal(0, 2.0, (n, 128))).astype(np.float32)
    q = (rng.random((500, 128)) * 200).astype(np.float32)
    on = fr["truth_rows"] >= 0
    q[on] = (desc[fr["truth_rows"][on]] + rng.normal(0, 2.0, (int(on.sum()), 128))).astype(np.float32)
    radius = 100.0                                                       # a point's rows are ~32 from its query, other rows > 800
    c = capi.Context(0)
    try:
        spans = c.db_load(desc, pts, off)
        knn = c.match_l2(q, 5, radius)
        rad = c.match_l2_radius(q, radius, 5)
        same(rad, knn, in_radius=False)                                  # identical by definition
        assert (rad[3][on] == 4).all() and not rad[3][~on].any()

        def verify(mt):
            return c.verify(fr["kp_xy"], fr["cloud"], mt[0], mt[1], mt[2], spans, 8, 2500, 0.01, capi.rng_new(1))

        p_knn, p_rad = verify(knn), verify(rad)
        assert len(p_knn) >= 1 and [p["object"] for p in p_knn] == [p["object"] for p in p_rad]
        for a, b in zip(p_knn, p_rad):
            assert np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"]) and np.array_equal(a["inliers"], b["inliers"])
        wide = c.match_l2_radius(q, radius, 64)
        p_wide = verify(wide)
    finally:
        c.close()
    rc, o_rp, o_m, o_xyz = O.l2_match(desc, off, pts, q, 64, radius)
    assert rc == 0
    same(wide, (o_rp, o_m, o_xyz), in_radius=False)
    rc, o_poses, _ = O.verify(fr["kp_xy"], fr["cloud"], o_rp, o_m, o_xyz, O.spans(pts, off), 8, 2500, 0.01, O.rng_new(1))
    assert rc == 0 and len(o_poses) >= 1 and [p["object"] for p in p_wide] == [p["object"] for p in o_poses]
    for g, o in zip(p_wide, o_poses):
        assert np.abs(g["R"] - o["R"]).max() < 1e-3 and np.abs(g["t"] - o["t"]).max() < 1e-3
