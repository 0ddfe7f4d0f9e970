"""todhip_match_radius[_device] on the GPU against its definition (include/todhip.h): the oracle's match with k = max_per_query for
the matches, a count over the oracle's complete key lists for in_radius, everything bit for bit. Shapes are the smallest at which
the kernels can go wrong: objects of 0, 1, 31, 32, 33, 257, 5 and 700 rows (short of, on and past a 32-row step), 1 / 33 / 70
queries (two, two and four query blocks per wave), 1 100 queries (six), thresholds on both sides of the integer block test
(radius 127 / 128), candidate buffers that overflow (the ordered rescan) and ones that do not.

The device form leaves the slots behind counts[q] as todhip_match_device leaves them: not written. The tests prefill them and
look."""
import numpy as np
import pytest

import match_radius_ref as R
import oracle_lib as O
from tod_amd import capi, synth

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 31, 32, 33, 257, 5, 700]
NQS = (1, 33, 70)
RADII = (1, 20, 35, 63, 64, 127, 128, 255, 256, 1000)
MPQS = (1, 5, 64, 1024)
FIELDS = ("queryIdx", "trainIdx", "imgIdx", "distance")
SENTINEL = 0x5A5A5A5A


class Db:
    """Random rows in objects of the given sizes; 70 queries: rows of the non-empty objects in turn with 0..20 flipped bits, every
    seventh random"""

    def __init__(self, rows, seed=2024, biased=False):
        rng = np.random.Generator(np.random.PCG64(seed))
        n = int(sum(rows))
        self.off = np.concatenate([[0], np.cumsum(rows)]).astype(np.uint32)
        self.desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        if biased:                                                      # the first 64 bits are set in a quarter of the rows only
            self.desc[:, :8] &= rng.integers(0, 256, (n, 8), dtype=np.uint8)
        self.pts = rng.standard_normal((n, 3)).astype(np.float32)
        full = [o for o in range(len(rows)) if rows[o] > 0]
        self.q = rng.integers(0, 256, (70, 32), dtype=np.uint8)
        for i in range(70):
            if i % 7 == 6:
                continue
            o = full[i % len(full)]
            bits = np.unpackbits(self.desc[int(self.off[o]) + int(rng.integers(0, rows[o]))])
            bits[rng.choice(256, int(rng.integers(0, 21)), replace=False)] ^= 1
            self.q[i] = np.packbits(bits)

    def rows_of(self, sel):
        return np.concatenate([np.arange(self.off[o], self.off[o + 1]) for o in sorted(set(sel))] + [np.zeros(0, np.int64)]).astype(np.int64)

    def want(self, q, radius, mpq, sel=None, keys=None):
        """The definition through the oracle: (row_ptr, matches, xyz, in_radius); sel: the selected objects (None: all); keys: the
        oracle's complete key lists of these queries, when the caller has them already"""
        if sel is None:
            desc, pts, off, S = self.desc, self.pts, self.off, np.arange(len(self.off) - 1)
        else:
            S = np.asarray(sorted(set(sel)), np.int64)
            rows = self.rows_of(sel)
            desc, pts = self.desc[rows], self.pts[rows]
            off = np.concatenate([[0], np.cumsum([int(self.off[o + 1] - self.off[o]) for o in S])]).astype(np.uint32)
        if len(desc) == 0:
            return np.zeros(len(q) + 1, np.uint32), np.zeros(0, capi.DMATCH_DTYPE), np.zeros((0, 3), np.float32), np.zeros(len(q), np.uint32)
        rc, rp, m, xyz = O.match(desc, off, pts, q, mpq, radius)
        assert rc == 0
        m["imgIdx"] = S.astype(np.int32)[m["imgIdx"]]
        keys = O.knn_keys(desc, q, len(desc)) if keys is None else keys
        return rp, m, xyz, ((keys >> np.uint64(32)) <= np.uint64(radius)).sum(axis=1).astype(np.uint32)


@pytest.fixture(scope="module")
def db():
    return Db(ROWS)


@pytest.fixture(scope="module")
def ctx(db):
    c = capi.Context(0)
    c.db_load(db.desc, db.pts, db.off)
    yield c
    c.close()


class Dev:
    """todhip_match_radius_device through torch tensors; the outputs are prefilled so that untouched slots show"""

    def __init__(self):
        import torch
        self.torch = torch

    def raw(self, c, q, radius, mpq, with_in_radius=True):
        torch = self.torch
        nq = len(q)
        d_q = torch.from_numpy(np.ascontiguousarray(q)).cuda()
        cnt = torch.full((nq,), 77, dtype=torch.int32, device="cuda")
        inr = torch.full((nq,), 78, dtype=torch.int32, device="cuda")
        mm = torch.full((nq * mpq, 4), SENTINEL, dtype=torch.int32, device="cuda")
        xx = torch.full((nq * mpq, 3), -7.5, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        c.match_radius_device(d_q.data_ptr(), nq, radius, mpq, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr(),
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
    for f in FIELDS:
        assert np.array_equal(got[1][f], want[1][f]), (what, f)
    assert np.array_equal(got[2], want[2]), what
    if in_radius:
        assert np.array_equal(got[3], want[3]), what


def prefix(want, nq):
    """the answer for the first nq queries of a call"""
    n = int(want[0][nq])
    return want[0][:nq + 1], want[1][:n], want[2][:n], want[3][:nq]


@pytest.fixture(scope="module")
def wants(db):
    """the oracle's answers for all 70 queries, once per (radius, max_per_query): every nq is a prefix of them"""
    keys = O.knn_keys(db.desc, db.q, len(db.desc))
    return {(r, m): db.want(db.q, r, m, keys=keys) for r in RADII for m in MPQS}


@pytest.mark.parametrize("nq", NQS)
def test_host_and_device_forms_equal_the_oracle(ctx, dev, db, wants, nq):
    n_over = 0
    for radius in RADII:
        for mpq in MPQS:
            want = prefix(wants[(radius, mpq)], nq)
            what = (nq, radius, mpq)
            same(ctx.match_radius(db.q[:nq], radius, mpq), want, what)
            same(dev.match(ctx, db.q[:nq], radius, mpq), want, what)
            n_over += int((want[3] > capi.radius_capacity(mpq)).sum())
            if radius >= 256:
                assert (want[3] == sum(ROWS)).all()
    assert n_over > 0                                                    # the sweep reaches the rescan as well
    same(dev.match(ctx, db.q[:nq], 35, 5, with_in_radius=False), prefix(wants[(35, 5)], nq), in_radius=False)
    cnt = ctx.counters()
    assert cnt.last_nq == nq and cnt.last_k == 5


def test_counters_and_kernel_timing(ctx, db, wants):
    ctx.set_kernel_timing(True)
    try:
        before = ctx.counters().n_match_kernel_launches
        rp, m, _, _ = ctx.match_radius(db.q, 35, 64)
        cnt = ctx.counters()
        assert cnt.last_nq == 70 and cnt.last_k == 64 and cnt.last_matches == len(m) == int(rp[-1])
        assert cnt.n_match_kernel_launches == before + 1 and cnt.last_match_kernel_ms > 0
    finally:
        ctx.set_kernel_timing(False)


# ---------------------------------------------------------------------------------------------------- ties and overflow
@pytest.fixture(scope="module")
def ties():
    """5 000 rows, 3 000 of them copies of one row in two runs (500..1999 and 3000..4499); 70 queries: every tenth is that row, the
    rest are other rows with a few flipped bits"""
    rng = np.random.Generator(np.random.PCG64(99))
    desc = rng.integers(0, 256, (5000, 32), dtype=np.uint8)
    desc[500:2000] = desc[4999]
    desc[3000:4500] = desc[4999]
    pts = rng.standard_normal((5000, 3)).astype(np.float32)
    off = np.array([0, 700, 2500, 5000], np.uint32)
    q = np.zeros((70, 32), np.uint8)
    for i in range(70):
        bits = np.unpackbits(desc[4999 if i % 10 == 0 else int(rng.integers(0, 500))])
        if i % 10:
            bits[rng.choice(256, int(rng.integers(0, 3)), replace=False)] ^= 1
        q[i] = np.packbits(bits)
    c = capi.Context(0)
    c.db_load(desc, pts, off)
    yield c, desc, pts, off, q
    c.close()


@pytest.mark.parametrize("mpq", [1, 8, 64, 1024])
@pytest.mark.parametrize("radius", [1, 256])
def test_ties_beyond_the_buffer_come_back_lowest_rows_first(ties, dev, radius, mpq):
    c, desc, pts, off, q = ties
    C = capi.radius_capacity(mpq)
    # one query equal to the repeated row
    rc, o_rp, o_m, o_xyz = O.match(desc, off, pts, q[:1], mpq, radius)
    n_in = 3001 if radius == 1 else 5000
    want = (o_rp, o_m, o_xyz, np.array([n_in], np.uint32))
    assert rc == 0 and n_in > C                                          # more than the buffer holds: the rescan answers
    same(c.match_radius(q[:1], radius, mpq), want)
    got = dev.match(c, q[:1], radius, mpq)
    same(got, want)
    rows = off[got[1]["imgIdx"]].astype(np.int64) + got[1]["trainIdx"]
    first = (list(range(500, 2000)) + list(range(3000, 4500)) + [4999])[:mpq]
    assert list(rows[:len(first)]) == first and (got[1]["distance"][:len(first)] == 0).all()
    # 70 queries, at radius 1 only every tenth overflows
    want = R.match_radius(desc, off, pts, q, radius, mpq)
    over = want[3] > C
    assert over[::10].all() and (radius == 256 or not np.delete(over, np.arange(0, 70, 10)).any())
    same(c.match_radius(q, radius, mpq), want)
    same(dev.match(c, q, radius, mpq), want)


def test_same_call_three_times_gives_identical_bytes(ties, dev):
    c, _, _, _, q = ties
    for radius, mpq in ((1, 8), (256, 64), (40, 1024)):
        runs = [dev.raw(c, q, radius, mpq) for _ in range(3)]
        for other in runs[1:]:
            for a, b in zip(runs[0], other):
                assert a.tobytes() == b.tobytes(), (radius, mpq)


# ---------------------------------------------------------------------------------------------------- composition
@pytest.mark.parametrize("sel", [[6], [7, 3, 3], [], list(range(len(ROWS)))], ids=["5rows", "unsorted", "nothing", "every"])
def test_selection_equals_the_oracle_on_the_subset(ctx, dev, db, sel):
    ctx.select_objects(sel)
    try:
        for radius, mpq in ((35, 5), (128, 64), (256, 1), (256, 1024)):
            want = db.want(db.q, radius, mpq, sel)
            same(ctx.match_radius(db.q, radius, mpq), want, (sel, radius, mpq))
            same(dev.match(ctx, db.q[:33], radius, mpq), prefix(want, 33), (sel, radius, mpq))
            if not sel:
                assert int(want[0][-1]) == 0 and not want[3].any()
    finally:
        ctx.select_objects(None)


def test_bit_order_ratio_test_and_lsh_change_nothing(dev):
    d2 = Db(ROWS, seed=11, biased=True)                                 # biased leading bits: the order is not the identity
    c = capi.Context(0)
    c.set_db_bit_order(1)
    c.db_load(d2.desc, d2.pts, d2.off)
    try:
        assert not np.array_equal(c.db_bit_order(), np.arange(256))
        cases = ((35, 5), (100, 64), (256, 8))
        wants = {k: d2.want(d2.q, *k) for k in cases}
        for k in cases:
            same(c.match_radius(d2.q, *k), wants[k], ("bit order", k))
        c.select_objects([7, 3])
        same(dev.match(c, d2.q, 100, 64), d2.want(d2.q, 100, 64, [7, 3]), "bit order + selection")
        c.select_objects(None)
        c.set_ratio_test(0.8)
        c.set_lsh(10, 16, 1)
        for k in cases:
            same(c.match_radius(d2.q, *k), wants[k], ("ratio + lsh", k))
            same(dev.match(c, d2.q, *k), wants[k], ("ratio + lsh", k))
    finally:
        c.close()


@pytest.mark.parametrize("rows", [ROWS, [700, 0, 1, 31, 32, 33, 257, 5]], ids=["one-shard-empty", "both-shards"])
def test_two_shards_concatenated_and_sorted_equal_the_unsharded_call(rows):
    d = Db(rows, seed=77)
    ctxs = []
    try:
        for s in range(2):
            c = capi.Context(0)
            c.db_load(d.desc, d.pts, d.off, shard_rank=s, shard_count=2)
            ctxs.append(c)
        one = capi.Context(0)
        ctxs.append(one)
        one.db_load(d.desc, d.pts, d.off)
        assert sum(c.db_info()["shard_rows"] for c in ctxs[:2]) == sum(rows)
        if rows[0] == 700:
            assert all(c.db_info()["shard_rows"] > 0 for c in ctxs[:2])
        for radius, mpq in ((35, 5), (120, 64), (256, 8)):
            whole = one.match_radius(d.q, radius, mpq)
            same(whole, d.want(d.q, radius, mpq))
            parts = [c.match_radius(d.q, radius, mpq) for c in ctxs[:2]]
            ms, xs, rp = [], [], [0]
            for qi in range(len(d.q)):
                m = np.concatenate([p[1][p[0][qi]:p[0][qi + 1]] for p in parts])
                x = np.concatenate([p[2][p[0][qi]:p[0][qi + 1]] for p in parts])
                order = np.lexsort((d.off[m["imgIdx"]].astype(np.int64) + m["trainIdx"], m["distance"]))[:mpq]
                ms.append(m[order]); xs.append(x[order]); rp.append(rp[-1] + len(order))
            merged = (np.asarray(rp, np.uint32), np.concatenate(ms), np.concatenate(xs), parts[0][3] + parts[1][3])
            same(merged, whole, (radius, mpq))
    finally:
        for c in ctxs:
            c.close()


# ---------------------------------------------------------------------------------------------------- tiling
def test_many_tiles_and_query_waves(dev):
    """70 000 random rows x 1 100 queries, radius 100 (about 16 random rows inside per query), 64 per query: several tiles, several
    query waves per tile, a ragged last wave"""
    rng = np.random.Generator(np.random.PCG64(5))
    n, nq, radius, mpq = 70000, 1100, 100, 64
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    pts = rng.standard_normal((n, 3)).astype(np.float32)
    off = np.array([0, 10000, 10001, 69999, 70000], np.uint32)
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    q[::3] = desc[rng.integers(0, n, len(q[::3]))]                      # a third of the queries are rows: distance 0 somewhere
    q[::3, 5] ^= 0x81
    c = capi.Context(0)
    try:
        c.db_load(desc, pts, off)
        host = c.match_radius(q, radius, mpq)
        device = dev.match(c, q, radius, mpq)
    finally:
        c.close()
    same(device, host)
    rp, m, xyz, in_radius = host
    sub = np.concatenate([np.arange(0, 32), np.arange(1068, 1100)])
    rc, o_rp, o_m, o_xyz = O.match(desc, off, pts, q[sub], mpq, radius)
    assert rc == 0
    o_in = (R.distances(desc, q[sub]) <= radius).sum(axis=1)
    for i, qi in enumerate(sub):
        lo, hi = int(rp[qi]), int(rp[qi + 1])
        assert hi - lo == int(o_rp[i + 1] - o_rp[i]) and in_radius[qi] == o_in[i], qi
        for f in FIELDS[1:]:
            assert np.array_equal(m[f][lo:hi], o_m[f][o_rp[i]:o_rp[i + 1]]), (qi, f)
        assert (m["queryIdx"][lo:hi] == qi).all() and np.array_equal(xyz[lo:hi], o_xyz[o_rp[i]:o_rp[i + 1]])
    # the rest by properties: counts, radius, order, the gathered point
    assert np.array_equal(np.diff(rp.astype(np.int64)), np.minimum(in_radius, mpq)) and in_radius[::3].min() >= 1
    assert (m["distance"] <= radius).all() and np.array_equal(m["queryIdx"], np.repeat(np.arange(nq), np.diff(rp.astype(np.int64))))
    rows = off[m["imgIdx"]].astype(np.int64) + m["trainIdx"]
    key = m["distance"].astype(np.int64) << 32 | rows
    inner = np.ones(len(key), bool)
    inner[rp[:-1][rp[:-1] < len(key)]] = False                          # a query's first match has no predecessor
    assert (np.diff(key)[inner[1:]] > 0).all()
    assert np.array_equal(xyz, pts[rows])
    assert np.array_equal(m["distance"], R.POPCOUNT[desc[rows] ^ q[m["queryIdx"]]].sum(axis=1).astype(np.float32))


@pytest.mark.parametrize("n_rows,nqs", [(1, (1, 32, 33, 64, 65, 129, 1025)), (31, (1, 33, 65)), (32, (32, 64, 129)), (33, (1, 33, 65)),
                                        (95, (1, 32, 33, 64, 65, 129, 1025)), (8193, (1, 32, 33, 64, 65, 129))])
def test_steps_tiles_and_query_blocks_at_their_edges(n_rows, nqs):
    """What the DB pass shares with the top-k kernels (match_fp4.h), at the shapes where it can go wrong. Rows: one tile whose last
    32-row step is partial or whole and whose load reaches into the slack behind the rows; 8 193 rows: several tiles, the last a
    single partial step. Queries: two blocks per wave (<= 64), four (<= 1024) and six, each with a ragged last block and with whole
    blocks of padding queries, which repeat query nq - 1. Radius 35: the integer block test; 200: the float one. Against the numpy
    statement of the definition, bit for bit."""
    rng = np.random.Generator(np.random.PCG64(n_rows))
    desc = rng.integers(0, 256, (n_rows, 32), dtype=np.uint8)
    pts = rng.standard_normal((n_rows, 3)).astype(np.float32)
    off = np.array([0, n_rows // 3, n_rows], np.uint32)
    q = rng.integers(0, 256, (max(nqs), 32), dtype=np.uint8)
    for i in range(len(q)):                                             # six of seven queries: a row with 0..20 flipped bits
        if i % 7 != 6:
            bits = np.unpackbits(desc[(i * 37) % n_rows])
            bits[rng.choice(256, i % 21, replace=False)] ^= 1
            q[i] = np.packbits(bits)
    c = capi.Context(0)
    try:
        c.set_matcher_engine("mfma")
        c.db_load(desc, pts, off)
        for radius in (35, 200):
            want = R.match_radius(desc, off, pts, q, radius, 8)
            assert want[3][::7].min() >= 1
            for nq in nqs:
                same(c.match_radius(q[:nq], radius, 8), prefix(want, nq), (n_rows, nq, radius))
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals(ctx, db):
    import ctypes as C
    import torch
    L = capi.lib()
    nq, mpq = 8, 4
    q = np.ascontiguousarray(db.q[:nq])
    rp, inr = np.zeros(nq + 1, np.uint32), np.zeros(nq, np.uint32)
    m, xyz = np.zeros(nq * mpq, capi.DMATCH_DTYPE), np.zeros((nq * mpq, 3), np.float32)
    n = C.c_uint32(nq * mpq)

    def host(h=ctx._h, q_=q.ctypes.data, nq_=nq, radius=35, mpq_=mpq, rp_=rp.ctypes.data, m_=m.ctypes.data, x_=xyz.ctypes.data,
             n_=C.addressof(n), in_=inr.ctypes.data):
        return L.todhip_match_radius(h, q_, nq_, radius, mpq_, rp_, m_, x_, n_, in_)

    assert host() == capi.OK and n.value == rp[nq]
    n.value = nq * mpq
    assert host(in_=None) == capi.OK                                     # in_radius may be NULL
    for bad in (dict(h=None), dict(q_=None), dict(rp_=None), dict(m_=None), dict(x_=None), dict(n_=None), dict(nq_=0), dict(radius=0),
                dict(mpq_=0), dict(mpq_=1025)):
        assert host(**bad) == capi.EINVAL, bad
    # capacity: the needed count comes back, row_ptr and in_radius are filled, matches are not
    want = db.want(q, 256, mpq)
    need = int(want[0][-1])
    assert need == nq * mpq
    rp[:] = 0; inr[:] = 0; m[:] = 0
    n.value = need - 1
    assert host(radius=256) == capi.ECAPACITY and n.value == need
    assert np.array_equal(rp, want[0]) and np.array_equal(inr, want[3]) and not m["distance"].any()
    assert host(radius=256) == capi.OK and n.value == need and np.array_equal(m["trainIdx"], want[1]["trainIdx"])

    d_q = torch.from_numpy(q).cuda()
    cnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
    mm = torch.zeros((nq * mpq, 4), dtype=torch.int32, device="cuda")
    xx = torch.zeros((nq * mpq, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def device(h=ctx._h, q_=d_q.data_ptr(), nq_=nq, radius=35, mpq_=mpq, c_=cnt.data_ptr(), m_=mm.data_ptr(), x_=xx.data_ptr(), in_=None):
        return L.todhip_match_radius_device(h, q_, nq_, radius, mpq_, c_, m_, x_, in_)

    assert device() == capi.OK
    ctx.synchronize()
    for bad in (dict(h=None), dict(q_=None), dict(c_=None), dict(m_=None), dict(x_=None), dict(nq_=0), dict(radius=0), dict(mpq_=0),
                dict(mpq_=1025)):
        assert device(**bad) == capi.EINVAL, bad
    empty = capi.Context(0)
    assert host(h=empty._h) == capi.ENODB and device(h=empty._h) == capi.ENODB
    empty.close()
    fl = capi.Context(0)
    rng = np.random.Generator(np.random.PCG64(5))
    fl.db_load(rng.standard_normal((40, 128)).astype(np.float32), db.pts[:40], np.array([0, 10, 40]))
    assert host(h=fl._h) == capi.EINVAL and device(h=fl._h) == capi.EINVAL
    fl.close()


# ---------------------------------------------------------------------------------------------------- end to end
def test_radius_matches_feed_the_verifier():
    desc, pts, off = synth.make_db(3, per_object=2000)
    fr = synth.make_frame(desc, pts, off, 500, frame=0, visible_object=1)
    c = capi.Context(0)
    try:
        spans = c.db_load(desc, pts, off)
        knn = c.match(fr["q_desc"], 5, 35)
        rad = c.match_radius(fr["q_desc"], 35, 5)
        same(rad, knn, in_radius=False)                                  # identical by definition
        assert np.array_equal(np.minimum(rad[3], 5), np.diff(rad[0].astype(np.int64)))

        def verify(mt):
            return c.verify(fr["kp_xy"], fr["cloud"], mt[0], mt[1], mt[2], spans, 8, 2500, 0.01, capi.rng_new(1))

        p_knn, p_rad = verify(knn), verify(rad)
        assert len(p_knn) >= 1 and [p["object"] for p in p_knn] == [p["object"] for p in p_rad]
        for a, b in zip(p_knn, p_rad):
            assert np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"]) and np.array_equal(a["inliers"], b["inliers"])
        wide = c.match_radius(fr["q_desc"], 35, 64)
        same(wide, R.match_radius(desc, off, pts, fr["q_desc"], 35, 64))
        p_wide = verify(wide)
    finally:
        c.close()
    # the reference path on the 64-match input, and every pose of the 5-match run found again
    rc, o_poses, _ = O.verify(fr["kp_xy"], fr["cloud"], wide[0], wide[1], wide[2], O.spans(pts, off), 8, 2500, 0.01, O.rng_new(1))
    assert rc == 0 and [p["object"] for p in p_wide] == [p["object"] for p in o_poses]
    for g, o in zip(p_wide, o_poses):
        assert np.abs(g["R"] - o["R"]).max() < 1e-3 and np.abs(g["t"] - o["t"]).max() < 1e-3
    for a in p_knn:
        assert any(b["object"] == a["object"] and np.abs(a["R"] - b["R"]).max() < 1e-3 and np.abs(a["t"] - b["t"]).max() < 1e-3
                   for b in p_wide), a["object"]
