"""The exact k-NN search over a DB of 64-byte (512-bit) binary descriptors (include/todhip.h; tod_amd/csrc/match_wide.hip)
on the GPU, bit for bit against the oracle (oracle_lib.match at desc_bytes = 64): queryIdx, trainIdx, imgIdx, distance, the points,
row_ptr. Shapes are the smallest at which the kernel can go wrong: objects of 0, 1, 31, 32, 33, 257, 5 and 700 rows (short of, on
and past a 32-row step), 1 / 32 / 33 / 64 / 70 queries (two query blocks per wave up to 64 queries; beyond, four for k <= 3 and
two from k = 4 on), radii on both sides of the integer block test (255 / 256) and of "no cut" (511 / 512). The neighbours are
planted (match_wide_ref.WideDb): random 512-bit rows are never within 200 bits of each other."""
import ctypes as C

import numpy as np
import pytest

import match_wide_ref as W
import oracle_lib as O
from tod_amd import capi, synth

pytestmark = pytest.mark.gpu

NQS = (1, 32, 33, 64, 70)
KS = (1, 2, 3, 4, 5, 6, 7, 8)
RADII = (1, 35, 70, 255, 256, 300, 511, 512, 1000)
FIELDS = ("queryIdx", "trainIdx", "imgIdx", "distance")
SENTINEL = 0x5A5A5A5A


def oracle(desc, off, pts, q, k, radius, ratio=0.0):
    rc, rp, m, xyz = O.match(desc, off, pts, q, k, radius, ratio)
    assert rc == 0
    return rp, m, xyz


def want_of(d, sel, q, k, radius, ratio=0.0):
    """the definition under a selection: the oracle on the subset DB, imgIdx in the full DB's numbering"""
    if sel is None:
        return oracle(d.desc, d.off, d.pts, q, k, radius, ratio)
    S, desc, pts, off = d.subset(sel)
    if len(desc) == 0:
        return np.zeros(len(q) + 1, np.uint32), np.zeros(0, capi.DMATCH_DTYPE), np.zeros((0, 3), np.float32)
    rp, m, xyz = oracle(desc, off, pts, q, k, radius, ratio)
    m["imgIdx"] = S[m["imgIdx"]]
    return rp, m, xyz


def same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), what
    for f in FIELDS:
        assert np.array_equal(got[1][f], want[1][f]), (what, f)
    assert np.array_equal(got[2], want[2]), what


def prefix(want, nq):
    n = int(want[0][nq])
    return want[0][:nq + 1], want[1][:n], want[2][:n]


class Dev:
    """todhip_match_device (or a merge of shard keys) through torch tensors; the outputs are prefilled so that untouched slots show"""

    def __init__(self):
        import torch
        self.torch = torch

    def raw(self, c, q, k, radius, fn=None):
        torch = self.torch
        nq = len(q)
        d_q = torch.from_numpy(np.ascontiguousarray(q)).cuda()
        cnt = torch.full((nq,), 77, dtype=torch.int32, device="cuda")
        mm = torch.full((nq * k, 4), SENTINEL, dtype=torch.int32, device="cuda")
        xx = torch.full((nq * k, 3), -7.5, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        (fn or c.match_device)(d_q.data_ptr(), nq, k, radius, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr())
        c.synchronize()
        return cnt.cpu().numpy(), mm.cpu().numpy(), xx.cpu().numpy()

    def match(self, c, q, k, radius, fn=None):
        nq = len(q)
        cnt, mm, xx = self.raw(c, q, k, radius, fn)
        cnt = cnt.astype(np.int64)
        keep = np.arange(k)[None, :] < cnt[:, None]
        assert (mm.reshape(nq, k, 4)[~keep] == SENTINEL).all() and (xx.reshape(nq, k, 3)[~keep] == -7.5).all(), "slots behind counts[q] were written"
        return np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32), mm.view(capi.DMATCH_DTYPE).reshape(nq, k)[keep], xx.reshape(nq, k, 3)[keep]


@pytest.fixture(scope="module")
def dev():
    return Dev()


@pytest.fixture(scope="module")
def db():
    return W.WideDb()


@pytest.fixture(scope="module")
def ctx(db):
    c = capi.Context(0)
    c.db_load(db.desc, db.pts, db.off)
    yield c
    c.close()


@pytest.fixture(scope="module")
def wants(db):
    """the oracle's answers for all 70 queries, once per (k, radius): every nq is a prefix of them"""
    return {(k, r): oracle(db.desc, db.off, db.pts, db.q, k, r) for k in KS for r in RADII}


# ---------------------------------------------------------------------------------------------------- 1. the load
def test_a_64_byte_db_loads_and_reports_its_rows(db):
    c = capi.Context(0)
    try:
        spans = c.db_load(db.desc, db.pts, db.off)
        assert c.db_info() == dict(total_rows=sum(W.ROWS), shard_first=0, shard_rows=sum(W.ROWS), n_objs=len(W.ROWS))
        assert c.desc_bytes() == 64 and np.array_equal(spans, O.spans(db.pts, db.off))
        same(c.match(db.q, 5, 70), oracle(db.desc, db.off, db.pts, db.q, 5, 70))
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------- 2. small shapes
def test_the_planted_neighbours_are_what_the_docstring_says(db, wants):
    rp, m, _ = wants[(2, 1000)]
    n = sum(W.ROWS)
    rows = db.off[m["imgIdx"]].astype(np.int64) + m["trainIdx"]
    assert list(rows[rp[0]:rp[0] + 1]) == [n - 100] and m["distance"][rp[0]] == 3          # flips in bytes 32..63 only
    assert list(rows[rp[1]:rp[1] + 1]) == [n - 101] and m["distance"][rp[1]] == 3          # flips in bytes 0..31 only
    d2 = W.distances(db.desc, db.q[2:3])[0]
    assert d2[n - 102] == 512 and d2.max() == 512                                             # the complement
    assert list(rows[rp[3]:rp[4]]) == [n - 7, n - 300] and list(m["distance"][rp[3]:rp[4]]) == [0, 1]   # bit 511 alone


@pytest.mark.parametrize("nq", NQS)
def test_host_and_device_forms_equal_the_oracle(ctx, dev, db, wants, nq):
    for k in KS:
        for radius in RADII:
            want = prefix(wants[(k, radius)], nq)
            same(ctx.match(db.q[:nq], k, radius), want, (nq, k, radius, "host"))
            same(dev.match(ctx, db.q[:nq], k, radius), want, (nq, k, radius, "device"))
    cnt = ctx.counters()
    assert cnt.last_nq == nq and cnt.last_k == 8 and cnt.last_block_split == 4


def test_the_farthest_row_comes_back_with_distance_512(db):
    """a one-row DB and the complement of its row: distance 512 is a distance like any other, and radius 511 cuts it"""
    n = sum(W.ROWS)
    c = capi.Context(0)
    try:
        c.db_load(db.desc[n - 102:n - 101], db.pts[:1], np.array([0, 1], np.uint32))
        rp, m, xyz = c.match(db.q[2:3], 3, 512)
        assert list(rp) == [0, 1] and m["distance"][0] == 512.0 and m["trainIdx"][0] == 0 and np.array_equal(xyz[0], db.pts[0])
        assert list(c.match(db.q[2:3], 3, 511)[0]) == [0, 0]
    finally:
        c.close()


def test_kernel_timing_brackets_the_wide_pass(ctx, db):
    ctx.set_kernel_timing(True)
    try:
        before = ctx.counters().n_match_kernel_launches
        ctx.match(db.q, 2, 70)
        cnt = ctx.counters()
        assert cnt.n_match_kernel_launches == before + 1 and cnt.last_match_kernel_ms > 0
    finally:
        ctx.set_kernel_timing(False)


# ---------------------------------------------------------------------------------------------------- 3. ties
@pytest.fixture(scope="module")
def ties():
    """5 000 rows, 3 000 of them copies of one row in two runs (500..1999 and 3000..4499); 70 queries: every tenth is that row, the
    rest are other rows with a few flipped bits"""
    rng = np.random.Generator(np.random.PCG64(99))
    desc = rng.integers(0, 256, (5000, 64), dtype=np.uint8)
    desc[500:2000] = desc[4999]
    desc[3000:4500] = desc[4999]
    pts = rng.standard_normal((5000, 3)).astype(np.float32)
    off = np.array([0, 700, 2500, 5000], np.uint32)
    q = np.zeros((70, 64), np.uint8)
    for i in range(70):
        q[i] = desc[4999] if i % 10 == 0 else W.flip(desc[int(rng.integers(0, 500))], rng.choice(512, int(rng.integers(0, 3)), replace=False))
    c = capi.Context(0)
    c.db_load(desc, pts, off)
    yield c, desc, pts, off, q
    c.close()


def test_ties_go_to_the_lowest_rows(ties, dev):
    c, desc, pts, off, q = ties
    for k, radius in ((8, 70), (8, 512), (3, 1)):
        want = oracle(desc, off, pts, q, k, radius)
        got = dev.match(c, q, k, radius)
        same(got, want, (k, radius))
        same(c.match(q, k, radius), want, (k, radius))
        rows = off[got[1]["imgIdx"]].astype(np.int64) + got[1]["trainIdx"]
        assert list(rows[:k]) == list(range(500, 500 + k)) and (got[1]["distance"][:k] == 0).all()


def test_same_call_three_times_gives_identical_bytes(ties, dev):
    c, _, _, _, q = ties
    for k, radius in ((8, 70), (2, 512)):
        runs = [dev.raw(c, q, k, radius) for _ in range(3)]
        for other in runs[1:]:
            for a, b in zip(runs[0], other):
                assert a.tobytes() == b.tobytes(), (k, radius)


# ---------------------------------------------------------------------------------------------------- 4. tiling
@pytest.mark.parametrize("n,nq", [(70000, 1100), (2049, 2100)])
def test_many_tiles_and_query_waves(dev, n, nq):
    """Many tiles, both numbers of query blocks per wave (k = 2: four, k = 5: two), a ragged last wave, the bound exchange between
    tiles (a third of the queries have a planted row, so their lists fill and publish), a last tile of one partial step (2 049)."""
    rng = np.random.Generator(np.random.PCG64(n))
    desc = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    pts = rng.standard_normal((n, 3)).astype(np.float32)
    off = np.array([0, n // 7, n // 7 + 1, n - 1, n], np.uint32)
    q = rng.integers(0, 256, (nq, 64), dtype=np.uint8)
    src = rng.integers(0, n, len(q[::3]))
    q[::3] = desc[src]
    q[::3, 5] ^= 0x81
    q[::3, 60] ^= 0x18
    q[::6] = desc[n - 1 - (np.arange(len(q[::6])) % 40)]                  # some in the last tile's last rows, at distance 0
    c = capi.Context(0)
    try:
        c.db_load(desc, pts, off)
        for k in (2, 5):
            for radius in (70, 512):
                want = oracle(desc, off, pts, q, k, radius)
                same(c.match(q, k, radius), want, (n, nq, k, radius, "host"))
                same(dev.match(c, q, k, radius), want, (n, nq, k, radius, "device"))
    finally:
        c.close()


def test_the_wide_pass_at_its_edges(dev):
    """The step loop of the DB pass (block_step_loop, match_fp4.h) where it turns: DBs of 1, 31, 32, 33 and 65 rows (a partial step,
    exactly one, one and a row, two and a row: the block carried from step to step and the drain), 1 / 33 / 65 / 129 queries (two query
    blocks per wave up to 64 queries; beyond, four for k <= 3 and two from k = 4 on, a last wave of one query), k on both sides of
    that switch, a radius that cuts and one that does not (every row comes back, ties by row). Bit for bit against the numpy
    definition (match_wide_ref.match); most queries are rows with 0..80 flipped bits, every seventh is random. One context, reloaded
    per DB size."""
    c = capi.Context(0)
    try:
        for n in (1, 31, 32, 33, 65):
            rng = np.random.Generator(np.random.PCG64(4000 + n))
            desc = rng.integers(0, 256, (n, 64), dtype=np.uint8)
            pts = rng.standard_normal((n, 3)).astype(np.float32)
            off = np.array([0, n // 2, n], np.uint32)
            q = rng.integers(0, 256, (129, 64), dtype=np.uint8)
            for i in range(len(q)):
                if i % 7 != 6:
                    q[i] = W.flip(desc[int(rng.integers(0, n))], rng.choice(512, int(rng.integers(0, 81)), replace=False))
            c.db_load(desc, pts, off)
            for k in (1, 3, 4, 8):
                for radius in (70, 512):
                    want_all = W.match(desc, off, pts, q, k, radius)
                    assert want_all[0][-1] > 0
                    for nq in (1, 33, 65, 129):
                        want = prefix(want_all, nq)
                        same(c.match(q[:nq], k, radius), want, (n, nq, k, radius, "host"))
                        same(dev.match(c, q[:nq], k, radius), want, (n, nq, k, radius, "device"))
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------- 5. shards and selections
def shard_ctxs(d, n_shards):
    ctxs = []
    for s in range(n_shards):
        c = capi.Context(0)
        c.db_load(d.desc, d.pts, d.off, shard_rank=s, shard_count=n_shards)
        ctxs.append(c)
    return ctxs


def sharded_match(dev, ctxs, q, k, radius):
    import torch
    n_shards, nq = len(ctxs), len(q)
    d_q = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    keys_all = torch.zeros((n_shards, nq, k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    for s, c in enumerate(ctxs):
        c.match_shard_device(d_q.data_ptr(), nq, k, radius, keys_all[s].data_ptr())
        c.synchronize()
    return dev.match(ctxs[-1], q, k, radius,
                     fn=lambda q_, n_, k_, r_, cn, mm, xx: ctxs[-1].merge_shards_device(keys_all.data_ptr(), n_shards, n_, k_, r_, cn, mm, xx))


def test_three_shards_equal_the_unsharded_call_and_the_oracle(ctx, dev, db, wants):
    ctxs = shard_ctxs(db, 3)
    try:
        rows = [c.db_info()["shard_rows"] for c in ctxs]
        assert sum(rows) == sum(W.ROWS) and 0 in rows                     # one shard is empty
        for k, radius in ((2, 70), (5, 512), (8, 35)):
            got = sharded_match(dev, ctxs, db.q, k, radius)
            same(got, wants[(k, radius)], (k, radius))
            same(got, ctx.match(db.q, k, radius), (k, radius))
        # the sharded and selected combination: some selections leave two shards without a selected row
        for sel in ([7], [5, 2, 2, 7], [1], [], None):
            for c in ctxs:
                c.select_objects(sel)
            for k, radius in ((2, 70), (5, 512)):
                same(sharded_match(dev, ctxs, db.q, k, radius), want_of(db, sel, db.q, k, radius), (sel, k, radius))
    finally:
        for c in ctxs:
            c.close()


def test_selection_equals_the_oracle_on_the_subset(ctx, dev, db, wants):
    try:
        for sel in ([5, 7], [7, 3, 3], [6], list(range(len(W.ROWS)))):
            ctx.select_objects(sel)
            n_sel = sum(W.ROWS[o] for o in set(sel))
            assert ctx.selection() == dict(n_objs=len(set(sel)), rows=n_sel, shard_rows=n_sel)
            for k, radius in ((2, 70), (5, 512), (8, 255)):
                want = want_of(db, sel, db.q, k, radius)
                same(ctx.match(db.q, k, radius), want, (sel, k, radius))
                same(dev.match(ctx, db.q[:33], k, radius), prefix(want, 33), (sel, k, radius))
        ctx.select_objects([])
        rp, m, _ = ctx.match(db.q, 5, 512)
        assert not rp.any() and len(m) == 0
        ctx.select_objects(None)
        same(ctx.match(db.q, 5, 512), wants[(5, 512)])
    finally:
        ctx.select_objects(None)


# ---------------------------------------------------------------------------------------------------- 6. ratio test
def test_ratio_test_sees_the_true_two_nearest(ctx, dev, db, ties):
    tc, t_desc, t_pts, t_off, t_q = ties
    for c, d_, off, pts, q in ((ctx, db.desc, db.off, db.pts, db.q), (tc, t_desc, t_off, t_pts, t_q)):
        c.set_ratio_test(0.8)
        try:
            for k, radius in ((1, 70), (5, 70), (5, 512), (1, 1)):
                want = oracle(d_, off, pts, q, k, radius, 0.8)
                same(c.match(q, k, radius), want, (k, radius))
                same(dev.match(c, q, k, radius), want, (k, radius))
        finally:
            c.set_ratio_test(0.0)
    # a query whose two nearest tie (the repeated row: 0 < 0.8 * 0 fails) keeps nothing; one with a single near row keeps it
    tc.set_ratio_test(0.8)
    try:
        rp, m, _ = tc.match(t_q, 5, 70)
        assert rp[1] == rp[0] and rp[2] > rp[1]
    finally:
        tc.set_ratio_test(0.0)


# ---------------------------------------------------------------------------------------------------- 7. refusals and no-ops
def test_what_a_64_byte_db_refuses(ctx, db, wants):
    import torch
    L = capi.lib()
    nq, k = 8, 4
    q = np.ascontiguousarray(db.q[:nq])
    rp, inr = np.zeros(nq + 1, np.uint32), np.zeros(nq, np.uint32)
    m, xyz = np.zeros(nq * 64, capi.DMATCH_DTYPE), np.zeros((nq * 64, 3), np.float32)
    n = C.c_uint32(nq * 64)
    d_q = torch.from_numpy(q).cuda()
    cnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
    mm = torch.zeros((nq * 64, 4), dtype=torch.int32, device="cuda")
    xx = torch.zeros((nq * 64, 3), dtype=torch.float32, device="cuda")
    keys = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    h = ctx._h
    # the radius search and the float search
    assert L.todhip_match_radius(h, q.ctypes.data, nq, 35, 64, rp.ctypes.data, m.ctypes.data, xyz.ctypes.data, C.addressof(n), inr.ctypes.data) == capi.EINVAL
    assert L.todhip_match_radius_device(h, C.c_void_p(d_q.data_ptr()), nq, 35, 64, C.c_void_p(cnt.data_ptr()), C.c_void_p(mm.data_ptr()),
                                        C.c_void_p(xx.data_ptr()), None) == capi.EINVAL
    qf = np.zeros((nq, 128), np.float32)
    with pytest.raises(capi.TodError) as e:
        ctx.match_l2(qf, k, 1.0)
    assert e.value.status == capi.EINVAL
    with pytest.raises(capi.TodError) as e:
        ctx.match_l2_device(d_q.data_ptr(), nq, k, 1.0, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr())
    assert e.value.status == capi.EINVAL
    # radius 0 and k out of range, as on a 32-byte DB
    assert L.todhip_match(h, q.ctypes.data, nq, k, 0, rp.ctypes.data, m.ctypes.data, xyz.ctypes.data) == capi.EINVAL
    assert L.todhip_match(h, q.ctypes.data, nq, 9, 70, rp.ctypes.data, m.ctypes.data, xyz.ctypes.data) == capi.EINVAL
    # the LSH mode: every match form refuses, and the exact search is back when it is switched off
    ctx.set_lsh(10, 16, 1)
    try:
        rp[:] = 0x77777777
        assert L.todhip_match(h, q.ctypes.data, nq, k, 70, rp.ctypes.data, m.ctypes.data, xyz.ctypes.data) == capi.EINVAL
        assert (rp == 0x77777777).all()
        assert L.todhip_match_device(h, C.c_void_p(d_q.data_ptr()), nq, k, 70, C.c_void_p(cnt.data_ptr()), C.c_void_p(mm.data_ptr()),
                                     C.c_void_p(xx.data_ptr())) == capi.EINVAL
        assert L.todhip_match_shard_device(h, C.c_void_p(d_q.data_ptr()), nq, k, 70, C.c_void_p(keys.data_ptr())) == capi.EINVAL
    finally:
        ctx.set_lsh(0)
    same(ctx.match(db.q, 5, 70), wants[(5, 70)])
    # queries of another width than the DB's are refused by the binding
    with pytest.raises(capi.TodError) as e:
        ctx.match(db.q[:, :32], 5, 70)
    assert e.value.status == capi.EINVAL
    # the pipeline's DB stays 32 bytes wide
    p = capi.Pipeline(0)
    try:
        assert p.db_load(db.desc, db.pts, db.off) == capi.EINVAL
    finally:
        p.close()


def test_bit_order_engine_and_split_setters_change_nothing(dev, db, wants):
    c = capi.Context(0)
    try:
        c.set_db_bit_order(1)
        c.db_load(db.desc, db.pts, db.off)
        assert np.array_equal(c.db_bit_order(), np.arange(256))           # the rows stay in identity order
        same(c.match(db.q, 5, 70), wants[(5, 70)])
        for engine in ("valu", "mfma", "auto"):
            for split in (0, 2, 3, -1):
                c.set_matcher_engine(engine)
                c.set_matcher_block_split(split)
                for k, radius in ((2, 35), (5, 70)):
                    same(c.match(db.q, k, radius), wants[(k, radius)], (engine, split, k, radius))
                    same(dev.match(c, db.q[:33], k, radius), prefix(wants[(k, radius)], 33), (engine, split, k, radius))
                assert c.counters().last_block_split == 4
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------- 8. one context, reloaded
def test_one_context_reloaded_with_other_widths(dev):
    d64, d32 = W.WideDb(seed=5), W.WideDb(width=32, seed=6)
    rng = np.random.Generator(np.random.PCG64(8))
    f_desc = rng.standard_normal((sum(W.ROWS), 128)).astype(np.float32)
    f_q = f_desc[::17] + 0.01 * rng.standard_normal((len(f_desc[::17]), 128)).astype(np.float32)
    c = capi.Context(0)
    try:
        for step in ("32", "64", "float", "64", "32"):
            if step == "float":
                c.db_load(f_desc, d64.pts, d64.off)
                assert c.desc_bytes() == 512
                rc, rp, m, xyz = O.l2_match(f_desc, d64.off, d64.pts, f_q, 5, 100.0)
                assert rc == 0
                same(c.match_l2(f_q, 5, 100.0), (rp, m, xyz), step)
                continue
            d, other = (d64, d32) if step == "64" else (d32, d64)
            c.db_load(d.desc, d.pts, d.off)
            assert c.desc_bytes() == int(step)
            c.select_objects([7, 2])                                       # a view of this width, gone with the next load
            same(c.match(d.q, 5, 70), want_of(d, [7, 2], d.q, 5, 70), step)
            c.select_objects(None)
            for k, radius in ((2, 35), (5, 70), (8, 1000)):
                want = oracle(d.desc, d.off, d.pts, d.q, k, radius)
                same(c.match(d.q, k, radius), want, (step, k, radius))
                same(dev.match(c, d.q, k, radius), want, (step, k, radius))
            with pytest.raises(capi.TodError) as e:
                c.match(other.q, 5, 70)
            assert e.value.status == capi.EINVAL
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------- 9. into the verifier
def test_wide_matches_feed_the_verifier():
    desc, pts, off = synth.make_db_ragged([3000, 10, 2500], desc_bytes=64)
    fr = synth.make_frame(desc, pts, off, 500, visible_object=2)
    c = capi.Context(0)
    try:
        spans = c.db_load(desc, pts, off)
        got = c.match(fr["q_desc"], 5, 70)
        poses = c.verify(fr["kp_xy"], fr["cloud"], got[0], got[1], got[2], spans, 8, 2500, 0.01, capi.rng_new(1))
    finally:
        c.close()
    want = oracle(desc, off, pts, fr["q_desc"], 5, 70)
    same(got, want)
    rc, o_poses, _ = O.verify(fr["kp_xy"], fr["cloud"], want[0], want[1], want[2], O.spans(pts, off), 8, 2500, 0.01, O.rng_new(1))
    assert rc == 0 and len(poses) == len(o_poses) == 1 and poses[0]["object"] == o_poses[0]["object"] == 2
    assert np.abs(poses[0]["R"] - o_poses[0]["R"]).max() < 1e-3 and np.abs(poses[0]["t"] - o_poses[0]["t"]).max() < 1e-3
