"""todhip_set_db_bit_order on the GPU: the order is its definition (tests/bit_order_ref.py), every match form returns what the
unordered DB returns (and the CPU oracle), and the order does what it is for: on a DB whose first 128 stored positions say nothing,
the matrix-core engine's 2-split blocks stop early once the informative positions come first.

The "biased DB": dwords 0, 1, 4, 5 -- the positions a 2-split block evaluates -- are drawn once and shared by every row and every
query; dwords 2, 3, 6, 7 are independent and uniform; a few rows are near-duplicates of queries, so that matches exist."""
import numpy as np
import pytest

import bit_order_ref as R
import oracle_lib as O
from tod_amd import capi

pytestmark = pytest.mark.gpu

FIELDS = ("queryIdx", "trainIdx", "imgIdx", "distance")
IDENTITY = np.arange(256, dtype=np.uint8)
PLANTED = (0, 1, 5, 31, 32, 33, 128, 200, 255, 256, 640, 999)


def make_db(n, nq, seed, biased, sizes=None):
    """-> desc u8[n, 32], pts f32[n, 3], off, q u8[nq, 32]; query j of PLANTED has two near rows (2 and 5 bits away)"""
    rng = np.random.default_rng(seed)
    shared = rng.integers(0, 2 ** 32, 8, dtype=np.uint32)

    def rows(m):
        w = rng.integers(0, 2 ** 32, (m, 8), dtype=np.uint32)
        if biased:
            w[:, [0, 1, 4, 5]] = shared[[0, 1, 4, 5]]
        return w

    desc, q = rows(n), rows(nq)
    free = rng.permutation(n)
    for i, j in enumerate(x for x in PLANTED if x < nq):
        for t, flips in enumerate((0x00000003, 0x0001F000)):
            if 2 * i + t < n:
                desc[free[2 * i + t]] = q[j]
                desc[free[2 * i + t], 2 + 4 * t] ^= flips            # in an independent dword (2 or 6)
    pts = rng.standard_normal((n, 3)).astype(np.float32)
    if sizes is None:
        sizes = [n]
    assert sum(sizes) == n
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return desc.view(np.uint8).reshape(n, 32), pts, off, q.view(np.uint8).reshape(nq, 32)


RAGGED = [700, 1, 0, 333, 2049, 13, 1000]                             # 4 096 rows in 7 objects


def same(a, b):
    assert np.array_equal(a[0], b[0])
    for f in FIELDS:
        assert np.array_equal(a[1][f], b[1][f]), f
    assert np.array_equal(a[2], b[2])


def match_device(ctx, q, k, radius):
    """todhip_match_device in CSR form; the caller's query buffer must come back unchanged"""
    import torch
    nq = len(q)
    d_q = torch.from_numpy(q.copy()).cuda()
    cnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
    mm = torch.zeros((nq * k, 4), dtype=torch.int32, device="cuda")
    xx = torch.zeros((nq * k, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.match_device(d_q.data_ptr(), nq, k, radius, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr())
    ctx.synchronize()
    assert np.array_equal(d_q.cpu().numpy(), q)
    return csr(cnt, mm, xx, nq, k)


def csr(cnt, mm, xx, nq, k):
    cnt = cnt.cpu().numpy()
    keep = np.arange(k)[None, :] < cnt[:, None]
    m = mm.cpu().numpy().view(capi.DMATCH_DTYPE).reshape(nq, k)[keep]
    xyz = xx.cpu().numpy().reshape(nq, k, 3)[keep]
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32), m, xyz


# ------------------------------------------------------------------------------------------------ 1. the order is the definition
@pytest.fixture(scope="module")
def ctx_on():
    c = capi.Context(0)
    c.set_db_bit_order(1)
    yield c
    c.close()


@pytest.mark.parametrize("n", [1, 31, 1000, 70001])
def test_order_equals_the_definition(ctx_on, n):
    """70 001 rows: the sampling path (65 536 of them, row floor(i n / S)), n no multiple of anything. The DB is the biased
    one (constant positions: rejected), and a few positions are noisy copies of others (correlations either side of 1/2)."""
    desc, pts, off, _ = make_db(n, 4, 100 + n, biased=True)
    rng = np.random.default_rng(n)
    bits = R.bits_of(desc)
    for b, a, flip in ((70, 100, 0.05), (71, 100, 0.24), (72, 100, 0.26), (200, 201, 0.10)):
        bits[:, b] = bits[:, a] ^ (rng.random(n) < flip)
    desc = np.packbits(bits, axis=1, bitorder="little")
    ctx_on.db_load(desc, pts, off)
    got = ctx_on.db_bit_order()
    assert got.dtype == np.uint8 and sorted(got.tolist()) == list(range(256))
    assert np.array_equal(got, R.order_of(desc))
    if n >= 1000:                                                        # the constant dwords went to the back: positions of dwords 2, 6, 3, 7
        assert set(int(b) // 32 for p in (2, 3, 6, 7) for b in got[32 * p:32 * p + 32]) == {0, 1, 4, 5}


def test_identical_rows_mode_0_and_a_second_load(ctx_on):
    desc, pts, off, q = make_db(500, 40, 7, biased=False)
    flat = np.tile(desc[:1], (500, 1))
    ctx_on.db_load(flat, pts, off)                                      # nothing varies: all rejected, candidate order by index
    want = np.zeros(256, np.uint8)
    for r in range(256):
        want[32 * R.E[r // 32] + r % 32] = r
    assert np.array_equal(ctx_on.db_bit_order(), want) and np.array_equal(want, R.order_of(flat))
    ctx_on.db_load(desc, pts, off)                                      # other data: another order
    first = ctx_on.db_bit_order()
    assert np.array_equal(first, R.order_of(desc)) and not np.array_equal(first, want)
    ref = O.match(desc, off, pts, q, 2, 55)[1:]
    same(ctx_on.match(q, 2, 55), ref)
    c = capi.Context(0)
    assert np.array_equal(c.db_bit_order(), IDENTITY)                   # nothing loaded
    c.db_load(desc, pts, off)
    assert np.array_equal(c.db_bit_order(), IDENTITY)                   # never set
    for bad in (-1, 2, 7):
        with pytest.raises(capi.TodError) as e:
            c.set_db_bit_order(bad)
        assert e.value.status == capi.EINVAL
    assert capi.lib().todhip_db_bit_order(c._h, None) == capi.EINVAL
    c.set_db_bit_order(1)
    assert np.array_equal(c.db_bit_order(), IDENTITY)                   # applies to the loads that follow
    c.db_load(desc, pts, off)
    assert np.array_equal(c.db_bit_order(), first)
    c.set_db_bit_order(0)
    assert np.array_equal(c.db_bit_order(), first)                      # the resident DB keeps its order until the next load
    same(c.match(q, 2, 55), ref)
    c.db_load(desc, pts, off)
    assert np.array_equal(c.db_bit_order(), IDENTITY)
    same(c.match(q, 2, 55), ref)
    c.close()
    ctx_on.db_load(np.zeros((0, 32), np.uint8), np.zeros((0, 3), np.float32), [0, 0])   # an empty shard: nothing to order
    assert np.array_equal(ctx_on.db_bit_order(), IDENTITY)


# ------------------------------------------------------------------------------------------------ 2. exactness
# every value of every axis at least once: engine, block split, nq, k, radius
CONFIGS = [("valu", -1, 1, 1, 35), ("valu", -1, 33, 5, 300), ("valu", -1, 1000, 2, 55), ("valu", -1, 129, 8, 35),
           ("mfma", 0, 32, 2, 35), ("mfma", 2, 33, 1, 55), ("mfma", 3, 129, 5, 35), ("mfma", -1, 256, 8, 300),
           ("mfma", 2, 1000, 2, 35), ("mfma", -1, 1, 5, 55), ("mfma", 3, 256, 2, 55), ("mfma", 0, 1000, 5, 300)]


@pytest.fixture(scope="module", params=["biased", "uniform"])
def pair(request):
    """(DB, queries, a context with the order on, one with it off)"""
    db = make_db(4096, 1000, 11 if request.param == "biased" else 12, biased=request.param == "biased", sizes=RAGGED)
    on, offc = capi.Context(0), capi.Context(0)
    on.set_db_bit_order(1)
    sp_on, sp_off = on.db_load(*db[:3]), offc.db_load(*db[:3])
    assert np.array_equal(sp_on, sp_off)
    assert not np.array_equal(on.db_bit_order(), IDENTITY) and np.array_equal(offc.db_bit_order(), IDENTITY)
    yield db, on, offc
    on.close()
    offc.close()


@pytest.mark.parametrize("engine,split,nq,k,radius", CONFIGS)
def test_results_equal_the_unordered_db_and_the_oracle(pair, engine, split, nq, k, radius):
    (desc, pts, off, q_all), on, offc = pair
    q = q_all[:nq]
    rc, *ref = O.match(desc, off, pts, q, k, radius)
    assert rc == 0 and len(ref[1]) >= 1                                  # (query 0 has planted neighbours)
    for c in (on, offc):
        c.set_matcher_engine(engine)
        c.set_matcher_block_split(split)
    same(offc.match(q, k, radius), ref)
    same(on.match(q, k, radius), ref)
    same(match_device(on, q, k, radius), ref)


# ------------------------------------------------------------------------------------------------ 3. it does what it is for
def split2_fraction(order_on, desc, pts, off, q):
    c = capi.Context(0)
    c.set_db_bit_order(1 if order_on else 0)
    c.set_matcher_engine("mfma")
    c.set_matcher_block_split(2)
    c.db_load(desc, pts, off)
    res = [c.match(q, 2, 35) for _ in range(4)]                          # the counters are as of the last report read: three measured
    cnt = c.counters()                                                   # launches and one further launch that reads their report
    c.close()
    assert cnt.last_block_split == 2 and cnt.k4x_half_blocks > 0
    return cnt.k4x_half_blocks_completed / cnt.k4x_half_blocks, res[-1]


def test_two_split_blocks_stop_early_once_the_informative_bits_come_first():
    """Order off: the first 128 stored positions are identical in every pair, every block's partial distance is 0 and every block goes
    on (>= 0.99). Order on: the 128 independent bits come first; a pair survives them with P(Binomial(128, 1/2) <= 35) ~ 3e-7, a
    block of 1 024 pairs with ~ 3e-4, plus the planted matches: <= 0.05 is two orders above that. Both bounds are derived."""
    desc, pts, off, q = make_db(32768, 256, 21, biased=True)
    f_off, r_off = split2_fraction(False, desc, pts, off, q)
    f_on, r_on = split2_fraction(True, desc, pts, off, q)
    print("blocks that went on: order off %.5f, order on %.5f" % (f_off, f_on))
    same(r_on, r_off)
    assert len(r_on[1]) >= 2 * len([x for x in PLANTED if x < 256])
    assert f_off >= 0.99
    assert f_on <= 0.05


# ------------------------------------------------------------------------------------------------ 4. sharded
def test_sharded_with_an_order_per_shard_equals_unsharded_unordered():
    import torch
    desc, pts, off, q = make_db(4096, 200, 31, biased=True, sizes=RAGGED)
    desc[:3083, 8:12] = desc[0, 8:12]                                    # dword 2 is constant in the first shard (rows 0 .. 3082) only: the orders differ
    nq, k, radius = len(q), 3, 60
    plain = capi.Context(0)
    plain.db_load(desc, pts, off)
    ref = plain.match(q, k, radius)
    same(ref, O.match(desc, off, pts, q, k, radius)[1:])
    assert len(ref[1]) >= 10
    plain.close()
    d_q = torch.from_numpy(q.copy()).cuda()
    keys = torch.empty((2, nq, k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctxs, orders = [], []
    for s in range(2):
        c = capi.Context(0)
        c.set_db_bit_order(1)
        c.db_load(desc, pts, off, shard_rank=s, shard_count=2)
        info = c.db_info()
        lo = info["shard_first"]
        assert np.array_equal(c.db_bit_order(), R.order_of(desc[lo:lo + info["shard_rows"]]))
        orders.append(c.db_bit_order())
        c.match_shard_device(d_q.data_ptr(), nq, k, radius, keys[s].data_ptr())
        c.synchronize()
        ctxs.append(c)
    assert not np.array_equal(orders[0], orders[1])
    cnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
    mm = torch.zeros((nq * k, 4), dtype=torch.int32, device="cuda")
    xx = torch.zeros((nq * k, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctxs[0].merge_shards_device(keys.data_ptr(), 2, nq, k, radius, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr())
    ctxs[0].synchronize()
    assert np.array_equal(d_q.cpu().numpy(), q)
    same(csr(cnt, mm, xx, nq, k), ref)
    for c in ctxs:
        c.close()


# ------------------------------------------------------------------------------------------------ 5. with the other matcher options
@pytest.mark.parametrize("biased", [True, False])
def test_ratio_test_and_lsh_see_the_same_db(biased):
    desc, pts, off, q = make_db(4096, 300, 41, biased=biased, sizes=RAGGED)
    on, offc = capi.Context(0), capi.Context(0)
    on.set_db_bit_order(1)
    offc.set_lsh(10, 16, 1)                                              # the index set before the load ...
    on.set_lsh(10, 16, 1)
    on.db_load(desc, pts, off)
    offc.db_load(desc, pts, off)
    assert not np.array_equal(on.db_bit_order(), IDENTITY)
    lsh_ref = offc.match(q, 5, 55)
    assert len(lsh_ref[1]) >= 10
    same(on.match(q, 5, 55), lsh_ref)
    same(match_device(on, q, 5, 55), lsh_ref)
    for c in (on, offc):
        c.set_lsh(0)
        c.set_ratio_test(0.8)
    ratio_ref = offc.match(q, 2, 55)
    same(ratio_ref, O.match(desc, off, pts, q, 2, 55, 0.8)[1:])
    assert len(ratio_ref[1]) >= 10
    same(on.match(q, 2, 55), ratio_ref)
    on.set_lsh(10, 16, 1)                                                # ... and set after the load, the ratio test still on
    offc.set_lsh(10, 16, 1)
    both_ref = offc.match(q, 2, 55)
    assert len(both_ref[1]) >= 10
    same(on.match(q, 2, 55), both_ref)
    for c in (on, offc):
        c.set_ratio_test(0.0)
    same(on.match(q, 5, 55), lsh_ref)
    on.close()
    offc.close()


# ------------------------------------------------------------------------------------------------ 6. pipeline
def test_pipeline_with_the_matchers_order_on():
    """One step of 2 frames on a pipeline whose matcher orders its DB (todhip_set_db_bit_order on todhip_pipeline_matcher before
    todhip_pipeline_db_load) against the same step on a pipeline that does not: n_kp, keypoints, the poses and their order, R, t and
    the inlier lists are identical."""
    import test_pipeline_gpu as TP
    env = TP.Env()
    try:
        p_off = env.pipeline()
        p_on = env.pipeline(load_db=False)
        p_on.matcher().set_db_bit_order(1)
        assert p_on.db_load(*env.db) == capi.OK
        assert np.array_equal(p_off.matcher().db_bit_order(), IDENTITY)
        assert np.array_equal(p_on.matcher().db_bit_order(), R.order_of(env.db[0]))
        assert not np.array_equal(p_on.matcher().db_bit_order(), IDENTITY)
        b = env.batches[0]
        want = env.wait(p_off, env.submit(p_off, b, 2))
        got = env.wait(p_on, env.submit(p_on, b, 2))
        assert len(got) == len(want) == 2 and all(len(r["poses"]) >= 1 for r in want)
        for g, w in zip(got, want):
            TP.same_frame(g, w)
        p_on.close()
        p_off.close()
    finally:
        env.ctx.close()
