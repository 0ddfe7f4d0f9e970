"""todhip_db_select_objects on the GPU: after select(S) every Hamming match entry point returns what a context loaded with only the
selected objects would return, with imgIdx (and the sharded keys' rows) in the numbering of the full DB. The checker is the CPU
oracle on the subset DB; a second context loaded with the subset is compared as well. Everything bit for bit.

The DB has objects of 0, 1, 31, 32, 33, 257, 5 and 700 rows: views of 1, 5 and 64 rows (shorter than one 32-row step of the
matrix-core engine, ending on a step), multi-segment views with an unsorted, repeated list, and views without rows. Query 0 is a row
of object 5, which no restricted selection holds: a library that ignored the selection would answer it from object 5."""
import numpy as np
import pytest

import oracle_lib as O
from tod_amd import capi, synth

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 31, 32, 33, 257, 5, 700]
N_OBJ = len(ROWS)
ENGINES = ["valu", "mfma", "mfma-whole", "mfma-split2", "mfma-split3"]     # tests/test_match_gpu.py's list
SELECTIONS = {"5rows": [6], "1row": [1], "64rows": [2, 4], "unsorted": [7, 3, 3], "empty-object": [0], "nothing": [],
              "every": list(range(N_OBJ)), "null": None}
NQS, KS, RADII = (1, 33, 70), (1, 2, 5, 8), (35, 256)
FIELDS = ("queryIdx", "trainIdx", "imgIdx", "distance")


class Db:
    def __init__(self, rows, seed=2024, biased=False):
        rng = np.random.Generator(np.random.PCG64(seed))
        n = int(sum(rows))
        self.off = np.concatenate([[0], np.cumsum(rows)]).astype(np.uint32)
        self.desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        if biased:                                                      # the first 64 bits are set in a quarter of the rows only
            self.desc[:, :8] &= rng.integers(0, 256, (n, 8), dtype=np.uint8)
        self.pts = rng.standard_normal((n, 3)).astype(np.float32)
        # 70 queries: rows of the non-empty objects in turn, the object of 257 rows first, with 0..20 flipped bits; every 7th random
        order = [o for o in np.argsort([-r for r in rows], kind="stable") if rows[o] > 0]
        order = [order[1]] + [order[0]] + order[2:] if len(order) > 1 else order           # 257 rows, 700 rows, the rest
        q = np.zeros((70, 32), np.uint8)
        self.src_obj = np.full(70, -1)
        for i in range(70):
            if i % 7 == 6:
                q[i] = rng.integers(0, 256, 32, dtype=np.uint8)
                continue
            o = order[(i - i // 7) % len(order)]
            row = int(self.off[o]) + int(rng.integers(0, rows[o]))
            bits = np.unpackbits(self.desc[row])
            flip = rng.choice(256, int(rng.integers(0, 21)), replace=False)
            bits[flip] ^= 1
            q[i] = np.packbits(bits)
            self.src_obj[i] = o
        self.q = q

    def subset(self, sel):
        """(S, desc, pts, off, global row of every subset row) of the ascending distinct indices of sel"""
        S = sorted(set(sel))
        rows = np.concatenate([np.arange(self.off[o], self.off[o + 1]) for o in S] + [np.zeros(0, np.int64)]).astype(np.int64)
        off = np.concatenate([[0], np.cumsum([int(self.off[o + 1] - self.off[o]) for o in S])]).astype(np.uint32)
        return S, self.desc[rows], self.pts[rows], off, rows

    def want(self, sel, q, k, radius, ratio=0.0):
        """The definition: the oracle on the subset DB, imgIdx mapped through S. None / every object: the oracle on the whole DB."""
        if sel is None:
            rc, rp, m, xyz = O.match(self.desc, self.off, self.pts, q, k, radius, ratio)
            assert rc == 0
            return rp, m, xyz
        S, desc, pts, off, _ = self.subset(sel)
        if len(desc) == 0:
            return np.zeros(len(q) + 1, np.uint32), np.zeros(0, capi.DMATCH_DTYPE), np.zeros((0, 3), np.float32)
        rc, rp, m, xyz = O.match(desc, off, pts, q, k, radius, ratio)
        assert rc == 0
        m["imgIdx"] = np.asarray(S, np.int32)[m["imgIdx"]]
        return rp, m, xyz


@pytest.fixture(scope="module")
def db():
    d = Db(ROWS)
    # what the fixture promises: query 0 (part of every nq) is nearest to a row of object 5, within the smaller radius, and object 5
    # is in no restricted selection -- so for each of them the unrestricted answer differs from the selected one
    keys = O.knn_keys(d.desc, d.q, 1)
    owner = np.searchsorted(d.off, (keys[:, 0] & np.uint64(0xFFFFFFFF)).astype(np.int64), side="right") - 1
    assert owner[0] == 5 and int(keys[0, 0] >> np.uint64(32)) <= 20
    full = d.want(None, d.q[:1], 1, 35)
    for name, sel in SELECTIONS.items():
        if sel is None or len(set(sel)) == N_OBJ:
            continue
        assert 5 not in sel and any(o not in sel for o in owner), name
        got = d.want(sel, d.q[:1], 1, 35)
        assert not (np.array_equal(got[0], full[0]) and np.array_equal(got[1], full[1])), name
    assert set(owner) >= {1, 2, 3, 4, 5, 6, 7}                          # every non-empty object owns some query's nearest row
    return d


def make_ctx(engine):
    c = capi.Context(0)
    name, _, form = engine.partition("-")
    c.set_matcher_engine(name)
    if form:
        c.set_matcher_block_split({"whole": 0, "split2": 2, "split3": 3}[form])
    return c


@pytest.fixture(scope="module", params=ENGINES)
def ctx(request, db):
    c = make_ctx(request.param)
    c.engine = request.param
    c.db_load(db.desc, db.pts, db.off)
    yield c
    c.close()


class Dev:
    """todhip_match_device through torch tensors, results in the host form's CSR shape"""

    def __init__(self):
        import torch
        self.torch = torch

    def match(self, c, q, k, radius, fn=None):
        torch = self.torch
        nq = len(q)
        d_q = torch.from_numpy(np.ascontiguousarray(q)).cuda()
        cnt = torch.full((nq,), 77, dtype=torch.int32, device="cuda")
        mm = torch.zeros((nq * k, 4), dtype=torch.int32, device="cuda")
        xx = torch.zeros((nq * k, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        (fn or c.match_device)(d_q.data_ptr(), nq, k, radius, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr())
        c.synchronize()
        return self.csr(cnt, mm, xx, nq, k)

    @staticmethod
    def csr(cnt, mm, xx, nq, k):
        cnt = cnt.cpu().numpy().astype(np.int64)
        keep = np.arange(k)[None, :] < cnt[:, None]
        m = mm.cpu().numpy().view(capi.DMATCH_DTYPE).reshape(nq, k)[keep]
        xyz = xx.cpu().numpy().reshape(nq, k, 3)[keep]
        return np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32), m, xyz


@pytest.fixture(scope="module")
def dev():
    return Dev()


def same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), what
    for f in FIELDS:
        assert np.array_equal(got[1][f], want[1][f]), (what, f)
    assert np.array_equal(got[2], want[2]), what


def selection_numbers(db, sel):
    if sel is None:
        return dict(n_objs=N_OBJ, rows=int(db.off[-1]), shard_rows=int(db.off[-1]))
    n = int(sum(ROWS[o] for o in set(sel)))
    return dict(n_objs=len(set(sel)), rows=n, shard_rows=n)


@pytest.mark.parametrize("name", list(SELECTIONS))
def test_selected_match_equals_the_oracle_on_the_subset(ctx, dev, db, name):
    """case 1 (and the unrestricted forms of case 2): todhip_match and todhip_match_device against the definition and against a
    context that was loaded with the subset alone, over every launch shape of the sweep"""
    sel = SELECTIONS[name]
    ctx.select_objects(sel)
    assert ctx.selection() == selection_numbers(db, sel)
    assert ctx.db_info() == dict(total_rows=int(db.off[-1]), shard_first=0, shard_rows=int(db.off[-1]), n_objs=N_OBJ)
    other = None
    if sel is not None and sum(ROWS[o] for o in set(sel)) > 0:
        S, s_desc, s_pts, s_off, _ = db.subset(sel)
        other = make_ctx(ctx.engine)
        other.db_load(s_desc, s_pts, s_off)
    try:
        for nq in NQS:
            for k in KS:
                for radius in RADII:
                    q = db.q[:nq]
                    want = db.want(sel, q, k, radius)
                    what = (name, nq, k, radius)
                    same(ctx.match(q, k, radius), want, what)
                    same(dev.match(ctx, q, k, radius), want, what)
                    if sel is not None and sum(ROWS[o] for o in set(sel)) == 0:
                        assert int(want[0][-1]) == 0                     # [] and [0]: TODHIP_OK and every count 0
                    if other is not None:
                        rp, m, xyz = other.match(q, k, radius)
                        m["imgIdx"] = np.asarray(sorted(set(sel)), np.int32)[m["imgIdx"]]
                        same((rp, m, xyz), want, what + ("subset context",))
    finally:
        if other is not None:
            other.close()
        ctx.select_objects(None)


def test_back_to_all_objects_and_a_load_resets(ctx, db):
    """case 2: select(S) then select(None) is the state before any selection; so is a new load"""
    q = db.q
    before = ctx.match(q, 5, 35)
    same(before, db.want(None, q, 5, 35))
    ctx.select_objects([6])
    assert ctx.selection() == dict(n_objs=1, rows=5, shard_rows=5)
    same(ctx.match(q, 5, 35), db.want([6], q, 5, 35))
    ctx.select_objects(None)
    assert ctx.selection() == selection_numbers(db, None)
    same(ctx.match(q, 5, 35), before)
    ctx.select_objects([2, 4])
    ctx.db_load(db.desc, db.pts, db.off)
    assert ctx.selection() == selection_numbers(db, None)
    same(ctx.match(q, 5, 35), before)


def test_errors(ctx, db):
    """case 3"""
    L = capi.lib()
    ctx.select_objects([7, 3, 3])
    want = db.want([7, 3], db.q, 2, 35)
    bad = np.array([3, 8], np.uint32)
    assert L.todhip_db_select_objects(ctx._h, bad.ctypes.data, 2) == capi.EINVAL
    assert ctx.selection() == dict(n_objs=2, rows=732, shard_rows=732)
    same(ctx.match(db.q, 2, 35), want)                                  # the previous selection stays
    ctx.select_objects(None)
    ids = np.array([0], np.uint32)
    fl = capi.Context(0)
    rng = np.random.Generator(np.random.PCG64(5))
    fl.db_load(rng.standard_normal((40, 128)).astype(np.float32), db.pts[:40], np.array([0, 10, 40]))
    assert L.todhip_db_select_objects(fl._h, ids.ctypes.data, 1) == capi.EINVAL
    assert L.todhip_db_select_objects(fl._h, None, 0) == capi.EINVAL
    fl.close()
    empty = capi.Context(0)
    assert L.todhip_db_select_objects(empty._h, ids.ctypes.data, 1) == capi.ENODB
    assert L.todhip_db_select_objects(empty._h, None, 0) == capi.ENODB
    empty.close()


@pytest.mark.parametrize("name", ["5rows", "1row", "64rows", "unsorted", "nothing"])
def test_ratio_test_sees_the_selected_rows(ctx, dev, db, name):
    """case 4: ratio 0.8, k = 2 (and k = 1, which fetches the second neighbour internally)"""
    sel = SELECTIONS[name]
    ctx.select_objects(sel)
    ctx.set_ratio_test(0.8)
    try:
        for k in (2, 1):
            for radius in RADII:
                want = db.want(sel, db.q, k, radius, 0.8)
                same(ctx.match(db.q, k, radius), want, (name, k, radius))
                same(dev.match(ctx, db.q[:33], k, radius), db.want(sel, db.q[:33], k, radius, 0.8), (name, k, radius))
    finally:
        ctx.set_ratio_test(0.0)
        ctx.select_objects(None)


@pytest.mark.parametrize("engine", ["valu", "mfma", "mfma-split2"])
def test_bit_order_then_a_selection(db, engine):
    """case 5: the view copies the rows as the load stored them, and the queries follow that order"""
    d2 = Db(ROWS, seed=11, biased=True)                               # biased leading bits: the order is not the identity
    q = d2.q
    c = make_ctx(engine)
    c.set_db_bit_order(1)
    c.db_load(d2.desc, d2.pts, d2.off)
    assert not np.array_equal(c.db_bit_order(), np.arange(256))
    try:
        for name in ("5rows", "64rows", "unsorted", "nothing", "null"):
            sel = SELECTIONS[name]
            c.select_objects(sel)
            for k, radius in ((2, 35), (5, 256)):
                same(c.match(q, k, radius), d2.want(sel, q, k, radius), (name, k, radius))
    finally:
        c.close()


def _keys_of(m, rp, off):
    rows = off[m["imgIdx"]].astype(np.int64) + m["trainIdx"]
    return [[(int(d) << 32) | int(r) for d, r in zip(m["distance"][rp[i]:rp[i + 1]], rows[rp[i]:rp[i + 1]])] for i in range(len(rp) - 1)]


@pytest.mark.parametrize("name", ["5rows", "64rows", "unsorted", "nothing"])
def test_lsh_indexes_the_view(ctx, db, name):
    """case 6: 10 tables x 16 bits, level 1 -- the keys of the LSH checker on the subset DB, rows mapped; exact again afterwards"""
    sel = SELECTIONS[name]
    S, s_desc, _, _, rows = db.subset(sel)
    k = 5
    try:
        for lsh_first in (True, False):                                  # the index follows the selection whichever comes first
            if lsh_first:
                ctx.set_lsh(10, 16, 1)
                ctx.select_objects(sel)
            else:
                ctx.select_objects(sel)
                ctx.set_lsh(10, 16, 1)
            rp, m, _ = ctx.match(db.q, k, 256)
            got = _keys_of(m, rp, db.off)
            if len(s_desc):
                want, _ = O.lsh_knn_keys(s_desc, db.q, k, 10, 16, 1)
                n_found = 0
                for i in range(len(db.q)):
                    w = [(int(kk) >> 32) << 32 | int(rows[int(kk) & 0xFFFFFFFF]) for kk in want[i] if int(kk) != 0xFFFFFFFFFFFFFFFF]
                    assert got[i] == w, (name, i)
                    n_found += len(w)
                assert n_found > 0
            else:
                assert int(rp[-1]) == 0
            ctx.set_lsh(0)
            same(ctx.match(db.q, k, 35), db.want(sel, db.q, k, 35), name)
            ctx.select_objects(None)
    finally:
        ctx.set_lsh(0)
        ctx.select_objects(None)


SHARD_DBS = {"as-fixture": ROWS, "big-first": [700, 0, 1, 31, 32, 33, 257, 5]}    # the second one gives every shard some objects


@pytest.mark.parametrize("layout", list(SHARD_DBS))
def test_shards_with_the_same_selection_merge_to_the_single_context_result(ctx, dev, db, layout):
    """case 7: shards 0..2 of 3 with the selection set on each, todhip_match_shard_device + todhip_merge_shards_device"""
    import torch
    from tod_amd import sharded
    d = db if layout == "as-fixture" else Db(SHARD_DBS[layout], seed=77)
    n_shards, nq = 3, 70
    ctxs = []
    for s in range(n_shards):
        c = make_ctx(ctx.engine)
        c.db_load(d.desc, d.pts, d.off, shard_rank=s, shard_count=n_shards)
        ctxs.append(c)
    d_q = torch.from_numpy(d.q).cuda()
    rows_of = SHARD_DBS[layout]
    try:
        if layout == "big-first":
            assert all(c.db_info()["shard_rows"] > 0 for c in ctxs)
        for sel in ([0], [5, 2, 2, 7], [0, 6, 7], [3], [1], [], None):     # some leave one or two shards without a selected row
            empty_shards = 0
            for s, c in enumerate(ctxs):
                c.select_objects(sel)
                lo, hi, _, _ = sharded.shard_bounds(d.off, s, n_shards)
                mine = sum(rows_of[o] for o in (range(lo, hi) if sel is None else set(sel) & set(range(lo, hi))))
                total = int(d.off[-1]) if sel is None else sum(rows_of[o] for o in set(sel))
                assert c.selection() == dict(n_objs=len(rows_of) if sel is None else len(set(sel)), rows=total, shard_rows=mine)
                empty_shards += mine == 0
            for k, radius in ((2, 35), (5, 256)):
                keys_all = torch.zeros((n_shards, nq, k), dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                for s, c in enumerate(ctxs):
                    c.match_shard_device(d_q.data_ptr(), nq, k, radius, keys_all[s].data_ptr())
                    c.synchronize()
                got = dev.match(ctxs[1], d.q, k, radius,
                                fn=lambda q_, n_, k_, r_, cn, mm, xx: ctxs[1].merge_shards_device(keys_all.data_ptr(), n_shards, n_, k_, r_, cn, mm, xx))
                same(got, d.want(sel, d.q, k, radius), (layout, sel, k, radius, empty_shards))
    finally:
        for c in ctxs:
            c.close()


def test_verifier_takes_the_selected_matches_with_the_full_spans(dev):
    """case 9: todhip_match_device under a selection -> todhip_verify_device with the spans of every object == the oracle's verifier
    on the oracle's subset match with mapped imgIdx (objects, inliers and draws exactly, poses within the two verifiers' known
    1e-3), and bit for bit the library's own verifier on those oracle matches"""
    import torch
    desc, pts, off = synth.make_db(3, per_object=2000)
    fr = synth.make_frame(desc, pts, off, 500, frame=0, visible_object=1)
    sel, S = [2, 1], [1, 2]
    k, radius = 5, 35
    c = capi.Context(0)
    spans = c.db_load(desc, pts, off)
    c.select_objects(sel)
    rows = np.arange(off[1], off[3])
    rc, o_rp, o_m, o_xyz = O.match(desc[rows], off[1:] - off[1], pts[rows], fr["q_desc"], k, radius)
    assert rc == 0 and len(o_m) > 50
    o_m["imgIdx"] = np.asarray(S, np.int32)[o_m["imgIdx"]]
    nq = len(fr["q_desc"])
    d_q = torch.from_numpy(fr["q_desc"]).cuda()
    d_kp = torch.from_numpy(np.ascontiguousarray(fr["kp_xy"], np.float32)).cuda()
    d_cloud = torch.from_numpy(np.ascontiguousarray(fr["cloud"], np.float32)).cuda()
    H, W = fr["cloud"].shape[:2]
    cnt = torch.zeros(nq, dtype=torch.int32, device="cuda"); mm = torch.zeros((nq * k, 4), dtype=torch.int32, device="cuda")
    xx = torch.zeros((nq * k, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    c.match_device(d_q.data_ptr(), nq, k, radius, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr())
    rng_g, rng_h, rng_o = capi.rng_new(1), capi.rng_new(1), O.rng_new(1)
    poses = c.verify_device(d_kp.data_ptr(), nq, d_cloud.data_ptr(), H, W, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr(), k, spans,
                            8, 2500, 0.01, rng_g)
    same(Dev.csr(cnt, mm, xx, nq, k), (o_rp, o_m, o_xyz))
    rc, o_poses, _ = O.verify(fr["kp_xy"], fr["cloud"], o_rp, o_m, o_xyz, O.spans(pts, off), 8, 2500, 0.01, rng_o)
    h_poses = c.verify(fr["kp_xy"], fr["cloud"], o_rp, o_m, o_xyz, spans, 8, 2500, 0.01, rng_h)
    c.close()
    assert rc == 0 and [p["object"] for p in poses] == [p["object"] for p in o_poses] == [1]
    assert rng_g.draws == rng_o.draws == rng_h.draws
    for g, o, h in zip(poses, o_poses, h_poses):
        assert np.array_equal(g["inliers"], o["inliers"])
        assert np.abs(g["R"] - o["R"]).max() < 1e-3 and np.abs(g["t"] - o["t"]).max() < 1e-3
        assert h["object"] == g["object"] and np.array_equal(h["inliers"], g["inliers"])
        assert np.array_equal(h["R"], g["R"]) and np.array_equal(h["t"], g["t"])


# ---------------------------------------------------------------------------------------------------- case 8: the pipeline
NF, LEVELS, SCALE, PK, PRADIUS = 500, 3, 1.2, 5, 55
VERIFY = (8, 2500, 0.01)
B = 4
TIMEOUT_MS = 60000


def test_pipeline_selection_names_only_the_selected_decoy():
    """The trained plane plus two decoys that are copies of it: every query's nearest rows tie across the three and the unrestricted
    poses name the first. With a decoy selected the poses name that decoy only and equal, frame by frame, the single-frame device
    chain on a context with the same selection; EBUSY while a ticket is outstanding; NULL restores the unrestricted poses."""
    import torch
    from tod_amd import scenes
    H, W = scenes.H, scenes.W                                          # the frame size of tests/test_pipeline_gpu.py
    textures = scenes.make_textures(1)
    c = capi.Context(0)
    d1, p1, _ = scenes.train_db(c, textures, n_features=600)
    n = len(d1)
    desc, pts, off = np.concatenate([d1] * 3), np.concatenate([p1] * 3), np.array([0, n, 2 * n, 3 * n], np.uint32)
    spans = c.db_load(desc, pts, off)
    batch = scenes.make_detection_batches(textures, 1, B, visible_fraction=1.0)[0]
    kp = torch.zeros((NF, 2), device="cuda"); aux = torch.zeros((NF, 4), device="cuda")
    dd = torch.zeros((NF, 32), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(NF, dtype=torch.int32, device="cuda"); mm = torch.zeros((NF * PK, 4), dtype=torch.int32, device="cuda")
    xx = torch.zeros((NF * PK, 3), device="cuda")

    def chain(f):
        torch.cuda.synchronize()
        nk = c.orb_device(batch["images"][f].data_ptr(), H, W, W, NF, LEVELS, SCALE, kp.data_ptr(), aux.data_ptr(), dd.data_ptr(), NF)
        c.match_device(dd.data_ptr(), nk, PK, PRADIUS, cnt.data_ptr(), mm.data_ptr(), xx.data_ptr())
        poses = c.verify_device_depth(kp.data_ptr(), nk, batch["depth"][f].data_ptr(), False, H, W, scenes.K, cnt.data_ptr(), mm.data_ptr(),
                                      xx.data_ptr(), PK, spans, *VERIFY, capi.rng_new(1))
        c.synchronize()
        return dict(n_kp=nk, kp_xy=kp[:nk].cpu().numpy(), poses=poses)

    def same_step(res, ref):
        assert len(res) == B
        for got, want in zip(res, ref):
            assert got["n_kp"] == want["n_kp"] and np.array_equal(got["kp_xy"], want["kp_xy"])
            assert [p["object"] for p in got["poses"]] == [p["object"] for p in want["poses"]]
            for a, b in zip(got["poses"], want["poses"]):
                assert np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"]) and np.array_equal(a["inliers"], b["inliers"])

    p = capi.Pipeline(0, frames_per_step=B, H=H, W=W, K=scenes.K, n_features=NF, n_levels=LEVELS, scale_factor=SCALE, k=PK, radius=PRADIUS,
                      verify=VERIFY, ring_depth=3)
    try:
        assert p.db_load(desc, pts, off) == capi.OK

        def step():
            rc, t = p.submit_device(batch["images"].data_ptr(), batch["depth"].data_ptr(), B)
            assert rc == capi.OK
            rc, res = p.wait(t, TIMEOUT_MS)
            assert rc == capi.OK
            return res

        ref_all = [chain(f) for f in range(B)]
        assert all(r["poses"] for r in ref_all)
        same_step(step(), ref_all)
        c.select_objects([2])
        ref_sel = [chain(f) for f in range(B)]
        assert all(r["poses"] and {q["object"] for q in r["poses"]} == {2} for r in ref_sel)
        assert any({q["object"] for q in r["poses"]} != {2} for r in ref_all)
        assert p.select_objects([2]) == capi.OK
        same_step(step(), ref_sel)
        rc, t = p.submit_device(batch["images"].data_ptr(), batch["depth"].data_ptr(), B)
        assert rc == capi.OK
        assert p.select_objects(None) == capi.EBUSY                     # a ticket is outstanding
        assert p.select_objects([1]) == capi.EBUSY
        rc, res = p.wait(t, TIMEOUT_MS)
        assert rc == capi.OK
        same_step(res, ref_sel)                                          # and the refused calls changed nothing
        assert p.select_objects([3]) == capi.EINVAL
        assert p.select_objects(None) == capi.OK
        same_step(step(), ref_all)
    finally:
        p.close()
        c.close()
