"""todhip_model_compact / todhip_model_add_rows on the GPU against the numpy restatement of the header's definition
(tests/model_compact_ref.py). Every case goes add_rows -> compact -> finish; the kept descriptors, the kept points (compared as bytes),
rows_after and support must equal the restatement exactly -- the definition is exact, so there is no tolerance anywhere."""
import numpy as np
import pytest

from model_compact_ref import compact_ref, random_model
from tod_amd import capi, synth

pytestmark = pytest.mark.gpu

# (seed, rows, base rows, merge_dist, max_hamming, spread) of model_compact_ref.random_model; what they give is checked on the CPU by
# tests/test_model_compact_cpu.py: A keeps 1308 of 2000, B keeps 2522 of 3000
MODEL_A = (11, 2000, 300, 0.01, 20, 1.2)
MODEL_B = (12, 3000, 3500, 0.01, 20, 1.0)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _bits(*bits):
    d = np.zeros(32, np.uint8)
    for b in bits:
        d[b // 8] |= 1 << (b % 8)
    return d


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check(ctx, desc, pts, merge_dist, max_hamming):
    """add_rows -> compact -> finish against the restatement; returns the kept indices"""
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    n = len(desc)
    kept, sup = compact_ref(desc, pts, merge_dist, max_hamming)
    model = capi.Model(ctx, max(n, 1))
    try:
        assert model.add_rows(desc, pts) == n
        before, after, support = model.compact(merge_dist, max_hamming, want_support=True)
        d, p = model.finish()
        print("rows %d -> %d (restatement %d)" % (before, after, len(kept)))
        assert before == n and after == len(kept) == len(d)
        assert _same(d, desc[kept]) and _same(p, pts[kept])
        assert np.array_equal(support, sup) and int(support.sum()) == n
        assert model.device()[2] == after
    finally:
        model.close()
    return kept


def _spread_points(n):
    """n points nothing merges: 10 apart on the x axis"""
    p = np.zeros((n, 3), np.float32)
    p[:, 0] = 10.0 * np.arange(n)
    return p


SIZES = [0, 1, 2, 63, 64, 65, 129, 200]


@pytest.mark.parametrize("n", SIZES)
def test_all_rows_distinct(ctx, n):
    rng = np.random.Generator(np.random.PCG64(100 + n))
    kept = _check(ctx, rng.integers(0, 256, (n, 32), dtype=np.uint8), _spread_points(n), 1.0, 256)
    assert len(kept) == n


@pytest.mark.parametrize("n", SIZES)
def test_all_rows_identical(ctx, n):
    desc = np.tile(_bits(1, 77, 255), (n, 1))
    kept = _check(ctx, desc, np.tile(np.float32([0.1, 0.2, 0.3]), (n, 1)), 0.0, 0)
    assert len(kept) == min(n, 1)


@pytest.mark.parametrize("n", SIZES)
def test_mixed_rows(ctx, n):
    desc, pts = random_model(200 + n, n, max(n // 4, 1), 0.01, 20, 1.2)
    kept = _check(ctx, desc, pts, 0.01, 20)
    assert n < 63 or 0 < len(kept) < n


@pytest.mark.parametrize("at", [62, 63, 64])
def test_chain_across_a_block_boundary(ctx, at):
    """A, B, C at rows at .. at + 2: A-B and B-C conflict, A-C does not, so A and C stay -- with the 64-row block boundary before A,
    between A and B, between B and C"""
    pts = _spread_points(70)
    pts[at:at + 3, 0] = np.float32(10000.0) + np.float32([0.0, 0.6, 1.2])
    kept = _check(ctx, np.zeros((70, 32), np.uint8), pts, 1.0, 0)
    assert kept.tolist() == [i for i in range(70) if i != at + 1]


def test_dropped_row_counts_for_the_earlier_blocks_kept_row(ctx):
    """row 3 (block 0) and row 66 (block 1) are 1.5 apart and both kept; row 68 lies between them and conflicts with both: it goes
    to row 3, the lower index, although row 66 is a kept row of its own block"""
    pts = _spread_points(70)
    pts[3, 0], pts[66, 0], pts[68, 0] = 5000.0, 5001.5, 5000.75
    desc = np.zeros((70, 32), np.uint8)
    kept, sup = compact_ref(desc, pts, 1.0, 0)
    assert kept.tolist() == [i for i in range(70) if i != 68] and sup[3] == 2 and sup[66] == 1
    _check(ctx, desc, pts, 1.0, 0)


EDGES = {
    "ham_equal": (np.stack([_bits(), _bits(0, 9, 255)]), np.zeros((2, 3)), 0.0, 3, [0]),
    "ham_above": (np.stack([_bits(), _bits(0, 9, 255)]), np.zeros((2, 3)), 0.0, 2, [0, 1]),
    "ham_0_equal_rows": (np.stack([_bits(5), _bits(5), _bits(6)]), np.zeros((3, 3)), 0.0, 0, [0, 2]),
    "ham_256": (np.stack([_bits(), _bits(*range(256))]), np.zeros((2, 3)), 0.0, 256, [0]),
    "ham_255": (np.stack([_bits(), _bits(*range(256))]), np.zeros((2, 3)), 0.0, 255, [0, 1]),
    "dist_equal": (np.zeros((2, 32)), [[0, 0, 0], [0.5, 0, 0]], 0.5, 0, [0]),
    "dist_below": (np.zeros((2, 32)), [[0, 0, 0], [0.5, 0, 0]], float(np.nextafter(np.float32(0.5), np.float32(0))), 0, [0, 1]),
    "dist_0_signed_zero": (np.zeros((3, 32)), [[0.0, 1, 2], [-0.0, 1, 2], [1e-10, 1, 2]], 0.0, 0, [0, 2]),
    # d2 = 2.25e-40 and r2 = 1e-40 are subnormal: flushed to zero they would conflict
    "dist_subnormal": (np.zeros((2, 32)), [[0, 0, 0], [1.5e-20, 0, 0]], 1e-20, 0, [0, 1]),
    "nan_and_inf": (np.zeros((7, 32)), [[0, 0, 0], [np.nan, 0, 0], [0, 0, 0], [0, np.nan, 0], [np.inf, 0, 0], [np.inf, 0, 0], [0, 0, -np.inf]],
                    10.0, 256, [0, 1, 3, 4, 5, 6]),
    "dword_7_only": (np.stack([_bits(), _bits(255), _bits(*range(224, 232)), _bits(224)]), np.zeros((4, 3)), 0.0, 1, [0, 2]),
    "dword_7_ham_8": (np.stack([_bits(), _bits(255), _bits(*range(224, 232)), _bits(224)]), np.zeros((4, 3)), 0.0, 8, [0]),
    "bit_255_only": (np.stack([_bits(), _bits(255)]), np.zeros((2, 3)), 0.0, 0, [0, 1]),
}


@pytest.mark.parametrize("name", sorted(EDGES))
def test_threshold_edges(ctx, name):
    desc, pts, md, mh, want = EDGES[name]
    kept = _check(ctx, np.asarray(desc, np.uint8), np.asarray(pts, np.float32), md, mh)
    assert kept.tolist() == want                                          # the hand-worked answer, as in the CPU test


@pytest.fixture(scope="module")
def model_a():
    desc, pts = random_model(*MODEL_A)
    kept, sup = compact_ref(desc, pts, MODEL_A[3], MODEL_A[4])
    for a in (desc, pts, kept, sup):
        a.setflags(write=False)
    return desc, pts, kept, sup


def _compacted(ctx, model_a, cap=None):
    desc, pts, kept, sup = model_a
    model = capi.Model(ctx, cap or len(desc))
    assert model.add_rows(desc, pts) == len(desc)
    return model


def test_random_model_a_third_dropped(ctx, model_a):
    """kept front 1308 of 2000: it crosses lane, workgroup (256 partners) and the 1024 boundary while rows still go"""
    desc, pts, kept, sup = model_a
    model = _compacted(ctx, model_a)
    before, after, support = model.compact(MODEL_A[3], MODEL_A[4], want_support=True)
    d, p = model.finish()
    assert (before, after) == (2000, len(kept)) and _same(d, desc[kept]) and _same(p, pts[kept]) and np.array_equal(support, sup)
    # again with the same arguments: the identity
    before, after, support = model.compact(MODEL_A[3], MODEL_A[4], want_support=True)
    d2, p2 = model.finish()
    model.close()
    assert before == after == len(kept) and _same(d2, d) and _same(p2, p) and (support == 1).all()


def test_random_model_nearly_all_kept(ctx):
    kept = _check(ctx, *random_model(*MODEL_B)[:2], MODEL_B[3], MODEL_B[4])
    assert len(kept) > 2048


def test_support_capacity_and_invalid_arguments(ctx, model_a):
    desc, pts, kept, sup = model_a
    L, C = capi.lib(), capi.C
    model = _compacted(ctx, model_a)
    before, after, ns = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    small = np.zeros(8, np.uint32)
    for md, mh in ((-1.0, 20), (float("nan"), 20), (float("inf"), 20), (0.01, 257)):
        assert L.todhip_model_compact(ctx._h, model._h, md, mh, C.byref(before), C.byref(after), None, None) == capi.EINVAL
        d, p = model.finish()
        assert _same(d, desc) and _same(p, pts)                           # untouched
    assert L.todhip_model_compact(ctx._h, model._h, 0.01, 20, None, None, small.ctypes.data, None) == capi.EINVAL
    assert model.device()[2] == len(desc)
    ns.value = 8
    rc = L.todhip_model_compact(ctx._h, model._h, MODEL_A[3], MODEL_A[4], C.byref(before), C.byref(after), small.ctypes.data, C.byref(ns))
    assert rc == capi.ECAPACITY and ns.value == after.value == len(kept) and before.value == len(desc) and not small.any()
    d, p = model.finish()                                                 # already compacted
    model.close()
    assert _same(d, desc[kept]) and _same(p, pts[kept])


def test_add_rows_is_cut_at_the_capacity(ctx):
    rng = np.random.Generator(np.random.PCG64(5))
    desc, pts = rng.integers(0, 256, (15, 32), dtype=np.uint8), rng.random((15, 3)).astype(np.float32)
    model = capi.Model(ctx, 10)
    assert model.add_rows(desc[:4], pts[:4]) == 4 and model.add_rows(desc[4:], pts[4:]) == 6 and model.add_rows(desc, pts) == 0
    assert model.add_rows(desc[:0], pts[:0]) == 0
    d, p = model.finish()
    model.close()
    assert _same(d, desc[:10]) and _same(p, pts[:10])


def _view(i):
    img = synth.make_image(40 + i)
    mask = np.zeros((480, 640), np.uint8); mask[60:420, 120:560] = 255
    depth = np.full((480, 640), 0.7, np.float32)
    K = np.array([[525, 0, 319.5], [0, 525, 239.5], [0, 0, 1]], np.float32)
    return img, mask, depth, K, np.eye(3, dtype=np.float32), np.zeros(3, np.float32)


def test_observation_behind_added_rows(ctx):
    rng = np.random.Generator(np.random.PCG64(6))
    desc, pts = rng.integers(0, 256, (100, 32), dtype=np.uint8), rng.random((100, 3)).astype(np.float32)
    plain, behind = capi.Model(ctx, 1000), capi.Model(ctx, 1000)
    n = plain.add_observation(*_view(0), n_features=300, n_levels=3)
    assert behind.add_rows(desc, pts) == 100 and behind.add_observation(*_view(0), n_features=300, n_levels=3) == n > 100
    (d0, p0), (d1, p1) = plain.finish(), behind.finish()
    plain.close(); behind.close()
    assert _same(d1, np.concatenate([desc, d0])) and _same(p1, np.concatenate([pts, p0]))


def test_compact_observe_compact(ctx):
    """the compacted model takes further observations; the second compaction sees the first one's front plus the new rows, and a
    third with nothing new is the identity"""
    model = capi.Model(ctx, 2000)
    model.add_observation(*_view(0), n_features=300, n_levels=3)
    d0, p0 = model.finish()
    k0, _ = compact_ref(d0, p0, 0.003, 24)
    assert model.compact(0.003, 24) == (len(d0), len(k0))
    n1 = model.add_observation(*_view(0), n_features=300, n_levels=3)    # the same view again: every new row repeats an old one
    d1, p1 = model.finish()
    assert n1 == len(d0) and _same(d1, np.concatenate([d0[k0], d0])) and _same(p1, np.concatenate([p0[k0], p0]))
    k1, s1 = compact_ref(d1, p1, 0.003, 24)
    before, after, support = model.compact(0.003, 24, want_support=True)
    d2, p2 = model.finish()
    assert (before, after) == (len(d1), len(k1)) and after == len(k0) and _same(d2, d1[k1]) and np.array_equal(support, s1)
    assert model.compact(0.003, 24) == (after, after)
    d3, p3 = model.finish()
    model.close()
    assert _same(d3, d2) and _same(p3, p2)


def test_compacted_model_loads_device_to_device(ctx, model_a):
    """todhip_model_device reports rows_after, and the DB loaded from the device buffers answers as one loaded from finish()"""
    desc, pts, kept, sup = model_a
    model = _compacted(ctx, model_a)
    model.compact(MODEL_A[3], MODEL_A[4])
    assert model.device()[2] == len(kept)
    d, p = model.finish()
    ref = capi.Context(0)
    spans_dev, off = ctx.db_load_models([model])
    spans_host = ref.db_load(d, p, np.array([0, len(d)], np.uint32))
    model.close()
    assert off.tolist() == [0, len(kept)] and _same(np.asarray(spans_dev, np.float32), np.asarray(spans_host, np.float32))
    q = desc[::7]                                                          # kept and dropped rows alike
    a, b = ctx.match(q, 5, 55), ref.match(q, 5, 55)
    ref.close()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and int(a[0][-1]) >= len(q)


TRAIN_VIEWS = [(0.0, (0.0, 0.0)), (4.0, (6.0, -4.0)), (-5.0, (-7.0, 5.0))]   # theta_deg, shift px
E2E_MERGE = (0.003, 24)                                                        # 2 pixels at Z = 0.8 m, f = 525; bits


def test_train_three_views_compact_then_detect():
    """tests/test_end_to_end_gpu.py with a model from three views a few degrees apart, compacted before it is loaded: the held-out
    view's rendering pose is recovered within that test's tolerances, and the model got smaller.
    The settings were chosen on the CPU: the restatements of ORB -> training -> matcher -> verifier (tests/oracle_lib.py) followed by
    compact_ref give 1483 + 1469 + 1491 = 4443 rows before and 2074 after (largest support 10), and recover the pose with 900 inliers,
    max |R - R_true| = 1e-4, max |t - t_true| = 7e-4 m (uncompacted: 905 inliers, 1.3e-3, 7e-4 m)."""
    from test_end_to_end_gpu import F, H, K, W, _render
    Z = 0.8
    texture = synth.make_image(321)
    ctx = capi.Context(0)
    depth = np.full((H, W), Z, np.float32)
    border = np.zeros((H, W), bool); border[40:H - 40, 40:W - 40] = True
    v2, u2 = np.mgrid[0:H, 0:W].astype(np.float32)

    def pose(theta, shift):
        c, s = np.cos(theta), np.sin(theta)
        R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float32)
        t = np.array([shift[0] * Z / F, shift[1] * Z / F, 0.0], np.float32)
        return R, (t + (np.eye(3, dtype=np.float32) - R) @ np.array([0, 0, Z], np.float32)).astype(np.float32)

    model = capi.Model(ctx, 5000)
    for i, (theta_deg, shift) in enumerate(TRAIN_VIEWS):
        theta = np.deg2rad(theta_deg)
        img = _render(texture, theta, shift, 100 + i) if i else texture
        c, s = np.cos(theta), np.sin(theta)
        x, y = u2 - W / 2.0 - shift[0], v2 - H / 2.0 - shift[1]
        u1, v1 = c * x + s * y + W / 2.0, -s * x + c * y + H / 2.0
        mask = (((u1 >= 0) & (u1 <= W - 1) & (v1 >= 0) & (v1 <= H - 1) & border) * 255).astype(np.uint8)
        R, t = pose(theta, shift)
        model.add_observation(img, mask, depth, K, R, t, n_features=1500, n_levels=3, scale_factor=1.2)
    before, after = model.compact(*E2E_MERGE)
    desc, pts = model.finish(); model.close()
    print("rows %d -> %d" % (before, after))
    assert after == len(desc) and 800 < after < before
    rng = np.random.Generator(np.random.PCG64(9))
    d2 = rng.integers(0, 256, (2000, 32), dtype=np.uint8); p2 = (rng.random((2000, 3)) * 0.2).astype(np.float32)
    off = np.array([0, len(d2), len(d2) + len(desc)], np.uint32)
    spans = ctx.db_load(np.concatenate([d2, desc]), np.concatenate([p2, pts]), off)
    theta, shift = np.deg2rad(25.0), (30.0, -18.0)
    view = _render(texture, theta, shift, 5)
    kp, aux, qd = ctx.orb(view, 1000, 3, 1.2)
    cloud = np.stack([(u2 - K[0, 2]) * Z / F, (v2 - K[1, 2]) * Z / F, np.full((H, W), Z, np.float32)], axis=2).astype(np.float32)
    row_ptr, m, xyz = ctx.match(qd, 5, 55)
    poses = ctx.verify(kp, cloud, row_ptr, m, xyz, spans, 8, 2500, 0.01, capi.rng_new(1))
    assert len(poses) >= 1 and poses[0]["object"] == 1 and len(poses[0]["inliers"]) > 100
    R_true, t_true = pose(theta, shift)
    print("max |R - R_true| = %g, max |t - t_true| = %g" % (np.abs(poses[0]["R"] - R_true).max(), np.abs(poses[0]["t"] - t_true).max()))
    assert np.abs(poses[0]["R"] - R_true).max() < 0.02, (poses[0]["R"], R_true)
    assert np.abs(poses[0]["t"] - t_true).max() < 0.004, (poses[0]["t"], t_true)
    ctx.close()
