"""todhip_model_add_observations_device (tod_amd/csrc/train.hip: one batched masked ORB call, validate_batch_kernel, count / scan /
append_batch_kernel) against its definition: the model after the call is byte for byte the model after todhip_rescale_depth +
todhip_model_add_observation per view, in order. Inputs are tests/train_ref.py's cases; a view of a case is its image under its comb
mask (`orig`), both reversed along the columns (`fliplr`), the image under an all-zero mask (`closed`: no keypoint), the image reversed
along the rows under an all-255 mask (`flipud_open`), and the image under an all-255 mask (`orig_open`). All views of a case share its
depth, in float and in uint16. Every comb-mask view holds all four classes of validateKeyPoints, and one open vga_chunk2 view alone
accepts more than 1024 rows. Expected values come from a fresh model through the existing single-view calls on the same context; one
case uses the independent numpy statement on the CPU restatement's keypoints as well. Descriptors are compared by bytes, points with
train_ref.same_points (equal bytes where not NaN, NaN in the same places), and n_added per view. Every non-closed view must add rows,
so a wrong input cannot pass silently."""
import ctypes as C
import functools

import numpy as np
import pytest

import train_ref as TR
from tod_amd import capi

pytestmark = pytest.mark.gpu

BATCHES = (("orig",), ("orig", "fliplr"), ("closed", "orig", "closed"), ("fliplr", "closed", "orig_open", "orig", "flipud_open"))


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _view(name, kind):
    c = TR.case(name)
    img, mask = c["img"], c["mask"]
    opn = np.full(img.shape, 255, np.uint8)
    img, mask = {"orig": (img, mask), "fliplr": (img[:, ::-1], mask[:, ::-1]), "closed": (img, np.zeros_like(mask)),
                 "flipud_open": (img[::-1], opn), "orig_open": (img, opn)}[kind]
    img, mask = np.ascontiguousarray(img), np.ascontiguousarray(mask)
    img.setflags(write=False); mask.setflags(write=False)
    return img, mask


def _cameras(name, n):
    """a camera per view: fx != fy, the principal point moved with the view, a rotation and a matrix that is none in turn, T scaled"""
    W = TR.case(name)["img"].shape[1]
    K = np.stack([TR.camera(W, 160.25 + v) for v in range(n)])
    R = np.stack([TR.rotation_skew_axis() if v % 2 == 0 else TR.general_matrix() for v in range(n)])
    T = np.stack([TR.T * np.float32(v + 1) for v in range(n)])
    return K, R, T


def _orb_args(name, n_levels=None):
    c = TR.case(name)
    return dict(n_features=c["n_features"], n_levels=c["n_levels"] if n_levels is None else n_levels, scale_factor=c["scale_factor"])


def _upload(a):
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
    torch.cuda.synchronize()                                    # torch's stream is not the context's
    return t


def _sequence(model, name, kinds, depth, pattern=None, first_camera=0):
    """the definition: one add_observation per view -> n_added per view. depth: [H, W] float32 or uint16, shared by the views"""
    K, R, T = _cameras(name, first_camera + len(kinds))
    out = []
    for v, kind in enumerate(kinds):
        img, mask = _view(name, kind)
        out.append(model.add_observation(img, mask, depth, K[first_camera + v], R[first_camera + v], T[first_camera + v], pattern=pattern,
                                         **_orb_args(name)))
    return np.asarray(out, np.uint32)


def _batch(model, name, kinds, depth, pattern=None, stride=None, frame_stride=None, depth_size=None, nearest=False):
    """the same views in one call. depth: [dH, dW], shared by the views (uploaded once per view, packed)"""
    n = len(kinds)
    H, W = TR.case(name)["img"].shape
    imgs = np.stack([_view(name, k)[0] for k in kinds])
    masks = np.stack([_view(name, k)[1] for k in kinds])
    if stride is not None:                                      # rows of `stride` bytes, frames of frame_stride bytes, 255 in between
        buf = np.full(n * frame_stride, 255, np.uint8)
        for v in range(n):
            rows = buf[v * frame_stride: v * frame_stride + H * stride].reshape(H, stride)
            rows[:, :W] = imgs[v]
        imgs = buf
    d_gray, d_mask, d_depth = _upload(imgs), _upload(masks), _upload(np.stack([depth] * n))
    K, R, T = _cameras(name, n)
    return model.add_observations_device(d_gray.data_ptr(), d_mask.data_ptr(), d_depth.data_ptr(), n, H, W, K, R, T, stride=stride,
                                         frame_stride=frame_stride, depth_is_u16=depth.dtype == np.uint16, depth_size=depth_size,
                                         nearest=nearest, pattern=pattern, **_orb_args(name))


def _finish(model):
    desc, pts = model.finish()
    model.close()
    return desc, pts


def _same_model(got, want):
    return len(got[0]) == len(want[0]) and np.array_equal(got[0], want[0]) and TR.same_points(got[1], want[1])


def _open_views_added(kinds, n_added):
    return all(int(n) > 0 for k, n in zip(kinds, n_added) if k != "closed") and all(int(n) == 0 for k, n in zip(kinds, n_added) if k == "closed")


def _both(ctx, name, kinds, depth, capacity=9000, rows=None, **kw):
    """(model by the sequence, its n_added, model by the batch, its n_added), each from a fresh model (holding `rows` first)"""
    res = []
    for fn, extra in ((_sequence, {}), (_batch, kw)):
        model = capi.Model(ctx, capacity)
        if rows is not None:
            assert model.add_rows(*rows) == min(len(rows[0]), capacity)
        n_added = fn(model, name, kinds, depth, **extra)
        res += [_finish(model), n_added]
    return res


@pytest.mark.parametrize("kinds", BATCHES, ids=lambda k: "-".join(k))
@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
@pytest.mark.parametrize("name", ["tiny", "qvga"])
def test_batch_equals_sequence(ctx, name, u16, kinds):
    c = TR.case(name)
    want, n_want, got, n_got = _both(ctx, name, kinds, c["d16"] if u16 else c["z"])
    print(name, kinds, "n_added", n_want.tolist(), n_got.tolist())
    assert _open_views_added(kinds, n_want)
    assert np.array_equal(n_got, n_want) and len(got[0]) == int(n_want.sum())
    assert _same_model(got, want)


def test_independent_statement(ctx):
    """expected rows from tests/train_ref.py's numpy statement on the CPU restatement's masked ORB keypoints, view by view"""
    import oracle_lib as O
    name, kinds = "qvga", ("orig", "fliplr")
    c = TR.case(name)
    K, R, T = _cameras(name, len(kinds))
    rows = []
    for v, kind in enumerate(kinds):
        img, mask = _view(name, kind)
        kp, _, desc, _ = O.orb(img, c["n_features"], c["n_levels"], c["scale_factor"], mask=mask)
        rows.append(TR.observation(kp, desc, mask, c["z"], K[v], R[v], T[v]))
    model = capi.Model(ctx, 4000)
    n_added = _batch(model, name, kinds, c["z"])
    got = _finish(model)
    assert [len(r[0]) for r in rows] == n_added.tolist() and min(n_added) > 100
    assert _same_model(got, (np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])))


def test_more_than_1024_accepted_rows_in_one_view(ctx):
    name, kinds = "vga_chunk2", ("orig_open", "orig", "flipud_open")
    want, n_want, got, n_got = _both(ctx, name, kinds, TR.case(name)["z"])
    print("n_added", n_want.tolist())
    assert n_want[0] > 1024 and n_want[2] > 1024 and n_want[1] > 0
    assert np.array_equal(n_got, n_want) and _same_model(got, want)


def test_capacity_cut(ctx):
    """the cut inside view 1 (view 2 adds 0), exactly between views 0 and 1, after one row; and behind rows the model already held"""
    name, kinds = "qvga", ("orig", "fliplr", "orig_open")
    z = TR.case(name)["z"]
    _, a, _, _ = _both(ctx, name, kinds, z)
    a = [int(x) for x in a]
    assert min(a) > 2
    for cap, want_added in ((a[0] + a[1] // 2, [a[0], a[1] // 2, 0]), (a[0], [a[0], 0, 0]), (1, [1, 0, 0])):
        want, n_want, got, n_got = _both(ctx, name, kinds, z, capacity=cap)
        assert n_want.tolist() == want_added and n_got.tolist() == want_added, cap
        assert len(got[0]) == cap and _same_model(got, want), cap
    rng = np.random.Generator(np.random.PCG64(9))
    held = (rng.integers(0, 256, (a[0] // 2, 32), dtype=np.uint8), rng.random((a[0] // 2, 3)).astype(np.float32))
    for cap in (9000, a[0] // 2 + a[0] + 3):
        want, n_want, got, n_got = _both(ctx, name, kinds, z, capacity=cap, rows=held)
        assert np.array_equal(n_got, n_want) and _same_model(got, want), cap
        assert np.array_equal(got[0][:len(held[0])], held[0]) and np.array_equal(got[1][:len(held[0])], held[1])
        assert n_want.tolist() == (a if cap == 9000 else [a[0], 3, 0])


def test_strides(ctx):
    """rows of W + 13 bytes, frames H * stride + 64 bytes apart, 255 between the rows and the frames: the result of the packed call"""
    name, kinds = "qvga", ("orig", "fliplr", "orig_open")
    c = TR.case(name)
    H, W = c["img"].shape
    res = []
    for kw in ({}, dict(stride=W + 13, frame_stride=H * (W + 13) + 64)):
        model = capi.Model(ctx, 4000)
        n_added = _batch(model, name, kinds, c["d16"], **kw)
        res.append((_finish(model), n_added))
    assert _open_views_added(kinds, res[0][1])
    assert np.array_equal(res[0][1], res[1][1]) and _same_model(res[1][0], res[0][0])


@pytest.mark.parametrize("nearest", [False, True], ids=["bilinear", "nearest"])
@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
@pytest.mark.parametrize("size", [(120, 160), (480, 640)])
def test_depth_at_the_sensors_size(ctx, size, u16, nearest):
    """depth of half and of twice the image's size: the sequence rescales it for every view (Context.rescale_depth), the batch does not"""
    name, kinds = "qvga", ("orig", "fliplr")
    H, W = TR.case(name)["img"].shape
    z, _ = TR.special_depth(23, *size)
    depth = TR.depth_u16(z) if u16 else z
    model = capi.Model(ctx, 4000)
    n_want = _sequence(model, name, kinds, ctx.rescale_depth(depth, H, W, nearest))
    want = _finish(model)
    model = capi.Model(ctx, 4000)
    n_got = _batch(model, name, kinds, depth, depth_size=size, nearest=nearest)
    got = _finish(model)
    print(size, u16, nearest, "n_added", n_want.tolist())
    assert _open_views_added(kinds, n_want)
    assert np.array_equal(n_got, n_want) and _same_model(got, want)


def test_refused_depth_geometry_leaves_the_model(ctx):
    name, kinds = "qvga", ("orig",)
    c = TR.case(name)
    model = capi.Model(ctx, 4000)
    _batch(model, name, kinds, c["z"])
    before = model.finish()
    with pytest.raises(capi.TodError) as e:                     # 240 x 80 -> 320 columns is 960 rows: they do not fit into 240
        _batch(model, name, kinds, np.ones((240, 80), np.float32), depth_size=(240, 80))
    assert e.value.status == capi.EINVAL
    after = _finish(model)
    assert len(before[0]) > 0 and np.array_equal(after[0], before[0]) and np.array_equal(after[1].view(np.uint32), before[1].view(np.uint32))


def _history(ctx, batched):
    """a tiny batch, a single qvga observation, a qvga batch with another pattern, a compaction, a tiny batch again"""
    add = _batch if batched else _sequence
    tiny, qvga = TR.case("tiny"), TR.case("qvga")
    model = capi.Model(ctx, 6000)
    counts = [add(model, "tiny", ("orig", "fliplr"), tiny["z"])]
    counts.append(_sequence(model, "qvga", ("orig",), qvga["d16"], first_camera=2))
    counts.append(add(model, "qvga", ("fliplr", "orig_open"), qvga["z"], pattern=TR.permuted_pattern(3)))
    counts.append(np.asarray(model.compact(0.01, 256), np.uint32))   # (points within a centimetre, whatever the descriptors)
    counts.append(add(model, "tiny", ("closed", "orig", "flipud_open"), tiny["d16"]))
    return _finish(model), np.concatenate(counts)


def test_one_model_through_changing_shapes_and_mixed_calls(ctx):
    want, n_want = _history(ctx, False)
    runs = [_history(ctx, True) for _ in range(2)]
    print("counts", n_want.tolist())
    assert (n_want[[0, 1, 2, 3, 4, 8, 9]] > 0).all() and n_want[5] > n_want[6]          # every open view adds rows, the compaction merges some
    for got, n_got in runs:
        assert np.array_equal(n_got, n_want) and _same_model(got, want)
    assert np.array_equal(runs[0][0][0], runs[1][0][0]) and np.array_equal(runs[0][0][1].view(np.uint32), runs[1][0][1].view(np.uint32))


def test_orb_launch_graph_cache_between_masked_batches_unmasked_batches_and_single_views():
    """on one context: a masked training batch, orb_batch_device without a mask on the same shape, add_observation, twice over; each
    gives what it gives on a fresh context"""
    import torch
    name, kinds = "qvga", ("orig", "fliplr")
    c = TR.case(name)
    H, W = c["img"].shape
    nf, args = c["n_features"], _orb_args(name)
    d_imgs = _upload(np.stack([_view(name, k)[0] for k in kinds]))

    def train_batch(cx):
        model = capi.Model(cx, 4000)
        n = _batch(model, name, kinds, c["z"])
        return _finish(model) + (n,)

    def orb_unmasked(cx):
        kp = torch.zeros((2, nf, 2), device="cuda"); aux = torch.zeros((2, nf, 4), device="cuda")
        desc = torch.zeros((2, nf, 32), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        n = cx.orb_batch_device(d_imgs.data_ptr(), 2, H * W, H, W, W, nf, args["n_levels"], args["scale_factor"], kp.data_ptr(), aux.data_ptr(),
                                desc.data_ptr(), nf)
        return kp.cpu().numpy(), desc.cpu().numpy(), np.asarray(n, np.uint32)

    def single(cx):
        model = capi.Model(cx, 4000)
        n = _sequence(model, name, ("orig",), c["d16"])
        return _finish(model) + (n,)

    def fresh(fn):
        cx = capi.Context(0)
        try:
            return fn(cx)
        finally:
            cx.close()
    steps = (train_batch, orb_unmasked, single)
    want = [fresh(fn) for fn in steps]
    assert want[0][2].min() > 0 and want[1][2].min() > want[0][2].max() and want[2][2].min() > 0   # (no mask: more keypoints)
    cx = capi.Context(0)
    try:
        for _ in range(2):
            for fn, w in zip(steps, want):
                got = fn(cx)
                assert np.array_equal(got[2], w[2]), fn.__name__
                if fn is orb_unmasked:
                    assert all(np.array_equal(got[0][f, :w[2][f]], w[0][f, :w[2][f]]) and np.array_equal(got[1][f, :w[2][f]], w[1][f, :w[2][f]])
                               for f in range(2))
                else:
                    assert _same_model(got[:2], w[:2]), fn.__name__
    finally:
        cx.close()


def test_refusals_leave_the_model(ctx):
    """every refusal of the header's list, on a model that holds rows: TODHIP_EINVAL, n_added untouched, the same rows afterwards"""
    name = "tiny"
    c = TR.case(name)
    H, W = c["img"].shape
    model = capi.Model(ctx, 4000)
    _batch(model, name, ("orig", "fliplr"), c["z"])
    before = model.finish()
    assert len(before[0]) > 0
    n = 2
    d_gray, d_mask = _upload(np.stack([_view(name, "orig")[0]] * n)), _upload(np.stack([_view(name, "orig")[1]] * n))
    d_depth = _upload(np.stack([c["z"]] * n))
    K, R, T = (np.ascontiguousarray(a.reshape(-1)) for a in _cameras(name, n))
    n_added = (C.c_uint32 * 64)(*([7] * 64))
    L = capi.lib()

    def call(ctx_h=ctx._h, model_h=model._h, gray=d_gray.data_ptr(), fs=H * W, stride=W, mask=d_mask.data_ptr(), depth=d_depth.data_ptr(),
             dH=0, dW=0, n_views=n, h=H, w=W, k=K.ctypes.data, r=R.ctypes.data, t=T.ctypes.data, n_features=500, n_levels=2, sf=1.2):
        return L.todhip_model_add_observations_device(ctx_h, model_h, gray, fs, stride, mask, depth, 0, dH, dW, 0, n_views, h, w, k, r, t,
                                                      n_features, n_levels, sf, None, n_added)
    refused = (dict(ctx_h=None), dict(model_h=None), dict(gray=None), dict(depth=None), dict(k=None), dict(r=None), dict(t=None),
               dict(h=7), dict(w=7, stride=7), dict(n_features=0), dict(n_levels=0), dict(n_levels=17), dict(sf=1.0),
               dict(mask=None), dict(n_views=0), dict(n_views=65), dict(stride=W - 1), dict(fs=H * W - 1),
               dict(stride=W + 8, fs=H * (W + 8) - 1), dict(dH=H), dict(dW=W), dict(dH=H, dW=W // 4), dict(dH=1, dW=16 * W))
    for kw in refused:
        assert call(**kw) == capi.EINVAL, kw
        after = model.finish()
        assert np.array_equal(after[0], before[0]) and np.array_equal(after[1].view(np.uint32), before[1].view(np.uint32)), kw
    assert list(n_added) == [7] * 64
    assert call() == capi.OK and list(n_added[:2]) != [7, 7]   # and the same call without a fault is accepted
    model.close()


def test_scenes_train_db_batched(ctx):
    from tod_amd import scenes
    tex = scenes.make_textures(2)
    want = scenes.train_db(ctx, tex, batched=False)
    got = scenes.train_db(ctx, tex, batched=True)
    assert len(want[0]) > 500 and np.array_equal(got[2], want[2])
    assert np.array_equal(got[0], want[0]) and TR.same_points(got[1], want[1])
