"""Stage A where the rest of the suite never goes: row and frame strides (copy_rows_kernel), an output capacity other than
n_features, rankings whose thresholds fall into huge classes of equal keys (rank_tiled_kernel over more than one tile), patches without
a direction, pyramids whose levels are too small or have no pixels at all, and one context alternating between masks and patterns.
Every comparison is the contract of tests/test_orb_gpu.py (_equal: everything bit-exact, the angle within 16 ulp of 360 = 4.9e-4 degrees) against the
CPU restatement, on the inputs of tests/orb_inputs.py; tests/test_orb_inputs_cpu.py pins that those inputs reach these paths.
Training has no device form that takes a stride (todhip_model_add_observation is a host form of packed images), so it has no
case here."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import orb_inputs as I
import pattern_learn_ref as P
from test_orb_gpu import _equal
from tod_amd import capi, synth

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 8                                                             # sentinel rows behind the last frame's capacity


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def image(name):
    img = {"lattice": I.dot_lattice, "blocks": I.binary_blocks, "image": lambda: synth.make_image(3),
           "flat": lambda: I.flat(480, 640),
           "q0": lambda: synth.make_image(4, H=240, W=320, n_rect=500), "q1": lambda: synth.make_image(5, H=240, W=320, n_rect=500),
           "qlattice": lambda: I.dot_lattice(240, 320, seed=3), "qflat": lambda: I.flat(240, 320),
           "small_lattice": I.small_lattice}[name]()
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def ref(name, nf, nl, sf):
    """the restatement's full result, computed once and shared (read-only)"""
    out = O.orb(image(name), nf, nl, sf)
    for a in out:
        a.setflags(write=False)
    return out


def check(got, want, img=None):
    """_equal, and the extra rule: a level-0 keypoint whose patch has both moments zero reports an angle of exactly 0.
    Returns how many such keypoints there were."""
    _equal(got, want)
    if img is None:
        return 0
    aux, lvl = want[1], want[3]
    zero = [i for i in np.flatnonzero(aux[:, 3] == 0) if I.disc_moments(img, int(lvl[i, 0]), int(lvl[i, 1])) == (0, 0)]
    assert (got[1][zero, 1] == 0).all()
    return len(zero)


def prefix(want, n):
    return tuple(a[:n] for a in want)


class DeviceOut:
    """Device outputs of F frames of `cap` rows plus guard rows, every byte a sentinel"""

    def __init__(self, F, cap):
        import torch
        self.F, self.cap, rows = F, cap, F * cap + GUARD
        self.t = [torch.full((rows * w,), SENTINEL, dtype=torch.uint8, device="cuda") for w in (8, 16, 32)]

    def ptrs(self):
        return [t.data_ptr() for t in self.t]

    def frame(self, f, n):
        """(kp, aux, desc) of frame f's first n rows, and whether every byte behind them (up to the next frame) is still the sentinel"""
        lo, hi = f * self.cap, (f + 1) * self.cap + (GUARD if f == self.F - 1 else 0)
        h = [t.cpu().numpy().reshape(-1, w) for t, w in zip(self.t, (8, 16, 32))]
        untouched = all((a[lo + n:hi] == SENTINEL).all() for a in h)
        kp, aux, desc = (np.ascontiguousarray(a[lo:lo + n]) for a in h)
        return (kp.view(np.float32), aux.view(np.float32), desc), untouched


def to_device(buf):
    import torch
    return torch.from_numpy(np.array(buf, np.uint8)).cuda()                # (a copy: the shared images are read-only)


def orb_device(ctx, img, nf, nl, sf, cap, stride=None):
    """todhip_orb_device on one frame -> (n_out, DeviceOut)"""
    H, W = img.shape
    d = to_device(img if stride is None else I.padded(img, stride)[0])
    out = DeviceOut(1, cap)
    n = ctx.orb_device(d.data_ptr(), H, W, stride or W, nf, nl, sf, *out.ptrs(), cap)
    return n, out


def batch_buffer(imgs, stride, frame_stride, seed=11):
    """the frames at row pitch `stride`, frame f at byte f * frame_stride, in a buffer that ends with the last frame's last pixel;
    every byte between rows and frames is random"""
    H, W = imgs[0].shape
    rng = np.random.Generator(np.random.PCG64(seed))
    buf = rng.integers(0, 256, (len(imgs) - 1) * frame_stride + (H - 1) * stride + W, dtype=np.uint8)
    for f, img in enumerate(imgs):
        np.lib.stride_tricks.as_strided(buf[f * frame_stride:], (H, W), (stride, 1))[:] = img
    return buf


def orb_batch(ctx, imgs, nf, nl, sf, cap, stride=None, frame_stride=None):
    H, W = imgs[0].shape
    stride = stride or W
    frame_stride = frame_stride or H * stride
    d = to_device(batch_buffer(imgs, stride, frame_stride))
    out = DeviceOut(len(imgs), cap)
    n = ctx.orb_batch_device(d.data_ptr(), len(imgs), frame_stride, H, W, stride, nf, nl, sf, *out.ptrs(), cap)
    return n, out


def ordinary_call_still_right(ctx):
    """after a degenerate call in the same context: the captured sequence is rebuilt for an ordinary geometry"""
    got = ctx.orb(image("q0"), 300, 3, 1.2)
    _equal(got, ref("q0", 300, 3, 1.2))
    assert len(got[0]) == 300


# ------------------------------------------------------------------------------------------ a. ranking and ties
@pytest.mark.parametrize("name,nf,nl,n_expected,zero_at_least", [
    ("lattice", 1000, 1, 1000, 200),      # keep = 2000 inside the top class of 2482: nothing above the threshold, ties > one rank tile
    ("lattice", 1500, 1, 1500, 200),      # threshold class 100: 2482 sure, 518 of 640 ties kept
    ("lattice", 2500, 1, 2500, 200),      # no threshold; the Harris ranking of 3744 > 2048 records is nearly all ties
    ("lattice", 5000, 1, 3744, 200),      # fewer candidates than wanted
    ("lattice", 1000, 3, 1000, 200),
    ("blocks", 1000, 3, 604, 0),          # scores up to 255, plateaus, the largest Harris sums
])
def test_ranking_and_ties(ctx, name, nf, nl, n_expected, zero_at_least):
    want = ref(name, nf, nl, 1.2)
    assert len(want[0]) == n_expected
    got = ctx.orb(image(name), nf, nl, 1.2)
    assert check(got, want, image(name) if zero_at_least else None) >= zero_at_least


def test_fewer_candidates_than_wanted_leaves_the_rest_alone(ctx):
    want = ref("lattice", 5000, 1, 1.2)
    n, out = orb_device(ctx, image("lattice"), 5000, 1, 1.2, 5000)
    assert n == 3744 == len(want[0])
    got, untouched = out.frame(0, n)
    _equal(got, want)
    assert untouched                                                   # rows 3744 .. of the outputs


# ------------------------------------------------------------------------------------------ b. capacity
@pytest.mark.parametrize("cap", [1, 300, 396, 397, 999, 1500])
@pytest.mark.parametrize("name", ["lattice", "image"])
def test_capacity_cuts_a_prefix(ctx, name, cap):
    """levels hold 396 / 330 / 274 keypoints on the lattice: capacities inside a level, at a level's end, one behind it, one short of
    everything and beyond everything"""
    full = ref(name, 1000, 3, 1.2)
    assert len(full[0]) == 1000
    n_want = min(cap, 1000)
    got = ctx.orb(image(name), 1000, 3, 1.2, cap=cap)
    assert len(got[0]) == n_want
    _equal(got, prefix(full, n_want))
    n, out = orb_device(ctx, image(name), 1000, 3, 1.2, cap)
    assert n == n_want
    d_got, untouched = out.frame(0, n)
    _equal(d_got, prefix(full, n_want))
    assert untouched
    assert all(np.array_equal(a, b) for a, b in zip(got, d_got))      # host and device forms: the same bits, the angle too


def test_capacity_of_a_batch(ctx):
    names, cap = ["lattice", "flat", "image"], 500
    n, out = orb_batch(ctx, [image(k) for k in names], 1000, 3, 1.2, cap)
    assert n == [500, 0, 500]
    for f, k in enumerate(names):
        got, untouched = out.frame(f, n[f])
        _equal(got, prefix(ref(k, 1000, 3, 1.2), n[f]))
        assert untouched, k


# ------------------------------------------------------------------------------------------ c. strides
QNF, QNL, QSF = 300, 3, 1.2                                            # the 240 x 320 frames' arguments


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("pad", [1, 37])
def test_host_form_with_a_row_stride(ctx, pad, masked):
    """the buffers end with the last row's W pixels; the padding is random, in the image and in the mask (which shares the stride)"""
    img = image("q0")
    H, W = img.shape
    stride = W + pad
    mask = None
    if masked:
        mask = np.zeros(img.shape, np.uint8)
        mask[40:200, 50:300] = 255
        mask[100:130, 150:200] = 0
    want = O.orb(img, QNF, QNL, QSF, mask=mask)
    assert len(want[0]) > 100
    buf, rows = I.padded(img, stride)
    assert buf.size == (H - 1) * stride + W
    mrows = None if mask is None else I.padded(mask, stride, seed=8)[1]
    got = ctx.orb(rows, QNF, QNL, QSF, mask=mrows, stride=stride, W=W)
    _equal(got, want)
    packed = ctx.orb(img, QNF, QNL, QSF, mask=mask)
    assert all(np.array_equal(a, b) for a, b in zip(got, packed))


def test_device_form_with_a_row_stride(ctx):
    img, want = image("q0"), ref("q0", QNF, QNL, QSF)
    n, out = orb_device(ctx, img, QNF, QNL, QSF, QNF, stride=320 + 37)
    assert n == len(want[0]) == QNF
    got, untouched = out.frame(0, n)
    _equal(got, want)
    assert untouched
    n_p, out_p = orb_device(ctx, img, QNF, QNL, QSF, QNF)
    assert n_p == n and all(np.array_equal(a, b) for a, b in zip(got, out_p.frame(0, n)[0]))


@pytest.mark.parametrize("names,pad,gap", [
    (("q0", "qlattice", "q1"), 0, 4096),       # packed rows, frames apart
    (("q0", "qlattice", "q1"), 37, 123),       # padded rows, frames apart by an odd number of bytes
    (("q1",), 37, 0),                          # one strided frame through the batch form
])
def test_batch_forms_with_strides(ctx, names, pad, gap):
    imgs = [image(k) for k in names]
    H, W = imgs[0].shape
    stride = W + pad
    n, out = orb_batch(ctx, imgs, QNF, QNL, QSF, QNF, stride=stride, frame_stride=H * stride + gap)
    n_p, out_p = orb_batch(ctx, imgs, QNF, QNL, QSF, QNF)
    assert n == n_p
    for f, k in enumerate(names):
        want = ref(k, QNF, QNL, QSF)
        assert n[f] == len(want[0]) > 100
        got, untouched = out.frame(f, n[f])
        _equal(got, want)
        assert untouched, k
        assert all(np.array_equal(a, b) for a, b in zip(got, out_p.frame(f, n[f])[0]))


# ------------------------------------------------------------------------------------------ d. degenerate pyramids
def degenerate(ctx, img, nf, nl, sf, count):
    want = O.orb(img, nf, nl, sf)
    assert len(want[0]) == count
    got = ctx.orb(img, nf, nl, sf)
    check(got, want, img)
    ordinary_call_still_right(ctx)
    flat = I.flat(*img.shape)
    n, out = orb_batch(ctx, [img, flat, img], nf, nl, sf, nf)
    assert n == [count, 0, count]
    for f in (0, 1, 2):
        b_got, untouched = out.frame(f, n[f])
        _equal(b_got, want if f != 1 else prefix(want, 0))
        assert untouched
    ordinary_call_still_right(ctx)
    return got


@pytest.mark.parametrize("shape,count", sorted(I.TINY_SHAPES.items()))
def test_tiny_images(ctx, shape, count):
    """no admissible level at all (nothing is launched, 0 keypoints), and the smallest image that has one admissible pixel"""
    kp, _, _ = degenerate(ctx, I.tiny(*shape), 10, 1, 1.2, count)
    assert kp.tolist() == ([[31.0, 31.0]] if count else [])


@pytest.mark.parametrize("case,count", sorted(I.SMALL_LATTICE_CASES.items()))
def test_levels_of_zero_pixels(ctx, case, count):
    """the upper levels round to 1 x 1 and 0 x 0 pixels: they are in the level table, ask for nothing and launch nothing"""
    degenerate(ctx, image("small_lattice"), 50, case[0], case[1], count)


def status_of(call):
    try:
        call()
    except capi.TodError as e:
        return e.status
    return capi.OK


def test_refused_arguments(ctx):
    import torch
    img = image("q0")
    assert status_of(lambda: ctx.orb(np.zeros((7, 320), np.uint8), 100, 1, 1.2)) == capi.EINVAL
    assert status_of(lambda: ctx.orb(img, 100, 0, 1.2)) == capi.EINVAL
    assert status_of(lambda: ctx.orb(img, 100, 17, 1.2)) == capi.EINVAL
    assert status_of(lambda: ctx.orb(img, 100, 3, 1.0)) == capi.EINVAL
    assert status_of(lambda: ctx.orb(img, 100, 3, 1.2, cap=0)) == capi.ECAPACITY
    # the device forms are refused before anything is read or written: one small buffer stands for every pointer
    d = torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()
    H, W = 240, 320
    batch = lambda F, nl, fs, cap=100, sf=1.2, H=H: ctx.orb_batch_device(p, F, fs, H, W, W, 100, nl, sf, p, p, p, cap)
    assert status_of(lambda: batch(4096, 16, H * W)) == capi.EINVAL            # n_levels * n_frames = 65536 (level, frame) pairs
    assert status_of(lambda: batch(2, 3, H * W - 1)) == capi.EINVAL            # frames overlap
    assert status_of(lambda: batch(1, 0, H * W)) == capi.EINVAL
    assert status_of(lambda: batch(1, 17, H * W)) == capi.EINVAL
    assert status_of(lambda: batch(1, 3, H * W, sf=1.0)) == capi.EINVAL
    assert status_of(lambda: batch(1, 3, 7 * W, H=7)) == capi.EINVAL
    assert status_of(lambda: batch(1, 3, H * W, cap=0)) == capi.ECAPACITY
    assert status_of(lambda: ctx.orb_device(p, H, W, W, 100, 3, 1.2, p, p, p, 0)) == capi.ECAPACITY
    assert status_of(lambda: ctx.orb_device(p, H, W, W - 1, 100, 3, 1.2, p, p, p, 100)) == capi.EINVAL   # stride < W
    assert (d.cpu().numpy() == SENTINEL).all()
    ordinary_call_still_right(ctx)


# ------------------------------------------------------------------------------------------ e. one context, alternating
def test_one_context_alternating_masks_and_patterns():
    """same geometry throughout, so only the mask pointer and the pattern decide between replaying and re-recording"""
    ctx = capi.Context(0)
    img = image("q0")
    m1 = np.zeros(img.shape, np.uint8); m1[30:210, 40:200] = 255
    m2 = np.zeros(img.shape, np.uint8); m2[60:230, 120:310] = 255; m2[100:140, 200:260] = 0
    custom = np.ascontiguousarray(O.orb_default_pattern()[::-1])
    results = []
    for mask, pattern in ((m1, None), (None, None), (m2, None), (None, custom), (None, None), (m1, custom), (m1, None)):
        want = O.orb(img, QNF, QNL, QSF, pattern=pattern, mask=mask)
        assert len(want[0]) > 100
        got = ctx.orb(img, QNF, QNL, QSF, pattern=pattern, mask=mask)
        _equal(got, want)
        results.append(got)
    assert not np.array_equal(results[1][2], results[3][2])           # the custom pattern is another pattern
    assert np.array_equal(results[1][2], results[4][2]) and not np.array_equal(results[0][0], results[1][0])
    ctx.close()


def test_one_context_through_the_graph_cache():
    """The captured launch sequence's transitions in one fresh context, every call against the restatement: first capture, a geometry
    without an admissible level (nothing is launched and the captured sequence goes), capture again, replay, a batch (the frame count
    is part of the key), one frame again. TODHIP_ORB_NO_GRAPH is read once per process, so it stays as the suite was started: unset,
    this walks the cache; set, the same calls launch directly."""
    ctx = capi.Context(0)
    img, (nl, sf), nf = image("small_lattice"), (16, 1.5), 50         # two levels yield keypoints, the upper ones have no pixels
    want = ref("small_lattice", nf, nl, sf)
    assert len(want[0]) == I.SMALL_LATTICE_CASES[(nl, sf)] == 17
    nothing = I.tiny(62, 62)
    assert I.TINY_SHAPES[(62, 62)] == 0
    _equal(ctx.orb(img, nf, nl, sf), want)                             # A: captures
    got = ctx.orb(nothing, 10, 1, 1.2)                                 # B: drops
    assert len(got[0]) == len(got[1]) == len(got[2]) == 0
    _equal(got, O.orb(nothing, 10, 1, 1.2))
    _equal(ctx.orb(img, nf, nl, sf), want)                             # A: captures again
    _equal(ctx.orb(img, nf, nl, sf), want)                             # A: replays
    n, out = orb_batch(ctx, [img, img], nf, nl, sf, nf)                # A twice in one call
    assert n == [17, 17]
    for f in (0, 1):
        b_got, untouched = out.frame(f, n[f])
        _equal(b_got, want)
        assert untouched
    _equal(ctx.orb(img, nf, nl, sf), want)                             # A: one frame again
    ctx.close()


# ------------------------------------------------------------------------------------------ f. the learner through a stride
def test_learner_view_through_a_stride(ctx):
    gray, mask = P.learn_views()[1]
    H, W = gray.shape
    stride = W + 37
    cands = P.crafted_candidates()
    d_mask = to_device(mask)                                           # the mask keeps row pitch W
    got = []
    for buf, s in ((gray, W), (I.padded(gray, stride)[0], stride)):
        d_gray = to_device(buf)
        L = capi.PatternLearner(ctx, 1000, cands)
        n = L.add_view_device(d_gray.data_ptr(), d_mask.data_ptr(), H, W, s, P.NF, P.LEVELS, P.SCALE)
        got.append((n, L.responses(0, len(cands))))
        L.close()
    assert got[0][0] == got[1][0] == len(O.orb(gray, P.NF, P.LEVELS, P.SCALE, mask=mask)[0]) > 50
    assert got[0][1].any() and np.array_equal(got[0][1], got[1][1])
    # and the host form at that stride, from a buffer that ends with the last row's pixels
    L = capi.PatternLearner(ctx, 1000, cands)
    n = add_view_strided(ctx, L, I.padded(gray, stride)[1], I.padded(mask, stride, seed=8)[1], stride, W)
    assert n == got[0][0] and np.array_equal(L.responses(0, len(cands)), got[0][1])
    L.close()


def add_view_strided(ctx, L, rows, mrows, stride, W):
    """todhip_pattern_learn_add_view with a row stride (PatternLearner.add_view packs its views)"""
    import ctypes as C
    n = C.c_uint32(0)
    rc = capi.lib().todhip_pattern_learn_add_view(ctx._h, L._h, C.c_void_p(rows.ctypes.data), C.c_void_p(mrows.ctypes.data),
                                                  C.c_uint32(rows.shape[0]), C.c_uint32(W), C.c_uint32(stride), C.c_uint32(P.NF),
                                                  C.c_uint32(P.LEVELS), C.c_float(P.SCALE), C.byref(n))
    assert rc == capi.OK
    L.n_keypoints += n.value
    return n.value
