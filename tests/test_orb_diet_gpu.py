"""Stage A's resize from tap tables, compass test on four positions per lane and patch moments from four-pixel words, at the
smallest shapes where each can go wrong, against the CPU restatement (the contract of tests/test_orb_gpu.py: everything bit-exact, the
angle within 4.9e-4 degrees):
  level rows that end 1, 2 or 3 pixels into a lane's group of four (resize_kernel's byte tail), at level 0 for the FAST groups and at
  level 1 for the resize; levels at or under 62 pixels, which are resized but yield nothing; FAST tiles whose right edge cuts a
  group; noise, where pass 1's survivor list is as full as it gets; a constant image; a row stride; a mask; two geometries
  alternating on one context, so that the tap tables follow the captured sequence; a batch of three frames."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from test_orb_gpu import _equal
from tod_amd import capi

pytestmark = pytest.mark.gpu

NF, NL, SF = 500, 3, 1.2


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def textured(H, W, seed=0):
    """small rectangles of random grey on mid-grey and a little noise: corners every few pixels, also in the few pixels of a 70-row
    image that lie 31 inside every border"""
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    img = np.full((H, W), 128.0, np.float32)
    n = H * W // 20
    x0 = rng.integers(0, W, n); y0 = rng.integers(0, H, n); w = rng.integers(2, 10, n); h = rng.integers(2, 10, n)
    val = rng.integers(0, 256, n)
    for i in range(n):
        img[y0[i]:y0[i] + h[i], x0[i]:x0[i] + w[i]] = val[i]
    img += rng.normal(0, 2.0, (H, W))
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def noise(H, W, seed=5):
    img = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (H, W), dtype=np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def ref(H, W, kind="textured"):
    """the restatement's result for an image of this module, computed once and shared (read-only)"""
    out = O.orb({"textured": textured, "noise": noise}[kind](H, W), NF, NL, SF)
    for a in out:
        a.setflags(write=False)
    return out


def levels_of(want):
    return sorted(set(int(l) for l in want[1][:, 3]))


# H = 70: levels 1 and 2 are 58 and 49 rows, resized and empty. The widths leave 3, 1, 2 and 2 pixels in level 0's last group of four,
# and levels 1 of 62, 64, 65 and 108 pixels. 129 x 65 and 131 x 81: the third FAST tile of a row is 1 and 3 pixels wide; 131 x 81 has
# a level 1 of 109 x 68 that yields keypoints from resized pixels, its row ending 1 pixel into a group. 84 x 141 and 84 x 143: level 1
# is 70 rows of 118 and 119 pixels, 2 and 3 pixels into a group.
@pytest.mark.parametrize("H,W,top_level", [(70, 75, 0), (70, 77, 0), (70, 78, 0), (70, 130, 0), (65, 129, 0), (81, 131, 1), (84, 141, 1), (84, 143, 1)])
def test_rows_that_end_inside_a_group(ctx, H, W, top_level):
    want = ref(H, W)
    assert len(want[0]) > 0 and levels_of(want)[-1] == top_level and levels_of(want)[0] == 0
    _equal(ctx.orb(textured(H, W), NF, NL, SF), want)


def test_noise_fills_the_survivor_list(ctx):
    want = ref(81, 131, "noise")
    assert len(want[0]) > 20
    _equal(ctx.orb(noise(81, 131), NF, NL, SF), want)


def test_constant_image_yields_nothing(ctx):
    img = np.full((81, 131), 90, np.uint8)
    got = ctx.orb(img, NF, NL, SF)
    assert len(got[0]) == len(O.orb(img, NF, NL, SF)[0]) == 0


def test_row_stride_larger_than_the_width(ctx):
    import torch
    H, W, stride = 81, 131, 131 + 29
    want = ref(H, W)
    buf = np.random.Generator(np.random.PCG64(3)).integers(0, 256, (H, stride), dtype=np.uint8)
    buf[:, :W] = textured(H, W)
    d = torch.from_numpy(buf).cuda()
    out = [torch.zeros((NF, w), dtype=torch.uint8, device="cuda") for w in (8, 16, 32)]
    n = ctx.orb_device(d.data_ptr(), H, W, stride, NF, NL, SF, *[t.data_ptr() for t in out], NF)
    assert n == len(want[0])
    kp, aux, desc = (t.cpu().numpy()[:n] for t in out)
    _equal((kp.view(np.float32), aux.view(np.float32), desc), want)


def test_masked_call(ctx):
    H, W = 84, 143
    mask = np.zeros((H, W), np.uint8)
    mask[20:60, 25:100] = 255
    mask[38:44, 50:70] = 0
    want = O.orb(textured(H, W), NF, NL, SF, mask=mask)
    assert 0 < len(want[0]) < len(ref(H, W)[0])
    _equal(ctx.orb(textured(H, W), NF, NL, SF, mask=mask), want)


def test_two_geometries_alternating_on_one_context():
    """the tap tables belong to a geometry: they are refilled where the captured sequence is re-recorded, and only there"""
    c = capi.Context(0)
    for H, W in ((81, 131), (84, 143), (81, 131), (81, 131), (84, 143), (84, 141)):
        want = ref(H, W)
        assert levels_of(want)[-1] == 1
        _equal(c.orb(textured(H, W), NF, NL, SF), want)
    c.close()


def test_batch_of_three_frames(ctx):
    import torch
    H, W = 80, 96
    imgs = [textured(H, W, seed=s) for s in (1, 2, 3)]
    wants = [O.orb(img, NF, NL, SF) for img in imgs]
    assert all(len(w[0]) > 0 and levels_of(w)[-1] == 1 for w in wants)
    d = torch.from_numpy(np.stack(imgs)).cuda()
    out = [torch.zeros((3 * NF, w), dtype=torch.uint8, device="cuda") for w in (8, 16, 32)]
    n = ctx.orb_batch_device(d.data_ptr(), 3, H * W, H, W, W, NF, NL, SF, *[t.data_ptr() for t in out], NF)
    assert n == [len(w[0]) for w in wants]
    host = [t.cpu().numpy() for t in out]
    for f, want in enumerate(wants):
        kp, aux, desc = (np.ascontiguousarray(a[f * NF:f * NF + n[f]]) for a in host)
        _equal((kp.view(np.float32), aux.view(np.float32), desc), want)
