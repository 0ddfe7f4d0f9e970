"""fast_nms_kernel's suppression over the survivor list (tod_amd/csrc/orb_fast.h), at the places where a walk over list entries can
differ from a walk over tile positions, against the CPU restatement (keypoints and descriptors, the contract of tests/test_orb_gpu.py)
and, at one level with room for every candidate, against candidates() below: an independent numpy statement of the score, its border
rule, the strict 3 x 3 suppression and the mask. (The candidate list and its histogram are not reachable from outside the library;
with n_features above the number of candidates every candidate is a keypoint, and with n_features far below it the histogram's
threshold decides the keypoints, which the restatement then fixes.)

A block scores a 64 x 16 tile and one pixel around it; images here are 96 x 80 to 200 x 80, so tiles start at x = 0, 64, 128 and
y = 0, 16, .. 64, and keypoints lie in x = 31 .. w - 32, y = 31 .. h - 32. A lone pixel above a flat background scores its contrast
and nothing around it scores: every such dot is a corner of known score at a known place.

  noise: every position passes pass 1, the list is full and the walk as long as the tile;
  a flat image: the list is empty;
  one dot at each corner of a tile, on each of its edge rows and columns (its 3 x 3 neighbourhood lies in the halo), at kEdge and at
    w - kEdge - 1, h - kEdge - 1, and one pixel outside each (scored for its neighbours' sake, never kept);
  two adjacent dots of equal contrast, inside a tile and across a tile's edge in x, in y and diagonally: strict < keeps neither;
  a higher dot in the neighbouring tile's halo, in x, in y and diagonally: only the higher one stays;
  a level-0 mask that removes one of two kept dots;
  widths 96 .. 99 and 197 .. 200: the border rule ends at every place of a group of four, also in a row's last group of two;
  two frames in one call; three levels."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from test_orb_gpu import _equal
from tod_amd import capi

pytestmark = pytest.mark.gpu

EDGE, THR, BG = 31, 20, 100
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
ALL = 4000     # n_features above any candidate count of these images


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def candidates(img, mask=None):
    """{(x, y)}: the positions fast_nms_kernel appends for a one-level call, stated on the whole image at once"""
    H, W = img.shape
    a = img.astype(np.int32)
    score = np.zeros((H, W), np.int32)
    ys, xs = slice(EDGE - 1, H - EDGE + 1), slice(EDGE - 1, W - EDGE + 1)            # the border rule: elsewhere the score is 0
    d = np.stack([a[ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx] for dx, dy in RING]) - a[ys, xs]
    best = np.zeros_like(d[0])
    for start in range(16):
        arc = d[[(start + k) % 16 for k in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(axis=0), (-arc).min(axis=0)))
    score[ys, xs] = np.where(best > THR, best, 0)
    out = set()
    for y in range(EDGE, H - EDGE):
        for x in range(EDGE, W - EDGE):
            s = score[y, x]
            if s == 0 or (mask is not None and mask[y, x] == 0):
                continue
            nb = score[y - 1:y + 2, x - 1:x + 2].copy()
            nb[1, 1] = -1
            if (nb < s).all():
                out.add((x, y))
    return out


def dots(H, W, *xyv):
    img = np.full((H, W), BG, np.uint8)
    for x, y, v in xyv:
        img[y, x] = v
    return img


@functools.lru_cache(maxsize=None)
def noise(H, W, seed=11):
    img = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (H, W), dtype=np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def textured(H, W, seed=0):
    rng = np.random.Generator(np.random.PCG64(2000 + seed))
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


def one_level(ctx, img, expect, mask=None):
    """one level, room for every candidate: the keypoints are the candidates. expect: their positions, or None for candidates() alone"""
    want = O.orb(img, ALL, 1, 1.2, mask=mask)
    cand = candidates(img, mask)
    assert set((int(x), int(y)) for x, y in want[0]) == cand and len(want[0]) == len(cand)
    if expect is not None:
        assert cand == set(expect)
    got = ctx.orb(img, ALL, 1, 1.2, mask=mask)
    _equal(got, want)
    assert set((int(x), int(y)) for x, y in got[0]) == cand


# tiles of a 200 x 80 image: x0 = 0, 64, 128; y0 = 16, 32, 48 hold keypoints (y = 31 .. 48)
H, W = 80, 200
TILE_PLACES = {
    "tile corner top left": (64, 32), "tile corner top right": (127, 32), "tile corner bottom left": (64, 47), "tile corner bottom right": (127, 47),
    "left edge column": (64, 40), "right edge column": (127, 40), "top edge row": (100, 32), "bottom edge row": (100, 47),
    "x = kEdge": (EDGE, 40), "x = w - kEdge - 1": (W - EDGE - 1, 40), "y = kEdge": (100, EDGE), "y = h - kEdge - 1": (100, H - EDGE - 1),
    "both borders": (EDGE, EDGE), "both far borders": (W - EDGE - 1, H - EDGE - 1),
}


@pytest.mark.parametrize("place", sorted(TILE_PLACES))
def test_a_single_corner(ctx, place):
    x, y = TILE_PLACES[place]
    one_level(ctx, dots(H, W, (x, y, 255)), [(x, y)])


@pytest.mark.parametrize("x,y", [(EDGE - 1, 40), (W - EDGE, 40), (100, EDGE - 1), (100, H - EDGE)])
def test_a_corner_one_pixel_outside_the_border_is_scored_and_not_kept(ctx, x, y):
    """and as the higher neighbour it removes the dot beside it that lies inside"""
    one_level(ctx, dots(H, W, (x, y, 255), (150, 45, 200)), [(150, 45)])
    inside = (min(max(x, EDGE), W - EDGE - 1), min(max(y, EDGE), H - EDGE - 1))
    one_level(ctx, dots(H, W, (x, y, 255), (inside[0], inside[1], 200), (150, 45, 200)), [(150, 45)])


@pytest.mark.parametrize("a,b", [((90, 40), (91, 40)), ((63, 40), (64, 40)), ((127, 36), (128, 36)), ((100, 47), (100, 48)),
                                 ((127, 47), (128, 48)), ((64, 47), (63, 48))])
def test_two_adjacent_equal_scores_keep_neither(ctx, a, b):
    one_level(ctx, dots(H, W, (a[0], a[1], 220), (b[0], b[1], 220), (150, 33, 180)), [(150, 33)])


@pytest.mark.parametrize("low,high", [((63, 40), (64, 40)), ((64, 40), (63, 40)), ((100, 47), (100, 48)), ((100, 32), (100, 31)),
                                      ((127, 47), (128, 48)), ((128, 32), (127, 31))])
def test_a_higher_score_in_the_neighbouring_tile(ctx, low, high):
    one_level(ctx, dots(H, W, (low[0], low[1], 200), (high[0], high[1], 255)), [high])


def test_the_mask_removes_a_kept_corner(ctx):
    img = dots(H, W, (64, 47, 255), (127, 32, 240), (90, 40, 230))
    mask = np.full((H, W), 255, np.uint8)
    mask[32, 127] = 0
    one_level(ctx, img, [(64, 47), (127, 32), (90, 40)])
    one_level(ctx, img, [(64, 47), (90, 40)], mask=mask)


def test_flat_image_has_an_empty_list(ctx):
    for shape in ((80, 96), (72, 200)):
        img = np.full(shape, BG, np.uint8)
        assert len(ctx.orb(img, 500, 3, 1.2)[0]) == len(O.orb(img, 500, 3, 1.2)[0]) == 0


@pytest.mark.parametrize("shape", [(80, 96), (72, 200)])
def test_noise_fills_the_list(ctx, shape):
    img = noise(*shape)
    one_level(ctx, img, None)
    n = len(candidates(img))
    assert n > 40
    # far fewer keypoints than candidates: the histogram's threshold picks them
    for nf, nl in ((n // 4, 1), (500, 3)):
        _equal(ctx.orb(img, nf, nl, 1.2), O.orb(img, nf, nl, 1.2))


@pytest.mark.parametrize("shape", [(80, 96), (80, 97), (76, 98), (72, 99), (72, 197), (75, 198), (80, 199), (72, 200)])
def test_widths_where_the_border_cuts_every_place_of_a_group(ctx, shape):
    img = textured(*shape)
    one_level(ctx, img, None)
    assert len(candidates(img)) > 0
    _equal(ctx.orb(img, 500, 3, 1.2), O.orb(img, 500, 3, 1.2))


def test_two_frames_in_one_call(ctx):
    import torch
    nf = 300
    imgs = [noise(H, W, seed=3), dots(H, W, (63, 40, 200), (64, 40, 255), (127, 47, 220), (128, 48, 220), (EDGE, EDGE, 255), (150, 33, 180))]
    wants = [O.orb(img, nf, 2, 1.2) for img in imgs]
    level0 = set((int(x), int(y)) for (x, y), a in zip(wants[1][0], wants[1][1]) if a[3] == 0)
    assert len(wants[0][0]) > 40 and level0 == {(64, 40), (EDGE, EDGE), (150, 33)}
    d = torch.from_numpy(np.stack(imgs)).cuda()
    out = [torch.zeros((2 * nf, w), dtype=torch.uint8, device="cuda") for w in (8, 16, 32)]
    n = ctx.orb_batch_device(d.data_ptr(), 2, H * W, H, W, W, nf, 2, 1.2, *[t.data_ptr() for t in out], nf)
    assert n == [len(w[0]) for w in wants]
    host = [t.cpu().numpy() for t in out]
    for f, want in enumerate(wants):
        kp, aux, desc = (np.ascontiguousarray(a[f * nf:f * nf + n[f]]) for a in host)
        _equal((kp.view(np.float32), aux.view(np.float32), desc), want)
