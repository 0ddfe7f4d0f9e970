"""Stage A at the seams of its tiles. fast_nms_kernel scores 64 x 16 pixel tiles from an LDS copy of their pixels in two passes (a
compass test over every position, the exact score over the compacted survivors) and blur_kernel filters 128 x 64 pixel tiles through
LDS, four pixels to a lane: what can go wrong is a halo, a row that ends inside a group of four pixels, a row pitch that is no
multiple of four, a survivor list that overflows, and a neighbouring frame read across a slice's end. Every comparison is against the
CPU restatement: counts, positions, size / response / octave and descriptors bit for bit; the reported angle within 4.9e-4 degrees,
the contract of every ORB comparison here (tests/test_orb_gpu.py: _equal -- it is atan2f of two libraries, of moments that are
themselves compared through the descriptors, which are steered by them).

The sweeps: image sizes around 224 = 3.5 FAST tiles and 160 = 10 FAST tile rows (every residue of the width mod 4), and, because
the blur's tile is 128 x 64, also around 256 = 2 blur tiles (4 FAST tiles) and 192 = 3 blur tile rows."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import orb_inputs as I
from test_orb_gpu import _equal
from tod_amd import capi, synth

pytestmark = pytest.mark.gpu

NF, NL, SF = 600, 2, 1.2
SEAM_SHAPES = sorted({(160, W) for W in range(221, 229)} | {(H, 225) for H in range(157, 165)} |
                     {(160, W) for W in range(253, 261)} | {(H, 225) for H in range(189, 197)})


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def base_image():
    img = synth.make_image(3)
    img.setflags(write=False)
    return img


def crop(H, W, y=100, x=200):
    return np.ascontiguousarray(base_image()[y:y + H, x:x + W])


def same_as_restatement(ctx, img, at_least):
    want = O.orb(img, NF, NL, SF)
    assert len(want[0]) >= at_least
    got = ctx.orb(img, NF, NL, SF)
    _equal(got, want)
    return got


@pytest.mark.parametrize("H,W", SEAM_SHAPES)
def test_seam_sweep(ctx, H, W):
    """194-320 keypoints per case in the restatement; at level 0 some lie within a pixel of a 64-column and of a 16-row seam"""
    same_as_restatement(ctx, crop(H, W), 150)


def test_noise_fills_the_survivor_list(ctx):
    """uniform noise: 85 % of the positions pass the compass test, so pass 2 runs several rounds over a nearly full list"""
    rng = np.random.Generator(np.random.PCG64(5))
    same_as_restatement(ctx, rng.integers(0, 256, (160, 225), dtype=np.uint8), 150)


def test_binary_blocks(ctx):
    """scores up to 255 and plateaus that the strict suppression removes across tile seams"""
    same_as_restatement(ctx, I.binary_blocks(), 150)


def test_dot_lattice(ctx):
    """isolated dots: one survivor every 8 pixels, equal scores on both sides of every seam"""
    same_as_restatement(ctx, I.dot_lattice(160, 225), 150)


def test_batch_with_distinct_neighbours(ctx):
    """five crops at five offsets in one batch: every frame equals its single call, so nothing was read across a slice's end"""
    import torch
    H, W = 160, 225
    offsets = [(100, 200), (37, 11), (300, 400), (5, 333), (250, 90)]
    imgs = [crop(H, W, y, x) for y, x in offsets]
    F = len(imgs)
    d = torch.from_numpy(np.stack(imgs)).cuda()
    kp = torch.zeros((F, NF, 2), device="cuda"); aux = torch.zeros((F, NF, 4), device="cuda")
    desc = torch.zeros((F, NF, 32), dtype=torch.uint8, device="cuda")
    n = ctx.orb_batch_device(d.data_ptr(), F, H * W, H, W, W, NF, NL, SF, kp.data_ptr(), aux.data_ptr(), desc.data_ptr(), NF)
    kp, aux, desc = kp.cpu().numpy(), aux.cpu().numpy(), desc.cpu().numpy()
    for f in range(F):
        single = same_as_restatement(ctx, imgs[f], 150)
        assert n[f] == len(single[0])
        for a, b in zip((kp[f], aux[f], desc[f]), single):
            assert np.array_equal(a[:n[f]], b)                          # the same device code: the angle too
