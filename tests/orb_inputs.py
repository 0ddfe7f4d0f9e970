"""Seeded inputs that force the rarely taken paths of stage A (tests/test_orb_edges_gpu.py). TEST CODE ONLY, nothing of the GPU is
imported here. What each input is for is pinned on the CPU, with the restatement alone, by tests/test_orb_inputs_cpu.py: a change to
a generator cannot silently turn a GPU test into one that no longer reaches its path."""
import numpy as np

BACKGROUND = 100


def dot_lattice(H=480, W=640, seed=1):
    """One-pixel dots of 160 / 200 / 255 every 8 pixels on a flat background, the left half all 255. A dot's FAST score is its
    value minus the background, so a level has three huge classes of equal scores (60, 100, 155) and at most three Harris values;
    a dot inside the uniform half has a point-symmetric patch: both of its moments are zero."""
    ys, xs = np.arange(4, H, 8), np.arange(4, W, 8)
    rng = np.random.Generator(np.random.PCG64(seed))
    vals = rng.choice(np.array([160, 200, 255]), (len(ys), len(xs)))
    vals[:, :len(xs) // 2] = 255
    img = np.full((H, W), BACKGROUND, np.uint8)
    img[np.ix_(ys, xs)] = vals.astype(np.uint8)
    return img


def binary_blocks(seed=2):
    """480 x 640 of random black and white 8 x 8 blocks: scores up to 255, plateaus of equal scores that the strict non-maximum
    suppression removes entirely (level 0 yields nothing), and the largest Harris sums the stage sees."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return np.kron((rng.random((60, 80)) < 0.5) * 255, np.ones((8, 8))).astype(np.uint8)


def tiny(H, W):
    """Flat, with one bright pixel at (31, 31) where the image has one: the only admissible position of a 63 x 63 image."""
    img = np.full((H, W), BACKGROUND, np.uint8)
    if H > 31 and W > 31:
        img[31, 31] = 255
    return img


# (H, W) -> keypoints at n_features 10, one level
TINY_SHAPES = {(8, 8): 0, (62, 62): 0, (62, 200): 0, (63, 63): 1, (63, 64): 1}


def small_lattice():
    """100 x 100 with 16 dots in the admissible middle; with many levels or a large scale factor the upper pyramid levels
    round to 1 x 1 and 0 x 0 pixels."""
    img = np.full((100, 100), BACKGROUND, np.uint8)
    img[np.ix_(np.arange(34, 66, 8), np.arange(34, 66, 8))] = 255
    return img


# (n_levels, scale_factor) -> keypoints of small_lattice() at n_features 50
SMALL_LATTICE_CASES = {(9, 2.0): 16, (16, 1.5): 17}


def flat(H, W, value=90):
    return np.full((H, W), value, np.uint8)


def padded(img, stride, seed=7, tail=0):
    """The image at row pitch `stride` in a buffer of exactly (H - 1) * stride + W + tail bytes -- what a region of a larger image
    is: nothing is behind the last row's W pixels. The padding bytes are random, so any read of them changes a result.
    Returns (the flat buffer, its [H, W] view with strides (stride, 1))."""
    H, W = img.shape
    rng = np.random.Generator(np.random.PCG64(seed))
    buf = rng.integers(0, 256, (H - 1) * stride + W + tail, dtype=np.uint8)
    rows = np.lib.stride_tricks.as_strided(buf, (H, W), (stride, 1))
    rows[:] = img
    return buf, rows


def disc_moments(img, x, y):
    """(m10, m01) of the radius-15 disc around (x, y), as the restatement sums them"""
    hp = 15
    vmax, vmin = int(np.floor(hp * np.sqrt(2.0) / 2 + 1)), int(np.ceil(hp * np.sqrt(2.0) / 2))
    umax = [0] * (hp + 2)
    for v in range(vmax + 1):
        umax[v] = int(np.rint(np.sqrt(hp * hp - v * v)))
    v0 = 0
    for v in range(hp, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    m10 = m01 = 0
    for v in range(-hp, hp + 1):
        d = hp if v == 0 else umax[abs(v)]
        row = img[y + v, x - d:x + d + 1].astype(np.int64)
        m10 += int((np.arange(-d, d + 1) * row).sum())
        m01 += v * int(row.sum())
    return m10, m01
