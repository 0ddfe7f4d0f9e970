"""The small depth-rescale geometries shared by test_depth_rescale_cpu.py and test_depth_lookup_gpu.py, their sources and the
reference result of each (oracle_lib.train_rescale_depth, computed once per case)."""
import functools

import numpy as np

import oracle_lib as O

# (dH, dW, H, W), what it exercises
GEOMETRIES = [
    ((5, 7, 10, 14), "upscale"),
    ((3, 5, 9, 16), "factor 3.2"),
    ((20, 28, 10, 14), "exact 2x shrink"),
    ((21, 28, 10, 14), "bilinear shrink, not the fast path"),
    ((4, 8, 12, 16), "rows 8-11 are the NaN band"),
    ((9, 13, 9, 13), "equal size"),
]
REFUSED = (8, 4, 6, 8)                                        # the resized rows (16) do not fit into H
# every accepted geometry in both modes and both source types; nearest and bilinear are one code path only for equal sizes
CASES = [(g, u16, nearest) for g, _ in GEOMETRIES for u16 in (False, True) for nearest in (False, True)
         if not (nearest and g[:2] == g[2:])]


def case_id(case):
    (dH, dW, H, W), u16, nearest = case
    return "%dx%d-%dx%d-%s-%s" % (dH, dW, H, W, "u16" if u16 else "f32", "nearest" if nearest else "bilinear")


def source(dH, dW, u16):
    """A dH x dW depth image with holes: float metres with NaN, or uint16 millimetres with 0."""
    rng = np.random.Generator(np.random.PCG64(dH * 1000 + dW * 10 + (1 if u16 else 0)))
    holes = rng.random((dH, dW)) < 0.12
    holes[dH // 2, dW // 2] = True
    if u16:
        d = rng.integers(300, 4000, (dH, dW)).astype(np.uint16)
        d[holes] = 0
    else:
        d = rng.uniform(0.3, 4.0, (dH, dW)).astype(np.float32)
        d[holes] = np.nan
    return d


@functools.lru_cache(maxsize=None)
def reference(case):
    """(source, the reference's H x W result) of a case; the result is read-only."""
    (dH, dW, H, W), u16, nearest = case
    src = source(dH, dW, u16)
    want = O.train_rescale_depth(src, H, W, nearest)
    assert want is not None, "the reference refuses %s" % case_id(case)
    want.setflags(write=False)
    src.setflags(write=False)
    return src, want


def same_bits(a, b):
    """float32 arrays equal bit for bit where both are numbers, NaN in the same places (a NaN's payload is not part of the result)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))
