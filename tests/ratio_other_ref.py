"""Lowe's ratio test against another object (todhip_other_object_min_device, todhip_ratio_other_apply_device,
todhip_ratio_other_device; include/todhip.h) in numpy, independent of the kernels and of tod_amd/csrc/ratio_other.h: complete distance
tables from a popcount table at any width, other(q, o) as a masked minimum over them, the limit by brute force over binary32 products,
and the filter. tests/test_ratio_other_cpu.py pins it on the oracle's sorted keys; the GPU tests hold the library against it bit for bit."""
import numpy as np

NONE = 0xFFFFFFFF
POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint16)


def hamming(a, b, chunk=64):
    """u8[n, B] x u8[m, B] -> the complete table of distances i64[n, m]"""
    a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
    out = np.zeros((len(a), len(b)), np.int64)
    for lo in range(0, len(a), chunk):
        out[lo:lo + chunk] = POP8[a[lo:lo + chunk, None, :] ^ b[None, :, :]].sum(axis=2, dtype=np.int64)
    return out


def row_objects(off):
    """the object of every row of the full DB"""
    off = np.asarray(off, np.int64)
    return np.searchsorted(off, np.arange(off[-1]), side="right") - 1


def searched_mask(off, shard=None, selection=None):
    """bool[N]: the rows a context searches -- its shard (first row, rows; None: the whole DB) under its selection (object ids; None:
    all objects)"""
    obj = row_objects(off)
    mask = np.ones(len(obj), bool)
    if shard is not None:
        rows = np.arange(len(obj))
        mask &= (rows >= shard[0]) & (rows < shard[0] + shard[1])
    if selection is not None:
        mask &= np.isin(obj, np.asarray(list(selection), np.int64))
    return mask


def other(D, off, excl, searched=None):
    """other(q, excl[q]) u32[nq]: the least D[q, r] over the searched rows r outside object excl[q] (NONE, or an index that is no
    object: nothing is excluded); NONE where there is no such row"""
    obj = row_objects(off)
    searched = np.ones(len(obj), bool) if searched is None else searched
    excl = np.asarray(excl, np.int64)
    allowed = searched[None, :] & (obj[None, :] != excl[:, None])
    big = np.int64(NONE)
    return np.where(allowed, D, big).min(axis=1, initial=big).astype(np.uint32)


def other_min(D, off, excl, limit=None, cap=NONE, searched=None):
    """the primitive: min(other, limit, cap) as unsigned integers"""
    out = np.minimum(other(D, off, excl, searched).astype(np.int64), np.int64(cap))
    if limit is not None:
        out = np.minimum(out, np.asarray(limit, np.int64))
    return out.astype(np.uint32)


def passes(d1, ratio, other_d):
    """(float)d1 < ratio * (float)other in binary32, elementwise"""
    rhs = np.float32(ratio) * np.asarray(other_d).astype(np.float32)          # one binary32 product
    assert rhs.dtype == np.float32
    return np.asarray(d1).astype(np.float32) < rhs


def survives(d1, ratio, other_d):
    return (np.asarray(other_d, np.int64) == NONE) | passes(d1, ratio, other_d)


def limit(d1, ratio, search_to=4096):
    """the least integer L with passes(d1, ratio, L), elementwise, by trying them all in order (ratios of at least d1 / search_to)"""
    tries = np.arange(search_to, dtype=np.int64)
    ok = passes(np.asarray(d1, np.int64).reshape(-1, 1), ratio, tries[None, :])
    assert ok.any(axis=1).all()
    return ok.argmax(axis=1).astype(np.uint32).reshape(np.shape(d1))


def limits_of(counts, matches, stride, ratio):
    """(excl u32[nq], limit u32[nq]) the filter hands to the primitive: slot 0's object and limit; no kept match: NONE and 0"""
    nq = len(counts)
    m0 = matches.reshape(nq, stride)[:, 0]
    live = counts > 0
    d1 = np.where(live, m0["distance"], 0).astype(np.int64)
    return (np.where(live, m0["imgIdx"].astype(np.int64), NONE).astype(np.uint32),
            np.where(live, limit(d1, ratio), 0).astype(np.uint32))


def apply(counts, matches, stride, ratio, other_d):
    """the predicate on a fixed-stride output: the new counts (a failing query: 0; nothing else changes)"""
    nq = len(counts)
    d1 = matches.reshape(nq, stride)[:, 0]["distance"].astype(np.int64)
    keep = (counts == 0) | survives(np.where(counts > 0, d1, 0), ratio, other_d)
    return np.where(keep, counts, 0).astype(np.uint32)


def ratio_other(counts, matches, stride, ratio, D, off, searched=None):
    """the whole filter from the exact other(q, o1): dict(counts, other, dropped, kept)"""
    excl, _ = limits_of(counts, matches, stride, ratio)
    o = other(D, off, excl, searched)
    new = apply(counts, matches, stride, ratio, o)
    live = counts > 0
    return dict(counts=new, other=o, dropped=int((live & (new == 0)).sum()), kept=int((new > 0).sum()))


def classic_ratio_keeps(D, ratio, searched=None):
    """bool[nq]: does todhip_set_ratio_test keep the query -- d1 < ratio * d2 over its two nearest searched rows (one row: kept)"""
    Dm = D if searched is None else D[:, searched]
    if Dm.shape[1] < 2:
        return np.ones(len(D), bool)
    two = np.partition(Dm, 1, axis=1)[:, :2]
    return passes(two[:, 0], ratio, two[:, 1])
