"""The two filters of the float matcher (todhip_set_l2_ratio_test, todhip_cross_check_l2_device; include/todhip.h) in numpy,
independent of the kernels. Both work on match_l2_radius_ref.d2, the defining squared distances. tests/test_l2_filters_cpu.py holds
each against a plain-loop statement; the GPU tests hold the library against them bit for bit."""
import numpy as np

import cross_check_ref as R
from match_l2_radius_ref import DMATCH_DTYPE, d2


def keys_of(dd_row):
    """u64[n]: (binary32 bits of d2) << 32 | row, the library's order"""
    return (dd_row.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(len(dd_row), dtype=np.uint64)


def ratio_passes(dd, ratio):
    """bool[nq]: does a query keep its matches? dd f32[nq, n] = d2(db, q). The two nearest rows in the order (d2, row); dist = sqrt in
    binary32; dist1 < ratio * dist2, one binary32 product. A one-row DB passes."""
    nq, n = dd.shape
    if n < 2:
        return np.ones(nq, bool)
    out = np.zeros(nq, bool)
    r = np.float32(ratio)
    for i in range(nq):
        two = np.sort(keys_of(dd[i]))[:2]
        d = np.sqrt((two >> np.uint64(32)).astype(np.uint32).view(np.float32))
        out[i] = d[0] < np.float32(r * d[1])
    return out


def ratio_filter(dd, k, radius, ratio, obj_off=None, pts=None, sentinel=None):
    """What todhip_match_l2_device leaves at stride k with the ratio test at `ratio` (0 = off): (counts u32[nq], matches DMATCH[nq * k],
    xyz f32[nq * k, 3] or None without pts). Slots behind counts hold zeros, or `sentinel` bytes."""
    nq, n = dd.shape
    radius = np.float32(radius)
    keep = ratio_passes(dd, ratio) if ratio else np.ones(nq, bool)
    counts = np.zeros(nq, np.uint32)
    fill = 0 if sentinel is None else sentinel
    m = np.frombuffer(bytes([fill]) * (nq * k * 16), DMATCH_DTYPE).copy()
    xyz = None if pts is None else np.frombuffer(bytes([fill]) * (nq * k * 12), np.float32).copy().reshape(-1, 3)
    off = np.array([0, n], np.int64) if obj_off is None else np.asarray(obj_off, np.int64)
    for i in range(nq):
        if not keep[i]:
            continue
        order = np.argsort(keys_of(dd[i]), kind="stable")[:k]
        dist = np.sqrt(dd[i][order])
        cut = np.flatnonzero(dist > radius)
        order = order[:cut[0]] if len(cut) else order
        counts[i] = len(order)
        s = slice(i * k, i * k + len(order))
        obj = np.searchsorted(off, order, side="right") - 1
        m["queryIdx"][s], m["trainIdx"][s], m["imgIdx"][s], m["distance"][s] = i, order - off[obj], obj, np.sqrt(dd[i][order])
        if xyz is not None:
            xyz[s] = np.asarray(pts, np.float32).reshape(-1, 3)[order]
    return counts, m, xyz


def ratio_passes_loops(db, q, ratio):
    """The definition word for word: scalar binary32 arithmetic in plain loops."""
    f = np.float32
    out = []
    for qi in range(len(q)):
        best = []                                                   # the two smallest (d2 bits, row)
        for r in range(len(db)):
            acc = f(0)
            for i in range(db.shape[1]):
                t = f(f(q[qi][i]) - f(db[r][i]))
                acc = f(acc + f(t * t))
            best = sorted(best + [(int(np.array(acc, f).view(np.uint32)), r)])[:2]
        if len(best) < 2:
            out.append(True)
            continue
        d1, d2_ = (np.sqrt(np.array(b[0], np.uint32).view(f)) for b in best)
        out.append(bool(f(d1) < f(f(ratio) * f(d2_))))
    return out


def d2_bits(db, q):
    """u32[nq, n]: d(q, g) of the float cross-check"""
    return np.ascontiguousarray(d2(db, q)).view(np.uint32)


def cross_check_l2(counts, matches, xyz, q_desc, db_desc, obj_off, Q, stride, frame_nq=None, dist=None):
    """cross_check_ref.cross_check with D = d2(...).view(uint32): the same frames, winners, ties and compaction; only the distance
    differs. dist: a replacement for d2_bits(db, q) -> [nq, n] (the order test hands in other summation orders). Returns
    cross_check_ref.cross_check's dict."""
    nq = len(counts)
    obj_off = np.asarray(obj_off, np.int64)
    m2 = matches.reshape(nq, stride)
    keep = np.zeros((nq, stride), bool)
    live = np.arange(stride)[None, :] < np.minimum(counts, stride)[:, None]
    g = obj_off[np.clip(m2["imgIdx"], 0, len(obj_off) - 2)] + m2["trainIdx"]
    tie_decided = 0
    for f in range(R.n_frames(nq, Q)):
        lo, hi = R.valid_range(f, nq, Q, frame_nq)
        if hi <= lo:
            continue
        rows = np.unique(g[lo:hi][live[lo:hi]])
        if len(rows) == 0:
            continue
        D = (d2_bits(db_desc[rows], q_desc[lo:hi]) if dist is None else dist(db_desc[rows], q_desc[lo:hi])).astype(np.int64)
        winner = lo + np.argmin(D, axis=0)                         # the first minimum: ties to the lower query index
        shared = (D == D.min(axis=0)[None, :]).sum(axis=0) > 1
        col = np.clip(np.searchsorted(rows, g[lo:hi]), 0, len(rows) - 1)
        mine = winner[col] == np.arange(lo, hi)[:, None]
        keep[lo:hi] = live[lo:hi] & mine
        at_min = D[np.arange(hi - lo)[:, None], col] == D.min(axis=0)[col]
        tie_decided += int((live[lo:hi] & shared[col] & at_min).sum())
    out_counts = keep.sum(axis=1).astype(np.uint32)
    x3 = xyz.reshape(nq, stride, 3)
    out_m, out_x = m2.copy(), x3.copy()
    for qi in np.nonzero(live.sum(axis=1) != out_counts)[0]:
        idx = np.nonzero(keep[qi])[0]
        out_m[qi, :len(idx)] = m2[qi, idx]
        out_x[qi, :len(idx)] = x3[qi, idx]
    total = int(live.sum())
    return dict(counts=out_counts, matches=out_m.reshape(-1), xyz=out_x.reshape(-1, 3), keep=keep.reshape(-1),
                removed=total - int(keep.sum()), total=total, tie_decided=tie_decided)


def cross_check_l2_loops(counts, matches, q_desc, db_desc, obj_off, Q, stride, frame_nq=None):
    """The definition word for word, in plain loops over scalar binary32 arithmetic: keep flags per slot (list of lists)."""
    f = np.float32
    nq = len(counts)

    def dist(a, b):
        acc = f(0)
        for x, y in zip(a, b):
            t = f(f(x) - f(y))
            acc = f(acc + f(t * t))
        return int(np.array(acc, f).view(np.uint32))
    keep = [[False] * stride for _ in range(nq)]
    for q in range(nq):
        lo, hi = R.valid_range(q // Q, nq, Q, frame_nq)
        if not lo <= q < hi:
            continue
        for j in range(min(int(counts[q]), stride)):
            m = matches[q * stride + j]
            row = db_desc[int(obj_off[m["imgIdx"]]) + int(m["trainIdx"])]
            d = dist(q_desc[q], row)
            keep[q][j] = not any((dist(q_desc[q2], row), q2) < (d, q) for q2 in range(lo, hi))
    return keep
