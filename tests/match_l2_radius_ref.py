"""The definition of todhip_match_l2_radius (include/todhip.h) in numpy. d2 is accumulated dimension by dimension over whole arrays
in binary32 -- one subtraction, one product, one addition per step, so the order is the defining one and nothing is fused -- then a
stable sort on (d2 bits, row), the cut and the counts. The checker of the GPU tests where the oracle's k = n_rows insertion lists
would be slow; tests/test_match_l2_radius_cpu.py pins it to the oracle."""
import numpy as np

DMATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])


def d2(db, q):
    """f32[nq, n]: the defining squared distances"""
    dbT, q = np.ascontiguousarray(np.asarray(db, np.float32).T), np.ascontiguousarray(q, np.float32)
    acc = np.zeros((len(q), dbT.shape[1]), np.float32)
    with np.errstate(over="ignore"):
        for q0 in range(0, len(q), 16):                                 # 16 queries at a time: the three arrays stay in the cache
            a = acc[q0:q0 + 16]
            t = np.empty_like(a)
            for i in range(dbT.shape[0]):                               # acc = acc + (q[i] - r[i]) * (q[i] - r[i]), one rounding each
                np.subtract(q[q0:q0 + 16, i, None], dbT[i][None, :], out=t)
                np.multiply(t, t, out=t)
                np.add(a, t, out=a)
    return acc


def match_l2_radius(db, obj_off, pts, q, radius, max_per_query, dd=None):
    """(row_ptr, matches, xyz, in_radius). dd: d2(db, q), when the caller has it already"""
    obj_off = np.asarray(obj_off, np.int64)
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    radius = np.float32(radius)
    row_ptr, in_radius, ms, xs = [0], [], [], []
    dd_all = d2(db, q) if dd is None else dd
    for q0 in range(0, len(q), 64):
        dd = dd_all[q0:q0 + 64]
        dist = np.sqrt(dd)                                              # correctly rounded, as sqrtf
        for i in range(len(dd)):
            inside = np.flatnonzero(~(dist[i] > radius))
            key = (dd[i][inside].view(np.uint32).astype(np.uint64) << np.uint64(32)) | inside.astype(np.uint64)
            g = inside[np.argsort(key, kind="stable")][:max_per_query]
            m = np.zeros(len(g), DMATCH_DTYPE)
            m["queryIdx"], m["distance"] = q0 + i, dist[i][g]
            m["imgIdx"] = np.searchsorted(obj_off, g, side="right") - 1
            m["trainIdx"] = g - obj_off[m["imgIdx"]]
            ms.append(m)
            xs.append(pts[g])
            in_radius.append(len(inside))
            row_ptr.append(row_ptr[-1] + len(g))
    return np.asarray(row_ptr, np.uint32), np.concatenate(ms), np.concatenate(xs), np.asarray(in_radius, np.uint32)
