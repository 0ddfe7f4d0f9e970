"""The definition of todhip_match_radius (include/todhip.h) in numpy: xor, popcount table, lexsort, cut. The checker of the GPU
tests where the oracle's k = n_rows insertion lists would take minutes; tests/test_match_radius_cpu.py pins it to the oracle."""
import numpy as np

POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.uint16)
DMATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])


def distances(db, q):
    """u16[nq, n]: Hamming distances of 32-byte rows"""
    out = np.zeros((len(q), len(db)), np.uint16)
    for i, row in enumerate(np.asarray(q, np.uint8)):
        out[i] = POPCOUNT[np.bitwise_xor(np.asarray(db, np.uint8), row[None, :])].sum(axis=1)
    return out


def match_radius(db, obj_off, pts, q, radius, max_per_query, rows=None):
    """(row_ptr, matches, xyz, in_radius). rows: the searched rows (ascending indices into db; default all) -- a shard or a selection;
    trainIdx / imgIdx / xyz always refer to the full DB."""
    obj_off = np.asarray(obj_off, np.int64)
    rows = np.arange(len(db)) if rows is None else np.asarray(rows, np.int64)
    d = distances(np.asarray(db)[rows], q) if len(rows) else np.zeros((len(q), 0), np.uint16)
    row_ptr, in_radius, ms = [0], [], []
    for qi in range(len(q)):
        inside = np.flatnonzero(d[qi] <= radius)                       # radius >= 256: every row
        order = inside[np.lexsort((rows[inside], d[qi][inside]))][:max_per_query]     # distance, then global row
        g = rows[order]
        m = np.zeros(len(g), DMATCH_DTYPE)
        m["queryIdx"], m["distance"] = qi, d[qi][order]
        m["imgIdx"] = np.searchsorted(obj_off, g, side="right") - 1
        m["trainIdx"] = g - obj_off[m["imgIdx"]]
        ms.append((m, np.asarray(pts, np.float32)[g].reshape(-1, 3)))
        in_radius.append(len(inside))
        row_ptr.append(row_ptr[-1] + len(g))
    return (np.asarray(row_ptr, np.uint32), np.concatenate([m for m, _ in ms]), np.concatenate([x for _, x in ms]),
            np.asarray(in_radius, np.uint32))
