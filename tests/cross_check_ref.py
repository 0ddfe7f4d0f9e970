"""The cross-check filter (todhip_cross_check_device, include/todhip.h) in numpy, independent of the kernels: popcount table, per-frame
argmin by (distance, query index), order-preserving compaction. tests/test_cross_check_cpu.py holds it against a triple-loop statement;
the GPU tests hold the library against it, bit for bit, on the library's own unfiltered output."""
import numpy as np

POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint16)


def hamming(a, b):
    """u8[n, B] x u8[m, B] -> distances i64[n, m]"""
    return POP8[a[:, None, :] ^ b[None, :, :]].sum(axis=2, dtype=np.int64)


def valid_range(f, nq, Q, frame_nq=None):
    """[lo, hi): the valid query rows of frame f"""
    lo = f * Q
    rows = min(Q, nq - lo)
    return lo, lo + (rows if frame_nq is None else min(int(frame_nq[f]), rows))


def n_frames(nq, Q):
    return (nq + Q - 1) // Q


def cross_check(counts, matches, xyz, q_desc, db_desc, obj_off, Q, stride, frame_nq=None):
    """counts u32[nq], matches DMATCH[nq * stride], xyz f32[nq * stride, 3] (the fixed-stride layout), q_desc u8[nq, B], db_desc
    u8[N, B] (the full DB), obj_off u32[n_obj + 1]. Returns dict(counts, matches, xyz, keep, removed, total, tie_decided): the filtered
    image (slots behind the new counts are left as they were: the definition leaves [new, old) unspecified and never writes behind
    old), keep bool[nq * stride] per input slot, and how many live matches the index tie decided (the nearest distance to the row is
    reached by more than one valid query and the match's query is one of them)."""
    nq = len(counts)
    obj_off = np.asarray(obj_off, np.int64)
    m2 = matches.reshape(nq, stride)
    keep = np.zeros((nq, stride), bool)
    live = np.arange(stride)[None, :] < np.minimum(counts, stride)[:, None]
    g = obj_off[np.clip(m2["imgIdx"], 0, len(obj_off) - 2)] + m2["trainIdx"]
    tie_decided = 0
    for f in range(n_frames(nq, Q)):
        lo, hi = valid_range(f, nq, Q, frame_nq)
        if hi <= lo:
            continue
        rows = np.unique(g[lo:hi][live[lo:hi]])
        if len(rows) == 0:
            continue
        D = hamming(q_desc[lo:hi], db_desc[rows])                  # [valid queries, named rows]
        winner = lo + np.argmin(D, axis=0)                         # the first minimum: ties to the lower query index
        shared = (D == D.min(axis=0)[None, :]).sum(axis=0) > 1
        col = np.searchsorted(rows, g[lo:hi])
        col = np.clip(col, 0, len(rows) - 1)
        mine = winner[col] == np.arange(lo, hi)[:, None]
        keep[lo:hi] = live[lo:hi] & mine
        at_min = D[np.arange(hi - lo)[:, None], col] == D.min(axis=0)[col]
        tie_decided += int((live[lo:hi] & shared[col] & at_min).sum())
    out_counts = keep.sum(axis=1).astype(np.uint32)
    out_m, out_x = m2.copy(), xyz.reshape(nq, stride, 3).copy()
    for q in np.nonzero(live.sum(axis=1) != out_counts)[0]:
        idx = np.nonzero(keep[q])[0]
        out_m[q, :len(idx)] = m2[q, idx]
        out_x[q, :len(idx)] = xyz.reshape(nq, stride, 3)[q, idx]
    total = int(live.sum())
    return dict(counts=out_counts, matches=out_m.reshape(-1), xyz=out_x.reshape(-1, 3), keep=keep.reshape(-1),
                removed=total - int(keep.sum()), total=total, tie_decided=tie_decided)


def cross_check_loops(counts, matches, q_desc, db_desc, obj_off, Q, stride, frame_nq=None):
    """The definition word for word, in plain loops: keep flags per slot (list of lists)."""
    nq = len(counts)

    def dist(a, b):
        return sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a, b))
    keep = [[False] * stride for _ in range(nq)]
    for q in range(nq):
        f = q // Q
        lo, hi = valid_range(f, nq, Q, frame_nq)
        for j in range(min(int(counts[q]), stride)):
            m = matches[q * stride + j]
            row = db_desc[int(obj_off[m["imgIdx"]]) + int(m["trainIdx"])]
            if not lo <= q < hi:
                continue
            d = dist(q_desc[q], row)
            beaten = False
            for q2 in range(lo, hi):
                if (dist(q_desc[q2], row), q2) < (d, q):
                    beaten = True
            keep[q][j] = not beaten
    return keep


def csr(counts, matches, xyz, stride):
    """the fixed-stride image packed as todhip_match's CSR"""
    nq = len(counts)
    sel = (np.arange(stride)[None, :] < counts[:, None]).reshape(-1)
    row_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    return row_ptr, matches[sel], xyz.reshape(nq * stride, 3)[sel]
