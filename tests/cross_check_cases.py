"""Inputs of the cross-check tests, shared by tests/test_cross_check_cpu.py (which pins them on the numpy reference alone) and
tests/test_cross_check_gpu.py: a small clustered DB at either binary width, planted query frames, and the brute-force search that
states what the library's unfiltered output is."""
import numpy as np

import cross_check_ref as R
from tod_amd import capi

OBJ_ROWS = (1, 31, 33, 257, 700)
N_ROWS = sum(OBJ_ROWS)                       # 1022
DENSE = 120                                  # rows of the one dense cluster: more than 64 of them inside any sensible radius
RADIUS = 40
WIDTHS = (32, 64)
SINGLE_FRAMES = (1, 2, 33, 64, 65, 70)       # Q with nq = Q
KS = (1, 2, 5, 8)
FRAMES3 = dict(Q=33, nq=99, frame_nq=[33, 0, 7])
SENTINEL = 0x5A


def flipped(row, rng, n):
    out = row.copy()
    for b in rng.choice(8 * len(row), n, replace=False):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


_db = {}


def make_db(width):
    """dict(desc u8[N_ROWS, width], pts f32[N_ROWS, 3], off u32[6], centres: row index of each cluster's first member, dense: the
    rows of the dense cluster). Clusters of 6 variants (0-12 flipped bits) of a random centre, one cluster of DENSE variants (0-10
    flipped bits), shuffled over the objects."""
    if width in _db:
        return _db[width]
    rng = np.random.Generator(np.random.PCG64(1000 + width))
    rows, cluster = [], []
    centre = rng.integers(0, 256, width, dtype=np.uint8)
    for i in range(DENSE):
        rows.append(flipped(centre, rng, int(rng.integers(0, 11))))
        cluster.append(0)
    c = 1
    while len(rows) < N_ROWS:
        centre = rng.integers(0, 256, width, dtype=np.uint8)
        for i in range(min(6, N_ROWS - len(rows))):
            rows.append(flipped(centre, rng, 0 if i == 0 else int(rng.integers(1, 13))))
            cluster.append(c)
        c += 1
    perm = rng.permutation(N_ROWS)
    desc = np.stack(rows)[perm]
    cluster = np.asarray(cluster)[perm]
    first = {}
    for r, cl in enumerate(cluster):
        first.setdefault(int(cl), r)
    _db[width] = dict(desc=np.ascontiguousarray(desc), pts=rng.standard_normal((N_ROWS, 3)).astype(np.float32),
                      off=np.concatenate([[0], np.cumsum(OBJ_ROWS)]).astype(np.uint32),
                      centres=[first[cl] for cl in range(1, c)], dense=np.nonzero(cluster == 0)[0])
    return _db[width]


def make_queries(width, n, seed=0):
    """n query rows, planted in triples on one DB row each: member 0 with 3 flipped bits, member 1 with 9 (the same row at a larger
    distance: beaten), member 2 with 3 other flipped bits (the same row at the SAME distance: beaten by the index tie). Every fifth
    triple sits on a row of the dense cluster (at 1, 6 and 1 flipped bits). From 33 queries on, the last query is byte-identical to
    query 0."""
    db = make_db(width)
    rng = np.random.Generator(np.random.PCG64(7000 + 100 * width + n + 10007 * seed))
    q = np.zeros((n, width), np.uint8)
    for t in range((n + 2) // 3):
        dense = t % 5 == 4
        row = db["desc"][db["dense"][t % DENSE] if dense else db["centres"][(7 * t + seed) % len(db["centres"])]]
        bits = rng.choice(8 * width, 12, replace=False)
        for i, (lo, cnt) in enumerate(((0, 1), (1, 6), (7, 1)) if dense else ((0, 3), (3, 9), (0, 0))):
            if 3 * t + i >= n:
                break
            use = bits[lo:lo + cnt] if cnt else rng.choice(np.setdiff1d(np.arange(8 * width), bits[:3]), 3, replace=False)
            v = row.copy()
            for b in use:
                v[b >> 3] ^= np.uint8(1 << (b & 7))
            q[3 * t + i] = v
    if n >= 33:
        q[n - 1] = q[0]
    return q


def make_frames3(width):
    """FRAMES3's 99 queries: frame 0 planted; frame 1 planted (frame_nq 0: none of it competes); frame 2 = frame 0's first 7 queries
    again (the same descriptors in two frames), then -- behind frame_nq[2] = 7 -- exact copies of the rows frame 2's queries sit on,
    which would take every one of those rows if they competed."""
    db = make_db(width)
    q0, q1 = make_queries(width, 33, 0), make_queries(width, 33, 1)
    q2 = make_queries(width, 33, 2)
    q2[:7] = q0[:7]
    D = R.hamming(q0[:7], db["desc"])
    q2[7:14] = db["desc"][np.argmin(D, axis=1)]
    return np.ascontiguousarray(np.concatenate([q0, q1, q2]))


def search_ref(db, q, stride, radius):
    """What todhip_match_device (stride = k) and todhip_match_radius_device (stride = max_per_query) leave: per query the first
    `stride` rows within `radius` in the order (distance, row). Slots behind counts hold SENTINEL bytes."""
    nq = len(q)
    D = R.hamming(q, db["desc"])
    counts = np.zeros(nq, np.uint32)
    m = np.frombuffer(bytes([SENTINEL]) * (nq * stride * 16), capi.DMATCH_DTYPE).copy()
    xyz = np.frombuffer(bytes([SENTINEL]) * (nq * stride * 12), np.float32).copy().reshape(-1, 3)
    off = db["off"].astype(np.int64)
    for i in range(nq):
        order = np.lexsort((np.arange(N_ROWS), D[i]))
        order = order[D[i][order] <= radius][:stride]
        counts[i] = len(order)
        obj = np.searchsorted(off, order, side="right") - 1
        s = slice(i * stride, i * stride + len(order))
        m["queryIdx"][s], m["trainIdx"][s], m["imgIdx"][s], m["distance"][s] = i, order - off[obj], obj, D[i][order]
        xyz[s] = db["pts"][order]
    return counts, m, xyz
