"""Inputs of the float filters' tests, shared by tests/test_l2_filters_cpu.py (which pins them on the numpy reference alone) and
tests/test_l2_filters_gpu.py: cross_check_cases' clustered DB transposed to floats, planted query frames, a frame on which the
defining summation order decides, the early-exit trap, and the planted rows of the ratio test. Descriptors are integer-valued
except where said, so that a distance can be put exactly where a test wants it."""
import numpy as np

import l2_filters_ref as F
from match_l2_radius_ref import d2

OBJ_ROWS = (1, 31, 33, 257, 700)
N_ROWS = sum(OBJ_ROWS)                       # 1022
DENSE = 120                                  # rows of the one dense cluster: all of them inside RADIUS of each other
RADIUS = 40.0
SINGLE_FRAMES = (1, 2, 33, 64, 65, 70)       # Q with nq = Q
KS = (1, 2, 5, 8)
FRAMES3 = dict(Q=33, nq=99, frame_nq=[33, 0, 7])
SENTINEL = 0x5A

_db = {}


def _variant(centre, rng, n_dims):
    out = centre.copy()
    dims = rng.choice(128, n_dims, replace=False)
    out[dims] += rng.choice([-3, -2, -1, 1, 2, 3], n_dims).astype(np.float32)
    return out


def make_db():
    """dict(desc f32[N_ROWS, 128], pts f32[N_ROWS, 3], off u32[6], centres: row index of each cluster's first member, dense: the rows
    of the dense cluster). Components 20 ... 230; clusters of 6 variants of a random centre (+-1 ... 3 in 0 - 12 dimensions), one
    cluster of DENSE variants (0 - 10 dimensions), shuffled over the objects."""
    if _db:
        return _db
    rng = np.random.Generator(np.random.PCG64(1512))
    rows, cluster = [], []
    centre = rng.integers(23, 228, 128).astype(np.float32)
    for i in range(DENSE):
        rows.append(_variant(centre, rng, int(rng.integers(0, 11))))
        cluster.append(0)
    c = 1
    while len(rows) < N_ROWS:
        centre = rng.integers(23, 228, 128).astype(np.float32)
        for i in range(min(6, N_ROWS - len(rows))):
            rows.append(_variant(centre, rng, 0 if i == 0 else int(rng.integers(1, 13))))
            cluster.append(c)
        c += 1
    perm = rng.permutation(N_ROWS)
    desc = np.stack(rows)[perm]
    cluster = np.asarray(cluster)[perm]
    first = {}
    for r, cl in enumerate(cluster):
        first.setdefault(int(cl), r)
    _db.update(desc=np.ascontiguousarray(desc), pts=rng.standard_normal((N_ROWS, 3)).astype(np.float32),
               off=np.concatenate([[0], np.cumsum(OBJ_ROWS)]).astype(np.uint32),
               centres=[first[cl] for cl in range(1, c)], dense=np.nonzero(cluster == 0)[0])
    return _db


def make_queries(n, seed=0):
    """n query rows, planted in triples on one DB row each: member 0 = row + 2 in 3 dimensions, member 1 = row + 2 in 9 dimensions
    (the same row at a larger distance: beaten), member 2 = row + 2 in 3 OTHER dimensions (the same d2 = 12: beaten by the index
    tie). Every fifth triple sits on a row of the dense cluster. From 33 queries on, the last query is byte-identical to query 0."""
    db = make_db()
    rng = np.random.Generator(np.random.PCG64(7000 + n + 10007 * seed))
    q = np.zeros((n, 128), np.float32)
    for t in range((n + 2) // 3):
        dense = t % 5 == 4
        row = db["desc"][db["dense"][t % DENSE] if dense else db["centres"][(7 * t + seed) % len(db["centres"])]]
        dims = rng.choice(128, 15, replace=False)
        for i, use in enumerate((dims[:3], dims[3:12], dims[12:15])):
            if 3 * t + i >= n:
                break
            v = row.copy()
            v[use] += 2
            q[3 * t + i] = v
    if n >= 33:
        q[n - 1] = q[0]
    return q


def make_frames3():
    """FRAMES3's 99 queries, as cross_check_cases.make_frames3 builds them: frame 0 planted; frame 1 planted (frame_nq 0: none of it
    competes); frame 2 = frame 0's first 7 queries again, then -- behind frame_nq[2] = 7, rows 73 - 79 -- exact copies of the DB rows
    frame 2's queries sit on, which would take every one of those rows if they competed."""
    db = make_db()
    q0, q1, q2 = make_queries(33, 0), make_queries(33, 1), make_queries(33, 2)
    q2[:7] = q0[:7]
    q2[7:14] = db["desc"][np.argmin(d2(db["desc"], q0[:7]), axis=1)]
    return np.ascontiguousarray(np.concatenate([q0, q1, q2]))


def make_frames70():
    """70 frames of Q = 2 (more frames than travel as a kernel argument): both queries of a frame sit on one row at the same d2 = 12,
    so the second loses every shared row by the index tie while it competes. frame_nq = [2] * 35 + [1] * 35."""
    db = make_db()
    rng = np.random.Generator(np.random.PCG64(70))
    q = np.zeros((140, 128), np.float32)
    for f in range(70):
        row = db["desc"][db["centres"][(3 * f) % len(db["centres"])]]
        dims = rng.choice(128, 6, replace=False)
        q[2 * f], q[2 * f + 1] = row, row
        q[2 * f, dims[:3]] += 2
        q[2 * f + 1, dims[3:]] += 2
    return q, np.array([2] * 35 + [1] * 35, np.uint32)


def search_ref(db, q, stride, radius, dd=None):
    """What todhip_match_l2_device (stride = k) and todhip_match_l2_radius_device (stride = max_per_query) leave: per query the first
    `stride` rows within `radius` in the order (d2, row). Slots behind counts hold SENTINEL bytes."""
    return F.ratio_filter(d2(db["desc"], q) if dd is None else dd, stride, radius, 0.0, db["off"], db["pts"], SENTINEL)


def order_frame(seed=99):
    """(db dict, q f32[80, 128]): 40 rows g = 50 N(0, 1) as one object; queries in pairs g + e and g + permuted(e), e = 3 N(0, 1). The
    real distances of a pair to its row are equal, the binary32 sums are not: who keeps the row depends on the order of the sum."""
    rng = np.random.Generator(np.random.PCG64(seed))
    g = (50 * rng.standard_normal((40, 128))).astype(np.float32)
    q = np.zeros((80, 128), np.float32)
    for r in range(40):
        e = (3 * rng.standard_normal(128)).astype(np.float32)
        q[2 * r] = g[r] + e
        q[2 * r + 1] = g[r] + rng.permutation(e)
    db = dict(desc=g, pts=rng.standard_normal((40, 3)).astype(np.float32), off=np.array([0, 40], np.uint32))
    return db, q


def pairwise_bits(db, q):
    """numpy's own (pairwise) binary32 sum of the squares, as bits [nq, n]"""
    t = (q[:, None, :] - db[None, :, :]).astype(np.float32)
    return np.ascontiguousarray((t * t).sum(axis=2, dtype=np.float32)).view(np.uint32)


def float64_bits(db, q):
    """the binary64 sum rounded to binary32, as bits [nq, n]"""
    t = q[:, None, :].astype(np.float64) - db[None, :, :].astype(np.float64)
    return np.ascontiguousarray((t * t).sum(axis=2).astype(np.float32)).view(np.uint32)


def trap(nq=70, at=(5, 40, 69), a=7.0):
    """(db dict, q, at): row 0 is the zero vector, the other 20 rows are far away. Query at[0] has its only non-zero component `a` in
    dimension 0, query at[1] in dimension 127, query at[2] in dimension 0 again: all three at d2 = a^2 of row 0, whose partial sums
    reach it in the first and in the last step. at[0] takes the row from at[1] and keeps it against at[2]. The other queries sit
    on the far rows. A `>=` in place of `>` in an early exit, or an exit taken on a lane's own query, fails here."""
    rng = np.random.Generator(np.random.PCG64(127))
    desc = np.zeros((21, 128), np.float32)
    desc[1:] = rng.integers(100, 200, (20, 128)).astype(np.float32)
    q = desc[1 + np.arange(nq) % 20] + rng.integers(1, 4, (nq, 128)).astype(np.float32)
    for i, dim in zip(at, (0, 127, 0)):
        q[i] = 0
        q[i, dim] = a
    db = dict(desc=desc, pts=rng.standard_normal((21, 3)).astype(np.float32), off=np.array([0, 1, 21], np.uint32))
    return db, np.ascontiguousarray(q, np.float32), at


# ---- the ratio test's planted rows: scenario s lives around the base vector 1000 (s + 1) in dimensions 64 ... 127, which cancels
# exactly in every difference; its rows differ from its query in dimensions 0 ... 63 only
RATIO_SCENARIOS = ("twins", "zero_then_far", "zero_twice", "boundary_3_6", "boundary_3_next6", "second_beyond_radius_passes",
                   "second_beyond_radius_fails")
RATIO_RADIUS = 10.0
# keeps its matches at ratio 0.5 / 0.8 / 1.0?
RATIO_WANT = {"twins": (False, False, False), "zero_then_far": (True, True, True), "zero_twice": (False, False, False),
              "boundary_3_6": (False, True, True), "boundary_3_next6": (True, True, True),
              "second_beyond_radius_passes": (True, True, True), "second_beyond_radius_fails": (False, False, True)}


def ratio_planted():
    """(db dict, q f32[7, 128]): query s is RATIO_SCENARIOS[s]'s.
    twins: two identical rows at distance 5, nearest to the query -- dropped even at ratio 1. zero_then_far: d2 = (0, 16), kept.
    zero_twice: d2 = (0, 0), dropped. boundary_3_6: single-component rows at distances 3 and 6, 3 < 0.5 * 6 is false.
    boundary_3_next6: 6 replaced by the next binary32 above it, kept. second_beyond_radius_passes: rows at 3 and 100 with
    RATIO_RADIUS 10 -- the second decides although the radius cuts it. second_beyond_radius_fails: rows at 9 and 11, 9 < 0.8 * 11
    is false although only the first lies inside the radius."""
    rows, owner, qs = [], [], []
    nxt6 = np.nextafter(np.float32(6), np.float32(7))

    def e(dim, v):
        x = np.zeros(128, np.float32)
        x[dim] = v
        return x
    plan = {"twins": [e(3, 5), e(3, 5), e(4, 9)], "zero_then_far": [e(0, 0), e(5, 4)], "zero_twice": [e(0, 0), e(0, 0), e(1, 2)],
            "boundary_3_6": [e(7, 3), e(8, 6)], "boundary_3_next6": [e(7, 3), e(8, nxt6)],
            "second_beyond_radius_passes": [e(9, 3), e(10, 100)], "second_beyond_radius_fails": [e(11, 9), e(12, 11)]}
    for s, name in enumerate(RATIO_SCENARIOS):
        base = np.zeros(128, np.float32)
        base[64:] = 1000.0 * (s + 1)
        qs.append(base)
        for r in plan[name]:
            rows.append(base + r)
            owner.append(s)
    rng = np.random.Generator(np.random.PCG64(8))
    perm = rng.permutation(len(rows))                               # the twins are not neighbours in the DB
    desc = np.stack(rows)[perm]
    db = dict(desc=np.ascontiguousarray(desc), pts=rng.standard_normal((len(rows), 3)).astype(np.float32),
              off=np.array([0, 4, 4, len(rows)], np.uint32))
    return db, np.stack(qs)
