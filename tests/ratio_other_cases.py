"""Inputs of the ratio-other tests, shared by tests/test_ratio_other_cpu.py (which pins them on the numpy reference alone) and
tests/test_ratio_other_gpu.py. Random rows lie ~128 / ~256 bits apart, so everything of interest is planted:

  clusters    a base row plus copies with 1-4 flipped bits INSIDE one object, at the object's first and last row among other places;
  confusers   near copies of a base in ANOTHER object, exactly at rows lo - 1 and hi of the cluster's object (these must count as the
              other-object neighbour; the duplicates at lo and hi - 1 must not);
  queries     a cluster row (or a confuser) with 0-6 flipped bits.
Copies, confusers and queries flip bits in three disjoint regions of the row, so distances to a base add up exactly: a query n bits from
a base is n + c bits from a confuser c bits from it."""
import numpy as np

import ratio_other_ref as R
from tod_amd import capi

OBJ_ROWS = (0, 1, 31, 32, 33, 257, 5, 700)
OFF = np.concatenate([[0], np.cumsum(OBJ_ROWS)]).astype(np.uint32)   # 0 0 1 32 64 97 354 359 1059
N_ROWS = int(OFF[-1])
WIDTHS = (32, 64)
NQS = (1, 33, 70, 1100)                      # two, two, four and six query blocks per wave at 32 bytes; two, two, four, four at 64
RATIOS = (0.5, 0.75, 0.8, 1.0)
SENTINEL = 0x5A5A5A5A
COPY_BITS, QUERY_BITS, CONF_BITS = (0, 64), (64, 128), (128, 192)

# (object, home rows (the first holds the base itself), [(confuser row, bits from the base)])
CLUSTERS = (
    (2, (1, 2, 3), [(0, 4)]),                # object 2's first row; the confuser is row lo - 1 = the 1-row object
    (2, (31, 30), [(32, 5)]),                # object 2's last row; the confuser is row hi, object 3's first
    (5, (97, 98, 200), [(96, 2)]),           # object 5 straddles the first tile's end (rows 97 .. 353, tiles of 288 rows)
    (5, (353, 352, 150), [(354, 3)]),
    (7, (359, 360, 700), [(358, 7)]),        # object 7 runs over three tiles to the DB's last row: there is no row hi
    (7, (1058, 1057, 800), [(40, 9)]),
    (4, (64, 70, 95), [(63, 1)]),
    (6, (355, 356), [(600, 6)]),             # the 5-row object between two confusers of its neighbours
    (3, (33, 50), []),                       # no confuser: the other objects are random rows ~BITS / 2 away
)


def flip(row, bits):
    out = row.copy()
    for b in bits:
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


_db = {}


def make_db(width):
    """dict(desc u8[N_ROWS, width], pts f32[N_ROWS, 3], off, bases: each cluster's base row, conf_bits: the bits its confuser flips)"""
    if width in _db:
        return _db[width]
    rng = np.random.Generator(np.random.PCG64(4200 + width))
    desc = rng.integers(0, 256, (N_ROWS, width), dtype=np.uint8)
    bases, conf_bits = [], []
    for obj, homes, confusers in CLUSTERS:
        base = rng.integers(0, 256, width, dtype=np.uint8)
        bases.append(base)
        for i, r in enumerate(homes):
            assert OFF[obj] <= r < OFF[obj + 1]
            desc[r] = base if i == 0 else flip(base, rng.choice(np.arange(*COPY_BITS), int(rng.integers(1, 5)), replace=False))
        conf_bits.append([])
        for r, c in confusers:
            assert not OFF[obj] <= r < OFF[obj + 1]
            conf_bits[-1] = rng.choice(np.arange(*CONF_BITS), c, replace=False)
            desc[r] = flip(base, conf_bits[-1])
    _db[width] = dict(desc=np.ascontiguousarray(desc), pts=rng.standard_normal((N_ROWS, 3)).astype(np.float32), off=OFF, bases=bases,
                      conf_bits=conf_bits)
    return _db[width]


def make_queries(width, n):
    """n queries. Query i sits on cluster i % 10's rows -- "cluster" 9 is row 0, the 1-row object (itself a confuser of cluster 0) --
    on its home row (i // 70) % homes, with (i // 10) % 7 bits flipped. The first queries are the planted equalities:
      0: 4 bits from cluster 0's base, its confuser 4 further: d1 = 4, other = 8  (0.5: dropped, 4 < 4.0 fails)
      1: 4 bits from cluster 1's base, its confuser 5 further: d1 = 4, other = 9  (0.5: kept)
      2: 6 bits from cluster 2's base, its confuser 2 further: d1 = 6, other = 8  (0.75: dropped, 6 < 6.0 fails)"""
    db = make_db(width)
    rng = np.random.Generator(np.random.PCG64(9100 + 10 * width + n))
    qbits = np.arange(*QUERY_BITS)
    q = np.zeros((n, width), np.uint8)
    for i in range(n):
        cl, flips = i % 10, (i // 10) % 7
        if cl == 9:
            src = db["desc"][0]
        else:
            homes = CLUSTERS[cl][1]
            src = db["desc"][homes[(i // 70) % len(homes)]]
        q[i] = flip(src, rng.choice(qbits, flips, replace=False))
        if cl == 2 and flips % 2 == 1:
            # one of the two bits cluster 2's confuser flips: from the base the query is as far as from the confuser, an exact tie
            # between two objects (the confuser's row is the lower one: it is the nearest match, the base the other object's row)
            q[i] = flip(q[i], db["conf_bits"][2][:1])
    for i, (cl, flips) in enumerate(((0, 4), (1, 4), (2, 6))[:n]):
        q[i] = flip(db["bases"][cl], rng.choice(qbits, flips, replace=False))
    return q


def search_ref(db, q, stride, radius, searched=None, D=None):
    """What todhip_match_device (stride = k) and todhip_match_radius_device (stride = max_per_query) leave: per query the first `stride`
    searched rows within `radius` in the order (distance, row). Returns (counts, matches, D)."""
    nq = len(q)
    D = R.hamming(q, db["desc"]) if D is None else D
    counts = np.zeros(nq, np.uint32)
    m = np.frombuffer(bytes([0x5A]) * (nq * stride * 16), capi.DMATCH_DTYPE).copy()
    off = db["off"].astype(np.int64)
    rows = np.arange(N_ROWS) if searched is None else np.nonzero(searched)[0]
    for i in range(nq):
        order = rows[np.lexsort((rows, D[i][rows]))]
        order = order[D[i][order] <= radius][:stride]
        counts[i] = len(order)
        obj = np.searchsorted(off, order, side="right") - 1
        s = slice(i * stride, i * stride + len(order))
        m["queryIdx"][s], m["trainIdx"][s], m["imgIdx"][s], m["distance"][s] = i, order - off[obj], obj, D[i][order]
    return counts, m, D


def single_object_db(width, rows=300):
    """one object: no row of another object anywhere"""
    db = make_db(width)
    return dict(desc=np.ascontiguousarray(db["desc"][97:97 + rows]), pts=db["pts"][97:97 + rows], off=np.array([0, rows], np.uint32))
