"""The float searches over a sharded DB (include/todhip.h: todhip_match_l2_shard_device + todhip_merge_l2_shards_device and
todhip_match_l2_radius_shard_device + todhip_merge_l2_radius_shards_device) in numpy, on tests/match_l2_radius_ref.py's d2: what a
shard sends, and the merge of what the shards sent. Also the small DB the CPU and GPU tests of the two pairs share.

A key is (binary32 bits of d2) << 32 | row of the full DB. The d2 of a (query, row) pair does not depend on which rows stand beside
it, so a shard's keys may be cut out of the d2 of the whole DB (`dd`), which the tests compute once."""
import numpy as np

import match_l2_radius_ref as R

PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
ROWS = [257, 33, 0, 300, 1, 31, 300, 32, 5, 100]           # objects short of, on and past the 32-row tile; 1059 rows
TIE_SRC = 100
TIE_ROWS = np.union1d(np.arange(3, 1059, 7), np.arange(104, 1059, 7))   # 288 copies of row 100, two in every seven rows: in every shard
NQ = 33
NEAR_SIGMA = 1.0                                           # a near query is about 11 from its row; random rows are about 900 apart


def keys_of(dd, rows):
    """u64[nq, len(rows)]: the keys of the global rows `rows` under the d2 matrix dd[nq, n]"""
    rows = np.asarray(rows, np.int64)
    return (np.ascontiguousarray(dd[:, rows]).view(np.uint32).astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)[None, :]


def shard_keys_knn(db, off, q, k, rows, dd=None):
    """u64[nq, k] of a shard that holds `rows` (ascending rows of the full DB): its min(k, len(rows)) nearest in key order, padding"""
    dd = R.d2(db, q) if dd is None else dd
    out = np.full((len(q), k), PAD, np.uint64)
    keys = np.sort(keys_of(dd, rows), axis=1)[:, :k]
    out[:, :keys.shape[1]] = keys
    return out


def shard_keys_radius(db, off, q, radius, mpq, rows, dd=None):
    """u64[nq, mpq + 1]: the first min(|R_s(q)|, mpq) keys of the shard's rows whose distance is not > radius, padding, |R_s(q)|"""
    dd = R.d2(db, q) if dd is None else dd
    rows = np.asarray(rows, np.int64)
    out = np.full((len(q), mpq + 1), PAD, np.uint64)
    keys = keys_of(dd, rows)
    inside = ~(np.sqrt(dd[:, rows]) > np.float32(radius))
    for qi in range(len(q)):
        mine = np.sort(keys[qi][inside[qi]])[:mpq]
        out[qi, :len(mine)] = mine
        out[qi, mpq] = int(inside[qi].sum())
    return out


def _resolve(keys, qi, off, pts):
    g = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    m = np.zeros(len(g), R.DMATCH_DTYPE)
    m["queryIdx"], m["distance"] = qi, np.sqrt((keys >> np.uint64(32)).astype(np.uint32).view(np.float32))
    m["imgIdx"] = np.searchsorted(off, g, side="right") - 1
    m["trainIdx"] = g - off[m["imgIdx"]]
    return m, np.asarray(pts, np.float32).reshape(-1, 3)[g]


def _pack(per_query):
    row_ptr = np.concatenate([[0], np.cumsum([len(m) for m, _ in per_query])]).astype(np.uint32)
    return row_ptr, np.concatenate([m for m, _ in per_query]), np.concatenate([x for _, x in per_query])


def merge_knn(keys_all, off, pts, k, radius):
    """u64[n_shards, nq, k] -> (row_ptr, matches, xyz): the k smallest keys of a query, cut at the first distance > radius"""
    keys_all = np.asarray(keys_all).view(np.uint64)
    off = np.asarray(off, np.int64)
    out = []
    for qi in range(keys_all.shape[1]):
        union = np.sort(keys_all[:, qi, :].reshape(-1))[:k]
        union = union[union != PAD]
        dist = np.sqrt((union >> np.uint64(32)).astype(np.uint32).view(np.float32))
        cut = np.flatnonzero(dist > np.float32(radius))
        out.append(_resolve(union[:cut[0]] if len(cut) else union, qi, off, pts))
    return _pack(out)


def merge_radius(keys_all, off, pts, mpq):
    """u64[n_shards, nq, mpq + 1] -> (row_ptr, matches, xyz, in_radius), the shape of match_l2_radius_ref.match_l2_radius"""
    keys_all = np.asarray(keys_all).view(np.uint64)
    off = np.asarray(off, np.int64)
    in_radius = keys_all[:, :, mpq].sum(axis=0)
    out = []
    for qi in range(keys_all.shape[1]):
        union = np.sort(keys_all[:, qi, :mpq].reshape(-1))
        union = union[union != PAD][:mpq]
        assert len(union) == min(int(in_radius[qi]), mpq)
        out.append(_resolve(union, qi, off, pts))
    return _pack(out) + (in_radius.astype(np.uint32),)


def make_queries(desc, nq, seed):
    """a third exact copies of a DB row (d2 = 0; every other one of them the tie's row), a third near a row (the first near the tie's),
    the rest random"""
    rng = np.random.Generator(np.random.PCG64(seed))
    q = (rng.random((nq, 128)) * 200).astype(np.float32)
    n0, n1 = len(q[0::3]), len(q[1::3])
    src0 = rng.integers(0, len(desc), n0)
    src0[0::2] = TIE_SRC
    src1 = rng.integers(0, len(desc), n1)
    src1[0] = TIE_SRC
    q[0::3] = desc[src0]
    q[1::3] = desc[src1] + rng.normal(0, NEAR_SIGMA, (n1, 128)).astype(np.float32)
    return np.ascontiguousarray(q, np.float32)


def make_db(seed=4243):
    """(desc f32[1059, 128], off u32[11], pts f32[1059, 3], q f32[33, 128]); rows TIE_ROWS are copies of row TIE_SRC"""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = int(sum(ROWS))
    off = np.concatenate([[0], np.cumsum(ROWS)]).astype(np.uint32)
    desc = (rng.random((n, 128)) * 200).astype(np.float32)
    desc[TIE_ROWS] = desc[TIE_SRC]
    pts = rng.standard_normal((n, 3)).astype(np.float32)
    return desc, off, pts, make_queries(desc, NQ, seed + 1)


def radii(desc, q):
    """(just short of the tie for the query near it, exactly on the tie, among the random rows' distances, beyond every row)"""
    on_tie = np.sqrt(R.d2(desc[TIE_SRC:TIE_SRC + 1], q[1:2]))[0, 0]
    return float(np.nextafter(on_tie, np.float32(0))), float(on_tie), 900.0, 1.0e9
