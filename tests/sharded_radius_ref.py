"""The radius search over a sharded DB (include/todhip.h: todhip_match_radius_shard_device + todhip_merge_radius_shards_device) in
numpy, on tests/match_radius_ref.py: what a shard sends, and the merge of what the shards sent. Also the small DB the CPU and GPU
tests of the pair share."""
import numpy as np

import match_radius_ref as R

PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
ROWS = [257, 33, 0, 300, 1, 31, 300, 32, 5, 100]           # objects short of, on and past a 32-row step; 1059 rows
TIE_ROWS = np.arange(200, 800, 2)                          # 300 copies of row 100: 195 below row 590, 105 from it on
NQ = 33


def shard_keys(db, off, pts, q, radius, mpq, rows):
    """u64[nq, mpq + 1] of a shard (or selection) that searches `rows` (ascending rows of the full DB): the nearest
    min(|R_s(q)|, mpq) keys distance << 32 | row ascending, padding, and |R_s(q)| in the last slot"""
    off = np.asarray(off, np.int64)
    rp, m, _, in_radius = R.match_radius(db, off, pts, q, radius, mpq, rows=rows)
    out = np.full((len(q), mpq + 1), PAD, np.uint64)
    key = (m["distance"].astype(np.uint64) << np.uint64(32)) | (off[m["imgIdx"]] + m["trainIdx"]).astype(np.uint64)
    for qi in range(len(q)):
        out[qi, :int(rp[qi + 1] - rp[qi])] = key[rp[qi]:rp[qi + 1]]
    out[:, mpq] = in_radius
    return out


def merge(keys_all, off, pts, mpq):
    """u64[n_shards, nq, mpq + 1] -> (row_ptr, matches, xyz, in_radius), the shape of match_radius_ref.match_radius"""
    keys_all = np.asarray(keys_all).view(np.uint64)
    off = np.asarray(off, np.int64)
    n_shards, nq, _ = keys_all.shape
    in_radius = keys_all[:, :, mpq].sum(axis=0)
    row_ptr, ms = [0], []
    for qi in range(nq):
        union = np.sort(keys_all[:, qi, :mpq].reshape(-1))
        union = union[union != PAD][:mpq]
        assert len(union) == min(int(in_radius[qi]), mpq)
        g = (union & np.uint64(0xFFFFFFFF)).astype(np.int64)
        m = np.zeros(len(g), R.DMATCH_DTYPE)
        m["queryIdx"], m["distance"] = qi, (union >> np.uint64(32)).astype(np.float32)
        m["imgIdx"] = np.searchsorted(off, g, side="right") - 1
        m["trainIdx"] = g - off[m["imgIdx"]]
        ms.append((m, np.asarray(pts, np.float32)[g].reshape(-1, 3)))
        row_ptr.append(row_ptr[-1] + len(g))
    return (np.asarray(row_ptr, np.uint32), np.concatenate([m for m, _ in ms]), np.concatenate([x for _, x in ms]),
            in_radius.astype(np.uint32))


def make_queries(desc, nq, seed):
    """every third query equal to row 100 (the 300-way tie), every third a DB row, the rest random"""
    rng = np.random.Generator(np.random.PCG64(seed))
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    q[0::3] = desc[100]
    q[1::3] = desc[rng.integers(0, len(desc), len(q[1::3]))]
    return q


def make_db(seed=4242):
    """(desc u8[1059, 32], off u32[11], pts f32[1059, 3], q u8[33, 32])"""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = int(sum(ROWS))
    off = np.concatenate([[0], np.cumsum(ROWS)]).astype(np.uint32)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    desc[TIE_ROWS] = desc[100]
    pts = rng.standard_normal((n, 3)).astype(np.float32)
    return desc, off, pts, make_queries(desc, NQ, seed + 1)
