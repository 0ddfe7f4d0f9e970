"""Inputs shared by tests/test_l2_dim64_cpu.py and tests/test_l2_dim64_gpu.py: float DBs of 64 x f32 rows (desc_bytes 256).
The generators of l2_radius_cases.py, l2_sharded_ref.py and l2_numerics_cases.py restated at the narrower width -- those hard-code 128.
The numpy definitions themselves (match_l2_radius_ref, l2_sharded_ref's keys and merges, l2_filters_ref) take the width from their
arguments and are used as they are."""
import numpy as np

DIM = 64
ROWS = [0, 1, 31, 32, 33, 257, 5, 700]          # objects short of, on and past a 32-row tile; one empty; 1059 rows
FIELDS = ("queryIdx", "trainIdx", "imgIdx", "distance")
# no row / at most the planted row / most rows (two random integer rows are ~835 apart at 64 dimensions) / every row inside, no cut
RADII = (0.5, 100.0, 815.0, 1.0e4, 1.0e9)
LO = np.float32(1 + 2.0 ** -8 - 2.0 ** -22)      # rounds to 1 in bf16
HI = np.float32(1 + 2.0 ** -8 + 2.0 ** -22)      # rounds to 1 + 2^-7


class Db:
    """l2_radius_cases.Db at 64 dimensions: integer-valued rows 0..255 in objects of the given sizes (every d2 an integer below 2^24,
    exact in binary32). Queries: rows in turn with integer noise in a few dimensions (never none), every seventh random."""

    def __init__(self, rows=ROWS, nq=513, seed=2064):
        rng = np.random.Generator(np.random.PCG64(seed))
        n = int(sum(rows))
        self.off = np.concatenate([[0], np.cumsum(rows)]).astype(np.uint32)
        self.desc = rng.integers(0, 256, (n, DIM)).astype(np.float32)
        self.pts = rng.standard_normal((n, 3)).astype(np.float32)
        self.q = rng.integers(0, 256, (nq, DIM)).astype(np.float32)
        for i in range(nq):
            if i % 7 == 6:
                continue
            row = self.desc[(i * 37) % n].copy()
            dims = rng.choice(DIM, 1 + i % 40, replace=False)
            row[dims] = np.clip(row[dims] + rng.choice([-9, -4, -1, 1, 3, 12], len(dims)), 0, 255)
            if np.array_equal(row, self.desc[(i * 37) % n]):
                row[dims[0]] = 255 - row[dims[0]]
            self.q[i] = row


def boundary():
    """(desc, off, pts, q, radius): row 40 lies at d2 = 3600 of query 0 (36 dimensions off by 10: distance exactly 60 = radius), rows 41
    and 42 at d2 = 3601 and 3597, the other rows far away. Query 1 is query 0 + 100 000 in every dimension against rows shifted alike,
    query 2 the plain one again."""
    rng = np.random.Generator(np.random.PCG64(31))
    desc = rng.integers(0, 256, (100, DIM)).astype(np.float32)
    q0 = rng.integers(20, 230, DIM).astype(np.float32)
    desc[40] = q0; desc[40, :36] += 10                                   # 36 * 100 = 3600
    desc[41] = desc[40]; desc[41, DIM - 1] += 1                          # 3601
    desc[42] = desc[40]; desc[42, 0] -= 1; desc[42, DIM - 1] += 4        # 3600 - 100 + 81 + 16 = 3597
    big = np.float32(100000.0)
    desc = np.concatenate([desc, desc[38:44] + big])                     # rows 100..105: 102 on the boundary of query 1
    q = np.stack([q0, q0 + big, q0])
    pts = rng.standard_normal((len(desc), 3)).astype(np.float32)
    off = np.array([0, 41, 41, len(desc)], np.uint32)
    return desc, off, pts, q, np.float32(60.0)


def ragged_offsets(n):
    """three objects, the middle one empty, the cut off every tile boundary"""
    return np.array([0, n // 3 + 1, n // 3 + 1, n], np.uint32)


# ---------------------------------------------------------------------------------------------- the bound's worst-case families
def planted(k):
    """l2_numerics_cases.planted at 64 dimensions: q = 31 x LO, 31 x HI, 0, 0. A LOW row is -LO where the query is LO and +HI where it
    is HI: all 124 first-order error terms of <q^, r^> are positive and its score is 0.97 too low; HIGH = -LOW scores 0.97 too high.
    Dimension 62 carries a bf16-exact adjuster: the k HIGH rows are the true k nearest (d2 = 124.97 + (j / 16)^2), the k LOW rows
    decoys 0.8 ... 1.5 farther away -- less than the 1.94 by which the filter misjudges the pair."""
    q = np.zeros(DIM, np.float32)
    q[:31], q[31:62] = LO, HI
    low = np.zeros(DIM, np.float32)
    low[:31], low[31:62] = -LO, HI
    highs, lows = np.repeat(-low[None, :], k, 0), np.repeat(low[None, :], k, 0)
    highs[:, 62] = np.arange(k, dtype=np.float32) / 16
    lows[:, 62] = 1 + np.arange(k, dtype=np.float32) / 32
    return q, highs, lows


def adversarial_case(n, k, scale_exp=0, nq=64, seed=7):
    """(desc, off, pts, q, adversarial query indices, rows of the highs, rows of the lows): the planted rows at seeded places among
    fillers -alpha q + noise (norms below the planted rows', far behind them), everything scaled by 2^scale_exp."""
    rng = np.random.Generator(np.random.PCG64(seed + 1000 * k + n))
    q0, highs, lows = planted(k)
    desc = (-rng.uniform(0.6, 0.9, (n, 1)) * q0[None, :].astype(np.float64) + rng.normal(0, 0.15, (n, DIM))).astype(np.float32)
    where = rng.permutation(n)[:2 * k]
    desc[where[:k]], desc[where[k:]] = highs, lows
    q = rng.normal(0, 1, (nq, DIM)).astype(np.float32)
    adversarial = sorted({0, nq // 2 + 1, nq - 1})
    q[adversarial] = q0
    s = np.float32(2.0 ** scale_exp)
    pts = rng.standard_normal((n, 3)).astype(np.float32)
    return desc * s, ragged_offsets(n), pts, q * s, adversarial, where[:k], where[k:]


def _unit(x):
    x = np.asarray(x, np.float32)
    return (x / np.sqrt((x.astype(np.float64) ** 2).sum(axis=1, keepdims=True))).astype(np.float32)


def descriptor_classes():
    """{name: (desc, off, pts, q, radius)}: zeros, one coordinate 1e4 times the rest, an Rmax row 1e3 times the rows near the queries
    (l2_numerics_cases.descriptor_classes' three that stress the filter's arithmetic, at 64 dimensions; signed unit rows as SURF's)."""
    out = {}
    rng = np.random.Generator(np.random.PCG64(64))

    def add(name, desc, q, radius):
        n = len(desc)
        out[name] = (np.ascontiguousarray(desc, np.float32), ragged_offsets(n), rng.standard_normal((n, 3)).astype(np.float32),
                     np.ascontiguousarray(q, np.float32), radius)

    def near(desc, nq, sigma):
        idx = rng.integers(0, len(desc), nq)
        q = desc[idx] + rng.normal(0, sigma, (nq, DIM)).astype(np.float32) * np.abs(desc[idx]).max(axis=1, keepdims=True)
        q[1::2] = rng.permutation(q[1::2].T).T                           # every second one: dimensions shuffled, near nothing
        return q.astype(np.float32)

    signed = _unit(rng.normal(0, 1, (1500, DIM)))
    zeros = signed[:700].copy()
    zeros[[0, 31, 32, 33, 300, 301, 500, 698, 699]] = 0                  # nine exact zero rows, more than k
    qz = _unit(near(zeros[100:200], 40, 0.3))
    qz[[0, 5, 39]] = 0                                                   # zero queries: eps is its second term alone
    add("zero_vectors", zeros, qz, 0.5)
    add("zero_db", np.zeros((64, DIM), np.float32), np.stack([np.zeros(DIM, np.float32), signed[3], signed[4] * 0]), 1.0)
    dom = rng.normal(0, 1, (1200, DIM)).astype(np.float32)               # bf16 resolves nothing: every row is a candidate
    dom[:, 17] = 1.0e4 + rng.normal(0, 1, 1200)
    add("dominant_coordinate", dom, dom[rng.integers(0, 1200, 40)] + rng.normal(0, 0.3, (40, DIM)).astype(np.float32), 11.0)
    far = _unit(rng.normal(0, 1, (2100, DIM)))                           # the eps band holds every row: the exact scan answers
    far[1000] *= np.float32(1.0e3)
    add("rmax_row", far, _unit(near(np.delete(far, 1000, 0), 40, 0.3)), 1.3)
    return out


# ---------------------------------------------------------------------------------------------- the sharded and the filter tests' DB
TIE_SRC = 100
TIE_ROWS = np.union1d(np.arange(3, 1059, 7), np.arange(104, 1059, 7))   # copies of row 100, two in every seven rows: in every shard


def make_tie_db(seed=4264):
    """l2_sharded_ref.make_db at 64 dimensions: (desc f32[1059, 64], off u32[9], pts, q f32[33, 64]) over ROWS (one object empty); rows
    TIE_ROWS are copies of row TIE_SRC. Queries: a third exact copies of a DB row (every other one the tie's), a third near a row (the
    first near the tie's), the rest random."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = int(sum(ROWS))
    off = np.concatenate([[0], np.cumsum(ROWS)]).astype(np.uint32)
    desc = (rng.random((n, DIM)) * 200).astype(np.float32)
    desc[TIE_ROWS] = desc[TIE_SRC]
    pts = rng.standard_normal((n, 3)).astype(np.float32)
    nq = 33
    q = (rng.random((nq, DIM)) * 200).astype(np.float32)
    n0, n1 = len(q[0::3]), len(q[1::3])
    src0 = rng.integers(0, n, n0)
    src0[0::2] = TIE_SRC
    src1 = rng.integers(0, n, n1)
    src1[0] = TIE_SRC
    q[0::3] = desc[src0]
    q[1::3] = desc[src1] + rng.normal(0, 1.0, (n1, DIM)).astype(np.float32)
    return desc, off, pts, np.ascontiguousarray(q, np.float32)
