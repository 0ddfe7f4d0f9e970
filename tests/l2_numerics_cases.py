"""Inputs shared by tests/test_l2_numerics_cpu.py and tests/test_l2_numerics_gpu.py: DBs and queries at which the float matcher's bf16
filter (tod_amd/csrc/l2_bound.h) is as wrong as it can be, and descriptor classes the rest of the suite never loads.

The adversarial construction. LO = 1 + 2^-8 - 2^-22 rounds to 1 in bf16 and HI = 1 + 2^-8 + 2^-22 to 1 + 2^-7: both move by 2^-8 of
their magnitude, the most round-to-nearest can do. The query is 63 x LO, 63 x HI, 0, 0. A LOW row is -LO where the query is LO and +HI
where it is HI: all 252 first-order error terms of <q^, r^> are positive and its score is 1.976 too low; a HIGH row is the negative of
that and scores 1.976 too high. Dimension 126, where the query is 0, carries a bf16-exact adjuster that moves d2 and the score alike,
so the k HIGH rows are made the true k nearest, pairwise distinct, and the k LOW rows decoys about 1 farther away. A filter whose
eps allows less than the error that bf16 can make (2^-6 |q||r|) sets its threshold by the decoys and drops the true neighbours.
Fillers are -alpha q + noise: norms below the planted rows' (so that Rmax and eps do not grow) and far behind them."""
import numpy as np

LO = np.float32(1 + 2.0 ** -8 - 2.0 ** -22)
HI = np.float32(1 + 2.0 ** -8 + 2.0 ** -22)
FIELDS = ("queryIdx", "trainIdx", "imgIdx", "distance")
NO_CUT = 3.0e38                                  # a k-NN radius beyond every distance at every scale used here

# the one-GEMM path: 2048 tiles of 32 rows, where l2_plan (tod_amd/csrc/l2_plan.h) samples every 4th tile from tile 0 on and the
# sample's seed is pass 2's threshold. tests/test_l2_numerics_cpu.py holds these against the plan itself.
ONE_GEMM_ROWS, TILE_ROWS, SAMPLE_STRIDE, SAMPLE_TILES = 65536, 32, 4, 512


class Case:
    """desc, off, pts, q: the call's inputs. adversarial: the query indices that carry the construction; highs / lows: the DB rows of
    the true neighbours (nearest first) and of the decoys."""

    def __init__(self, name, desc, off, pts, q, k, adversarial=(), highs=(), lows=()):
        self.name, self.desc, self.off, self.pts, self.q, self.k = name, desc, off, pts, q, k
        self.adversarial, self.highs, self.lows = list(adversarial), np.asarray(highs, np.int64), np.asarray(lows, np.int64)


def planted(k):
    """(q, highs[k], lows[k]) at scale 1; k = 1 is the triple q, r', r of the construction"""
    q = np.zeros(128, np.float32)
    q[:63], q[63:126] = LO, HI
    low = np.zeros(128, np.float32)
    low[:63], low[63:126] = -LO, HI
    highs, lows = np.repeat(-low[None, :], k, 0), np.repeat(low[None, :], k, 0)
    highs[:, 126] = np.arange(k, dtype=np.float32) / 16                  # d2 = 253.9726 + (j / 16)^2
    lows[:, 126] = 1 + np.arange(k, dtype=np.float32) / 32               # d2 = 253.9724 + (1 + j / 32)^2: 0.8 ... 1.5 behind every high
    return q, highs, lows


def fillers(rng, q, n):
    alpha = rng.uniform(0.6, 0.9, (n, 1))
    return (-alpha * q[None, :].astype(np.float64) + rng.normal(0, 0.15, (n, 128))).astype(np.float32)


def ragged_offsets(n):
    """three objects, the middle one empty, the cut off every tile boundary"""
    return np.array([0, n // 3 + 1, n // 3 + 1, n], np.uint32)


def adversarial_case(n, k, scale_exp=0, nq=64, positions=None, seed=7, filler=None):
    """The planted rows in a DB of n rows, everything scaled by 2^scale_exp (a power of two keeps every rounding pattern).
    positions: (rows of the highs, rows of the lows); by default a seeded choice. Queries: the adversarial one first, in the middle
    and last, random signed vectors of about its norm between them."""
    rng = np.random.Generator(np.random.PCG64(seed + 1000 * k + n))
    q0, highs, lows = planted(k)
    desc = fillers(rng, q0, n) if filler is None else filler.copy()
    if positions is None:
        where = rng.permutation(n)[:2 * k]
        positions = (where[:k], where[k:])
    desc[positions[0]], desc[positions[1]] = highs, lows
    q = rng.normal(0, 1, (nq, 128)).astype(np.float32)
    adversarial = sorted({0, nq // 2 + 1, nq - 1})
    q[adversarial] = q0
    s = np.float32(2.0 ** scale_exp)
    pts = rng.standard_normal((n, 3)).astype(np.float32)
    return Case("n%d_k%d_2^%d" % (n, k, scale_exp), desc * s, ragged_offsets(n), pts, q * s, k, adversarial, positions[0], positions[1])


def one_gemm_positions(k):
    """Decoys: one per sampled tile, 60 sampled tiles apart (so in k different chunks of the seed pass however it is cut) and in
    alternating lane halves -- the sample's k-th smallest partition minimum is then the k-th decoy's score and the seed is as tight
    as pass 1 would make it. True neighbours: in tiles the sample skips."""
    j = np.arange(k)
    lows = (32 + 60 * j) * SAMPLE_STRIDE * TILE_ROWS + (3 + 5 * j) % TILE_ROWS
    highs = ((40 + 50 * j) * SAMPLE_STRIDE + 1 + j % 3) * TILE_ROWS + (9 + 7 * j) % TILE_ROWS
    return highs, lows


def one_gemm_filler():
    return fillers(np.random.Generator(np.random.PCG64(65536)), planted(1)[0], ONE_GEMM_ROWS)


def one_gemm_case(k, filler):
    return adversarial_case(ONE_GEMM_ROWS, k, nq=32, positions=one_gemm_positions(k), filler=filler)


def radius_case():
    """the k = 1 triple in 2 100 rows; radii between the two planted distances and exactly on the nearer one"""
    c = adversarial_case(2100, 1)
    d2 = [d2_f32(c.q[0], c.desc[r]) for r in (c.highs[0], c.lows[0])]
    between = np.sqrt(np.float32((d2[0] + d2[1]) / 2))
    on = np.sqrt(d2[0])
    return c, (float(between), float(on))


def d2_f32(q, r):
    """the defining sequential f32 sum for one pair"""
    acc = np.float32(0)
    for a, b in zip(np.asarray(q, np.float32), np.asarray(r, np.float32)):
        t = np.float32(a - b)
        acc = np.float32(acc + np.float32(t * t))
    return acc


# ------------------------------------------------------------------------------------------------------ descriptor classes
def _unit(x):
    x = np.asarray(x, np.float32)
    return (x / np.sqrt((x.astype(np.float64) ** 2).sum(axis=1, keepdims=True))).astype(np.float32)


def _near(rng, desc, nq, sigma, renorm):
    """half of the queries next to a row, half random rows' negatives mixed (nothing near)"""
    idx = rng.integers(0, len(desc), nq)
    q = desc[idx] + rng.normal(0, sigma, (nq, 128)).astype(np.float32) * np.abs(desc[idx]).max(axis=1, keepdims=True)
    q[1::2] = rng.permutation(q[1::2].T).T                               # every second one: dimensions shuffled, near nothing
    return _unit(q) if renorm else q.astype(np.float32)


def descriptor_classes():
    """{name: (desc, off, pts, q, radius)}: what learned and hand-made 128-D float descriptors look like, and the zeros and signs
    the filter's arithmetic has to survive. Each runs at k = 1 and 8 and at the one radius."""
    out = {}
    rng = np.random.Generator(np.random.PCG64(128))

    def add(name, desc, q, radius):
        n = len(desc)
        out[name] = (np.ascontiguousarray(desc, np.float32), ragged_offsets(n), rng.standard_normal((n, 3)).astype(np.float32),
                     np.ascontiguousarray(q, np.float32), radius)

    signed = _unit(rng.normal(0, 1, (1500, 128)))                        # learned descriptors: signed, unit norm
    add("signed_unit", signed, _near(rng, signed, 48, 0.3, True), 1.3)
    sift = rng.integers(0, 256, (1500, 128)) * (rng.random((1500, 128)) < 0.6)
    root = np.sqrt(sift / sift.sum(axis=1, keepdims=True)).astype(np.float32)      # RootSIFT: L1-normalised, square roots
    add("rootsift", root, np.abs(_near(rng, root, 48, 0.2, True)), 0.8)
    dom = rng.normal(0, 1, (1200, 128)).astype(np.float32)               # one coordinate carries 1e4 times the rest: bf16 resolves
    dom[:, 17] = 1.0e4 + rng.normal(0, 1, 1200)                          # nothing, every row is a candidate
    qd = dom[rng.integers(0, 1200, 40)] + rng.normal(0, 0.3, (40, 128)).astype(np.float32)
    add("dominant_coordinate", dom, qd, 16.0)
    zeros = signed[:700].copy()
    zeros[[0, 31, 32, 33, 300, 301, 500, 698, 699]] = 0                  # nine exact zero rows, more than k
    qz = _near(rng, zeros[100:200], 40, 0.3, True)
    qz[[0, 5, 39]] = 0                                                   # zero queries: eps is its second term alone
    add("zero_vectors", zeros, qz, 0.5)
    add("zero_db", np.zeros((64, 128), np.float32), np.stack([np.zeros(128, np.float32), signed[3], signed[4] * 0]), 1.0)
    neg = (rng.normal(0, 1, (500, 128)) * (rng.random((500, 128)) < 0.5)).astype(np.float32)
    neg[neg == 0] = np.where(rng.random(int((neg == 0).sum())) < 0.5, np.float32(-0.0), np.float32(0.0))
    neg[77] = np.float32(-0.0)                                           # a row of negative zeros
    qn = neg[rng.integers(0, 500, 40)] + (rng.normal(0, 0.2, (40, 128)) * (rng.random((40, 128)) < 0.3)).astype(np.float32)
    qn[qn == 0] = np.float32(-0.0)
    qn[7] = np.float32(-0.0)
    add("negative_zeros", neg, qn, 6.0)
    far = _unit(rng.normal(0, 1, (2100, 128)))                           # Rmax 1e3 times the rows near the queries: the eps band holds
    far[1000] *= np.float32(1.0e3)                                       # every row and every query is answered by the exact scan
    add("rmax_row", far, _near(rng, np.delete(far, 1000, 0), 40, 0.3, True), 1.3)
    return out
