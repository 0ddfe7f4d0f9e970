"""Inputs shared by tests/test_match_l2_radius_cpu.py and tests/test_match_l2_radius_gpu.py: the float DB at the edges of the 32-row
tile and the planted boundary rows. Descriptors are integer-valued floats 0..255 (what OpenCV's SIFT stores): every d2 is an integer
below 2^24, exact in binary32 whatever the order of the sum, so a distance can be put EXACTLY on a radius."""
import numpy as np

ROWS = [0, 1, 31, 32, 33, 257, 5, 700]          # objects short of, on and past a 32-row tile; one empty
NQ = 600                                        # the CPU test uses the first 70
# no row / some rows / about a third of the rows / every row inside (two random rows are ~1180 apart, no two farther than 2886)
RADII = (0.5, 150.0, 1150.0, 1.0e4)
MPQS = (1, 5, 8, 64, 1024)
FIELDS = ("queryIdx", "trainIdx", "imgIdx", "distance")


class Db:
    """Random rows in objects of the given sizes. Queries: rows in turn with integer noise in a few dimensions (never none: no query
    equals a row, so the smallest radius admits nothing), every seventh random."""

    def __init__(self, rows=ROWS, nq=NQ, seed=2025):
        rng = np.random.Generator(np.random.PCG64(seed))
        n = int(sum(rows))
        self.off = np.concatenate([[0], np.cumsum(rows)]).astype(np.uint32)
        self.desc = rng.integers(0, 256, (n, 128)).astype(np.float32)
        self.pts = rng.standard_normal((n, 3)).astype(np.float32)
        self.q = rng.integers(0, 256, (nq, 128)).astype(np.float32)
        for i in range(nq):
            if i % 7 == 6:
                continue
            row = self.desc[(i * 37) % n].copy()
            dims = rng.choice(128, 1 + i % 40, replace=False)
            row[dims] = np.clip(row[dims] + rng.choice([-9, -4, -1, 1, 3, 12], len(dims)), 0, 255)
            if np.array_equal(row, self.desc[(i * 37) % n]):
                row[dims[0]] = 255 - row[dims[0]]                        # (clipped back onto the row)
            self.q[i] = row


def boundary():
    """(desc, off, pts, q, radius): row 40 lies at d2 = 3600 of query 0 (36 dimensions off by 10: distance exactly 60 = radius), rows 41
    and 42 at d2 = 3601 and 3597, the other rows far away. Query 1 is query 0 + 100 000 in every dimension against rows shifted alike
    (the same differences under a norm of 1.1e6, where bf16 resolves nothing), query 2 the plain one again."""
    rng = np.random.Generator(np.random.PCG64(31))
    desc = rng.integers(0, 256, (100, 128)).astype(np.float32)
    q0 = rng.integers(20, 230, 128).astype(np.float32)
    desc[40] = q0; desc[40, :36] += 10                                   # 36 * 100 = 3600
    desc[41] = desc[40]; desc[41, 127] += 1                              # 3601
    desc[42] = desc[40]; desc[42, 0] -= 1; desc[42, 127] += 4            # 3600 - 100 + 81 + 16 = 3597
    big = np.float32(100000.0)
    desc = np.concatenate([desc, desc[38:44] + big])                     # rows 100..105: 102 on the boundary of query 1
    q = np.stack([q0, q0 + big, q0])
    pts = rng.standard_normal((len(desc), 3)).astype(np.float32)
    off = np.array([0, 41, 41, len(desc)], np.uint32)
    return desc, off, pts, q, np.float32(60.0)
