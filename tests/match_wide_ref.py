"""The definition of todhip_match on a DB of 64-byte (512-bit) binary descriptors, stated in numpy (include/todhip.h; decision D1):
Hamming distance over all bits by a popcount table, the rows ordered by (distance, global row) with a lexsort, the first k of them,
cut at the first distance > radius; with the ratio test, a query whose two nearest rows d1 <= d2 do not satisfy
(float)d1 < ratio * (float)d2 keeps nothing (a one-row DB passes). Any descriptor width. Test infrastructure only: the CPU test
holds it against the oracle (oracle_lib.match), which is what the GPU is held to.

Also the shared test data of the wide matcher's tests: WideDb."""
import numpy as np

POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.uint16)
DMATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])

ROWS = [0, 1, 31, 32, 33, 257, 5, 700]      # short of, on and past a 32-row step; an empty object first


def distances(desc, q):
    """u16[nq, n]"""
    desc, q = np.asarray(desc, np.uint8), np.asarray(q, np.uint8)
    out = np.zeros((len(q), len(desc)), np.uint16)
    for i in range(len(q)):
        out[i] = POPCOUNT[desc ^ q[i]].sum(axis=1, dtype=np.uint16)
    return out


def match(desc, off, pts, q, k, radius, ratio=0.0):
    """(row_ptr u32[nq+1], matches DMATCH[n], xyz f32[n,3])"""
    off = np.asarray(off, np.int64)
    d_all = distances(desc, q)
    rows = np.arange(len(desc))
    rp, ms, xs = [0], [], []
    for qi in range(len(q)):
        d = d_all[qi]
        order = np.lexsort((rows, d))
        kept = []
        ambiguous = (ratio > 0 and len(order) >= 2 and
                     not (np.float32(d[order[0]]) < np.float32(ratio) * np.float32(d[order[1]])))
        if not ambiguous:
            for r in order[:k]:
                if int(d[r]) > radius:
                    break
                kept.append(int(r))
        for r in kept:
            o = int(np.searchsorted(off, r, side="right")) - 1
            ms.append((qi, r - int(off[o]), o, float(d[r])))
            xs.append(pts[r])
        rp.append(len(ms))
    return (np.asarray(rp, np.uint32), np.array(ms, DMATCH_DTYPE) if ms else np.zeros(0, DMATCH_DTYPE),
            np.asarray(xs, np.float32).reshape(-1, 3))


def flip(row, bits):
    b = np.unpackbits(row, bitorder="little")
    b[np.asarray(bits, np.int64)] ^= 1
    return np.packbits(b, bitorder="little")


class WideDb:
    """Random rows of `width` bytes in objects of the given sizes, and 70 queries. Random wide rows never come within 200 bits of each
    other, so the neighbours are planted: query 0 is a row with 3 flipped bits, all in bytes 32..63; query 1 one with 3, all in
    bytes 0..31; query 2 the complement of a row (distance 512 at 64 bytes); query 3 a row with only its last bit flipped (bit 511) --
    and the DB holds a second copy of that row which differs from it in that bit alone, so the two are at distances 0 and 1;
    every seventh query is random; the rest are rows with 0..80 flipped bits spread over the whole row, every fifth of those with its
    flips in the upper half only and every fifth in the lower half only."""

    def __init__(self, rows=ROWS, width=64, seed=2025, n_q=70):
        rng = np.random.Generator(np.random.PCG64(seed))
        n, nbits, half = int(sum(rows)), 8 * width, 4 * width
        self.off = np.concatenate([[0], np.cumsum(rows)]).astype(np.uint32)
        self.desc = rng.integers(0, 256, (n, width), dtype=np.uint8)
        self.pts = rng.standard_normal((n, 3)).astype(np.float32)
        self.last_bit_pair = (n - 300, n - 7)                               # rows that differ in the last bit alone
        self.desc[n - 7] = flip(self.desc[n - 300], [nbits - 1])
        self.q = rng.integers(0, 256, (n_q, width), dtype=np.uint8)
        full = [o for o in range(len(rows)) if rows[o] > 0]
        for i in range(n_q):
            if i % 7 == 6:
                continue
            o = full[i % len(full)]
            r = int(self.off[o]) + int(rng.integers(0, rows[o]))
            nf = int(rng.integers(0, 81))
            lo, hi = (half, nbits) if i % 5 == 0 else ((0, half) if i % 5 == 1 else (0, nbits))
            self.q[i] = flip(self.desc[r], lo + rng.choice(hi - lo, nf, replace=False))
        self.q[0] = flip(self.desc[n - 100], half + rng.choice(half, 3, replace=False))
        self.q[1] = flip(self.desc[n - 101], rng.choice(half, 3, replace=False))
        self.q[2] = ~self.desc[n - 102]
        self.q[3] = flip(self.desc[n - 300], [nbits - 1])                   # == row n - 7; row n - 300 is one bit away

    def subset(self, sel):
        """(S, desc, pts, off) of the ascending distinct object indices of sel"""
        S = sorted(set(sel))
        rows = np.concatenate([np.arange(self.off[o], self.off[o + 1]) for o in S] + [np.zeros(0, np.int64)]).astype(np.int64)
        off = np.concatenate([[0], np.cumsum([int(self.off[o + 1] - self.off[o]) for o in S])]).astype(np.uint32)
        return np.asarray(S, np.int32), self.desc[rows], self.pts[rows], off
