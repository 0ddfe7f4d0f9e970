"""The definition of todhip_set_db_bit_order's order (include/todhip.h) restated in numpy and Python integers, for
tests/test_bit_order_cpu.py and tests/test_bit_order_gpu.py. Not a test module."""
import numpy as np

E = (0, 4, 1, 5, 2, 6, 3, 7)          # rank block r // 32 -> dword: a matrix instruction of a block covers dwords s and s + 4
MAX_SAMPLE = 65536


def bits_of(desc):
    """u8[n, 32] -> u8[n, 256]: bit i of a descriptor is bit i % 8 (LSB first) of byte i // 8"""
    return np.unpackbits(np.ascontiguousarray(desc, np.uint8), axis=1, bitorder="little")


def stats_of_bits(X):
    """(S, ones[256], both[256][256]) of a 0/1 matrix [S, 256]; float32 sums of 0/1 products are exact up to 2^24 > 65536"""
    Xf = X.astype(np.float32)
    both = (Xf.T @ Xf).astype(np.int64)
    return len(X), np.diag(both).copy(), both


def sample_stats(desc):
    """the statistics of a resident shard: S = min(n, 65536) rows, sample row i = row floor(i * n / S)"""
    n = len(desc)
    S = min(n, MAX_SAMPLE)
    idx = (np.arange(S, dtype=np.int64) * n) // S
    return stats_of_bits(bits_of(desc[idx]))


def order_from_stats(S, ones, both):
    """-> (rank list, src_of u8[256]); exact (Python integers)"""
    ones = [int(x) for x in ones]
    both = np.asarray(both).tolist()
    v = [o * (S - o) for o in ones]
    acc, rej = [], []
    for b in sorted(range(256), key=lambda b: (-v[b], b)):
        ok = v[b] > 0 and all(4 * (S * both[a][b] - ones[a] * ones[b]) ** 2 < v[a] * v[b] for a in acc)
        (acc if ok else rej).append(b)
    rank = acc + rej
    src_of = np.zeros(256, np.uint8)
    for r, b in enumerate(rank):
        src_of[32 * E[r // 32] + r % 32] = b
    return rank, src_of


def order_of(desc):
    return order_from_stats(*sample_stats(desc))[1]
