"""numpy restatement of todhip_model_compact's definition (include/todhip.h): a sequential loop over the rows, each tested against
the rows kept so far. Written from the header's text, not from the kernels: float32 operation by operation in the stated order,
popcount through a 256-entry table."""
import numpy as np

POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.uint32)


def compact_ref(desc, pts, merge_dist, max_hamming):
    """desc u8[n, 32], pts f32[n, 3] -> (kept: indices of the kept rows, ascending; support u32[len(kept)])."""
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    md = np.float32(merge_dist)
    r2 = np.float32(md * md)
    kept, support = [], []
    kd = np.zeros((len(desc), 32), np.uint8)                 # the kept rows so far, in order
    kp = np.zeros((len(desc), 3), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(len(desc)):
            k = len(kept)
            ham = POPCOUNT[kd[:k] ^ desc[i]].sum(axis=1, dtype=np.uint32)
            dx = pts[i, 0] - kp[:k, 0]; dy = pts[i, 1] - kp[:k, 1]; dz = pts[i, 2] - kp[:k, 2]      # float32 throughout
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == np.float32
            conflict = (ham <= np.uint32(max_hamming)) & (d2 <= r2)                                # NaN: False
            hit = np.flatnonzero(conflict)
            if len(hit):
                support[hit[0]] += 1                         # the lowest-index conflicting kept row
            else:
                kd[k], kp[k] = desc[i], pts[i]
                kept.append(i); support.append(1)
    return np.asarray(kept, np.int64), np.asarray(support, np.uint32)


def random_model(seed, n_rows, n_base, merge_dist, max_hamming, spread=2.0):
    """A seeded synthetic model: n_rows rows, each a copy of one of n_base random base rows with 0 .. spread * max_hamming
    descriptor bits flipped and its point moved by 0 .. spread * merge_dist in a random direction, so that the copies of a base
    row lie on both sides of both bounds. In random order (a base row itself is not among the rows)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    base_d = rng.integers(0, 256, (n_base, 32), dtype=np.uint8)
    base_p = rng.random((n_base, 3)).astype(np.float32)
    which = rng.integers(0, n_base, n_rows)
    desc = base_d[which].copy()
    bits = np.unpackbits(desc, axis=1)
    for i in range(n_rows):
        flip = rng.choice(256, int(rng.integers(0, int(spread * max_hamming) + 1)), replace=False)
        bits[i, flip] ^= 1
    desc = np.packbits(bits, axis=1)
    direction = rng.normal(size=(n_rows, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    step = rng.random((n_rows, 1)) * spread * merge_dist
    pts = (base_p[which] + direction * step).astype(np.float32)
    return desc, pts
