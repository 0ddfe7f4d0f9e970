"""Child of tests/test_match_fp4_rows_gpu.py (TODHIP_K4X_FP4_ROWS and TODHIP_K4X_QT are read once per process): the matrix-core search
over the resident fp4 copy of the rows against the vector-ALU engine in the same process, bit for bit, in every block form. The
comparison itself: tests/k4x_children.py."""
import itertools

import numpy as np

import k4x_children as C


def flip(rows, rng, n_bits):
    out = rows.copy()
    for i in range(len(out)):
        for b in rng.choice(256, n_bits, replace=False):
            out[i, b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def make(kind, n_rows, nq, seed):
    """kind 0: independent bits, a third of the queries near a row; 1 / 2: every row equals one query on its first 128 / 192 bit
    positions, so the split blocks go on to their second part; 3: rows drawn from 40 distinct ones (ties, broken by the row index)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    if kind == 3:
        pool = rng.integers(0, 256, (40, 32), dtype=np.uint8)
        desc = pool[rng.integers(0, 40, n_rows)]
        q = flip(pool[rng.integers(0, 40, nq)], rng, 9)
    else:
        desc = rng.integers(0, 256, (n_rows, 32), dtype=np.uint8)
        q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
        near = rng.choice(nq, nq // 3, replace=False)
        q[near] = flip(desc[rng.integers(0, n_rows, len(near))], rng, 20)
        if kind in (1, 2):
            nb = 16 if kind == 1 else 24
            desc[:, :nb] = q[np.arange(n_rows) % nq, :nb]
    pts = rng.random((n_rows, 3), dtype=np.float32)
    off = np.array([0, n_rows // 3, 2 * n_rows // 3, n_rows], np.uint32)
    return np.ascontiguousarray(desc), pts, off, np.ascontiguousarray(q)


def compare(ctx, q, ks, radii, splits, what):
    n = 0
    for k, radius in itertools.product(ks, radii):
        n += C.compare_forms(ctx, q, k, radius, C.valu_answer(ctx, q, k, radius), splits, what)
    ctx.set_matcher_block_split(-1)
    return n


def main():
    C.qt_from_env()
    ctx = C.capi.Context(0)
    n, builds = 0, 0
    for kind, n_rows, nq in itertools.product((0, 1, 2, 3), (4096, 4113, 8191), (129, 200)):
        desc, pts, off, q = make(kind, n_rows, nq, 1000 * kind + n_rows + nq)
        ctx.db_load(desc, pts, off)
        n += compare(ctx, q, (1, 2, 5), (35, 64, 96, 255), (0, 2, 3), (kind, n_rows, nq))
        builds += 1
        assert ctx.counters().fp4_rows_builds == builds                    # one copy per load, whatever the number of launches
    # the copy follows the rows: a second load on the same context (above, 23 times), a selection on and off, the bit order on and off
    desc, pts, off, q = make(1, 4113, 200, 7)
    ctx.db_load(desc, pts, off)
    n += compare(ctx, q, (2,), (35, 96), (0, 2, 3), "load")
    for ids in ([0, 2], [1], None):
        ctx.select_objects(ids)
        n += compare(ctx, q, (2,), (35, 96), (0, 2, 3), ("select", ids))
    assert ctx.counters().fp4_rows_builds == builds + 4
    for mode in (1, 0):
        ctx.set_db_bit_order(mode)
        ctx.db_load(desc, pts, off)
        n += compare(ctx, q, (2,), (35, 96), (0, 2, 3), ("bit order", mode))
    ctx.select_objects([2, 1])
    ctx.set_db_bit_order(1)
    ctx.db_load(desc, pts, off)                                              # a load selects all objects again
    n += compare(ctx, q, (1, 5), (64, 255), (0, 3), "load over a selection")
    ctx.close()
    print("ok %d" % n)


if __name__ == "__main__":
    main()
