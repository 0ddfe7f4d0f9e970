"""Child of tests/test_match_tails_gpu.py (TODHIP_K4X_QT is read once per process): hamming_topk_fp4rows on the constructed DBs of
tests/tails_cases.py -- a block that goes on loads the tails of its own step and of its own query -- each block form forced, against
the vector-ALU engine in the same context, bit for bit; then the two counters of the split-2 form against the CPU's count. The loops
themselves: tests/k4x_children.py."""
import k4x_children as C
import fastpath_cases as FC
import tails_cases as TC

# radius -> the block forms forced at it (0: whole blocks; their code path has no tails, one radius is enough)
FORMS = ((35, (2, 3, 0)), (36, (2, 3)), (90, (3,)))


def found(res, off, qi):
    """[(row, distance)] of query qi in a match result"""
    m = res[1][int(res[0][qi]):int(res[0][qi + 1])]
    return [(int(off[x["imgIdx"]]) + int(x["trainIdx"]), int(x["distance"])) for x in m]


def main():
    qt = C.qt_from_env()
    nq = C.nq_of(qt)
    ctx = C.capi.Context(0)
    n = 0
    for n_rows in FC.ROWS:
        desc, pts, off, q, plants = TC.make(n_rows, nq, qt, 4100 + n_rows)
        ctx.db_load(desc, pts, off)
        for k in (1, 2, 5):
            for radius, splits in FORMS:
                want = C.valu_answer(ctx, q, k, radius)
                if radius < 90:                                # the plants are the answers (the CPU test holds them to the oracle)
                    for p in plants:
                        d = p["a"] + p["b"]
                        assert found(want, off, p["query"]) == ([(p["row"], d)] if d <= radius else []), (n_rows, k, radius, p)
                n += C.compare_forms(ctx, q, k, radius, want, splits, n_rows)
        ctx.set_matcher_block_split(-1)
    ctx.close()
    for n_rows in (2113, 4479, 4065, 2049):
        desc, pts, off, q, plants = TC.make(n_rows, nq, qt, 5200 + n_rows, clean=True)
        C.check_split_counters(desc, pts, off, q, qt, n_rows)
        n += 1
    print("ok %d" % n)


if __name__ == "__main__":
    main()
