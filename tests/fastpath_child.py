"""Child of tests/test_match_fastpath_gpu.py (TODHIP_K4X_QT is read once per process): the split-block fast path of hamming_topk_fp4rows
on the constructed DBs of tests/fastpath_cases.py, each block form forced, against the vector-ALU engine in the same context, bit for
bit; then the pass counter of the split-2 form against the CPU's count. The loops themselves: tests/k4x_children.py."""
import k4x_children as C
import fastpath_cases as FC


def main():
    qt = C.qt_from_env()
    nq = C.nq_of(qt)
    ctx = C.capi.Context(0)
    n = 0
    for n_rows in FC.ROWS:
        desc, pts, off, q, plants = FC.make(n_rows, nq, qt, 77 + n_rows)
        ctx.db_load(desc, pts, off)
        for k in (1, 2, 5):
            for radius, splits in ((35, (2, 3, 0)), (90, (3,))):
                want = C.valu_answer(ctx, q, k, radius)
                for row, qi, kind in plants:                   # the planted rows are the answers (the CPU test holds them to the oracle)
                    if kind == "full" or (kind == "part3" and radius == 90):
                        m = want[1][want[0][qi]]
                        assert int(off[m["imgIdx"]]) + int(m["trainIdx"]) == row and int(m["distance"]) == (0 if kind == "full" else 64), (n_rows, row, qi, kind)
                n += C.compare_forms(ctx, q, k, radius, want, splits, n_rows)
        ctx.set_matcher_block_split(-1)
    ctx.close()
    for n_rows in (2113, 4479, 4065):
        desc, pts, off, q, plants = FC.make(n_rows, nq, qt, 991 + n_rows, only_part2=True)
        C.check_split_counters(desc, pts, off, q, qt, n_rows)
        n += 1
    print("ok %d" % n)


if __name__ == "__main__":
    main()
