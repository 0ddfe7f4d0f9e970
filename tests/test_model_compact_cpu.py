"""todhip_model_compact / todhip_model_add_rows without a GPU: the exported symbols, the header as C99, the null-argument statuses, and
known answers of the numpy restatement (tests/model_compact_ref.py), each worked by hand here. The call has no host-side table code
(everything between its argument checks and its read-back runs on the device), so there is no stand-alone sanitised program."""
import os
import subprocess
import sys

import numpy as np

from tod_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from model_compact_ref import POPCOUNT, compact_ref, random_model   # noqa: E402

NEW = ("todhip_model_add_rows", "todhip_model_compact")


def _desc(*bits):
    """a descriptor with exactly the given bits set (bit b = byte b // 8, bit b % 8)"""
    d = np.zeros(32, np.uint8)
    for b in bits:
        d[b // 8] |= 1 << (b % 8)
    return d


def test_symbols_are_exported_and_declared():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "todhip.h")).read()
    for n in NEW:
        assert hasattr(L, n), n
        assert n + "(" in header and n in capi.EXPORTS
    assert callable(capi.Model.add_rows) and callable(capi.Model.compact)


def test_header_with_the_new_calls_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "todhip.h"\n'
                   "int f(todhip_ctx* c, todhip_model* m, const uint8_t* d, const float* p) {\n"
                   "  uint32_t added = 0, before = 0, after = 0, sup[4], ns = 4;\n"
                   "  int rc = todhip_model_add_rows(c, m, d, p, 4, &added) + todhip_model_add_rows(c, m, NULL, NULL, 0, NULL);\n"
                   "  rc += todhip_model_compact(c, m, 0.003f, 24, &before, &after, sup, &ns);\n"
                   "  rc += todhip_model_compact(c, m, 0.f, 256, NULL, NULL, NULL, NULL);\n"
                   "  return rc + (int)(added + before + after + ns + sup[0]);\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "t.o")], check=True)


def test_null_arguments_are_invalid():
    L = capi.lib()
    n = capi.C.c_uint32(7)
    assert L.todhip_model_compact(None, None, 0.01, 10, capi.C.byref(n), None, None, None) == capi.EINVAL
    assert n.value == 7
    assert L.todhip_model_add_rows(None, None, None, None, 0, None) == capi.EINVAL


def test_popcount_table():
    assert POPCOUNT[0] == 0 and POPCOUNT[255] == 8 and POPCOUNT[0x81] == 2 and int(POPCOUNT.sum()) == 1024


def test_chain_is_not_transitive():
    """A = 0, B = 0.6, C = 1.2 on the x axis, merge_dist 1: A-B and B-C conflict (0.36 <= 1), A-C does not (1.44 > 1).
    A is kept, B goes (to A), C meets only kept A and is kept."""
    pts = np.array([[0, 0, 0], [0.6, 0, 0], [1.2, 0, 0]], np.float32)
    desc = np.zeros((3, 32), np.uint8)
    kept, sup = compact_ref(desc, pts, 1.0, 0)
    assert kept.tolist() == [0, 2] and sup.tolist() == [2, 1]


def test_hamming_bound_is_inclusive():
    desc = np.stack([_desc(), _desc(0, 9, 255)])                       # ham = 3
    pts = np.zeros((2, 3), np.float32)
    assert compact_ref(desc, pts, 0.0, 3)[0].tolist() == [0]
    assert compact_ref(desc, pts, 0.0, 2)[0].tolist() == [0, 1]
    desc = np.stack([_desc(), _desc(*range(256))])                     # ham = 256: only max_hamming == 256 ignores descriptors
    assert compact_ref(desc, pts, 0.0, 256)[0].tolist() == [0]
    assert compact_ref(desc, pts, 0.0, 255)[0].tolist() == [0, 1]


def test_distance_bound_is_inclusive():
    """(0,0,0) and (0.5,0,0): d2 = 0.25 exactly; merge_dist 0.5 -> r2 = 0.25, merged; the float32 below 0.5 squares to less"""
    pts = np.array([[0, 0, 0], [0.5, 0, 0]], np.float32)
    desc = np.zeros((2, 32), np.uint8)
    assert compact_ref(desc, pts, 0.5, 0)[0].tolist() == [0]
    assert compact_ref(desc, pts, np.nextafter(np.float32(0.5), np.float32(0)), 0)[0].tolist() == [0, 1]
    # merge_dist 0: equal points only, and -0 == +0
    pts = np.array([[0.0, 1, 2], [-0.0, 1, 2], [np.float32(1e-10), 1, 2]], np.float32)
    assert compact_ref(np.zeros((3, 32), np.uint8), pts, 0.0, 0)[0].tolist() == [0, 2]


def test_nan_point_is_kept_and_inf_point_conflicts_with_nothing():
    pts = np.array([[0, 0, 0], [np.nan, 0, 0], [0, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [np.inf, 0, 0]], np.float32)
    kept, sup = compact_ref(np.zeros((6, 32), np.uint8), pts, 10.0, 256)
    # inf - inf = NaN and inf - 0 = inf > r2: the Inf rows conflict with nothing either
    assert kept.tolist() == [0, 1, 3, 4, 5] and sup.tolist() == [2, 1, 1, 1, 1]


def test_support_goes_to_the_lowest_conflicting_kept_row():
    """K0 = 0, K1 = 1.5 are both kept (2.25 > 1); X = 0.75 conflicts with both (0.5625 <= 1) and counts for K0 although K1
    is as near; Y = 2.0 conflicts with K1 only"""
    pts = np.array([[0, 0, 0], [1.5, 0, 0], [0.75, 0, 0], [2.0, 0, 0]], np.float32)
    kept, sup = compact_ref(np.zeros((4, 32), np.uint8), pts, 1.0, 0)
    assert kept.tolist() == [0, 1] and sup.tolist() == [2, 2]


def test_idempotent_and_support_sums_to_the_rows():
    desc, pts = random_model(3, 400, 60, 0.01, 20, spread=1.2)
    kept, sup = compact_ref(desc, pts, 0.01, 20)
    assert 0 < len(kept) < 400 and int(sup.sum()) == 400
    kept2, sup2 = compact_ref(desc[kept], pts[kept], 0.01, 20)
    assert kept2.tolist() == list(range(len(kept))) and (sup2 == 1).all()


def test_the_gpu_tests_random_models_are_what_they_claim():
    """tests/test_model_compact_gpu.py's two seeded models: the first drops at least a third of its rows and still keeps more than 1024
    (the kept front crosses lane, workgroup and the 1024 boundary); the second keeps about 2500 of 3000, beyond 2048."""
    import test_model_compact_gpu as g
    desc, pts = random_model(*g.MODEL_A)
    kept, _ = compact_ref(desc, pts, g.MODEL_A[3], g.MODEL_A[4])
    assert len(desc) == 2000 and 1024 < len(kept) <= 2000 * 2 // 3
    desc, pts = random_model(*g.MODEL_B)
    kept, _ = compact_ref(desc, pts, g.MODEL_B[3], g.MODEL_B[4])
    assert len(desc) == 3000 and 2400 <= len(kept) <= 2600
