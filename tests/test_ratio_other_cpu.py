"""Lowe's ratio test against another object without a GPU: the numpy definition (tests/ratio_other_ref.py) pinned on the oracle's sorted
keys; tod_amd/csrc/ratio_other.h (predicate, limit, interval clamp) in a stand-alone host program built with
-fsanitize=address,undefined; what the header declares and says; and the inputs of tests/test_ratio_other_gpu.py pinned on the
reference alone, so that the GPU test cannot pass vacuously: the planted equalities decide as stated, every ratio drops some queries
and keeps some, confusers at lo - 1 and hi are the other-object neighbours and the duplicates at lo and hi - 1 are not."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import ratio_other_cases as RC
import ratio_other_ref as R
from tod_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("width", RC.WIDTHS)
def test_reference_equals_the_oracles_first_key_of_another_object(width):
    db = RC.make_db(width)
    q = RC.make_queries(width, 70)
    keys = O.knn_keys(db["desc"], q, RC.N_ROWS)                    # every row of every query, ascending (distance << 32 | row)
    D = R.hamming(q, db["desc"])
    obj = R.row_objects(db["off"])
    kd, kr = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert np.array_equal(kd, np.sort(D, axis=1))                  # the tables agree
    for excl in (obj[kr[:, 0]], np.full(70, 5), np.full(70, 0), np.full(70, R.NONE)):     # the nearest row's object; one; the empty one; none
        want = np.zeros(70, np.uint32)
        for i in range(70):
            j = int(np.argmax(obj[kr[i]] != excl[i]))              # the first key of another object
            want[i] = kd[i, j]
        assert np.array_equal(R.other(D, db["off"], excl), want)
    assert np.array_equal(R.other(D, db["off"], np.full(70, R.NONE)), kd[:, 0])
    # a searched set of one object: nothing else is there
    only5 = R.searched_mask(db["off"], selection=[5])
    assert (R.other(D, db["off"], np.full(70, 5), only5) == R.NONE).all()
    assert (R.other(D, db["off"], np.full(70, 2), only5) != R.NONE).all()


def test_reference_limit_and_predicate():
    d1 = np.arange(513)
    for ratio in RC.RATIOS:
        L = R.limit(d1, ratio)
        assert R.passes(d1, ratio, L).all() and not R.passes(d1[1:], ratio, L[1:] - 1).any() and (L >= 1).all()
        # min(other, L) decides as other does, for every other
        for o in (0, 1, 7, 8, 9, 44, 200, 512):
            both = np.minimum(L, o)
            assert np.array_equal(R.survives(d1, ratio, both), R.survives(d1, ratio, np.full(513, o)))
    assert R.limit(4, 0.5) == 9 and R.limit(6, 0.75) == 9 and R.limit(35, 0.8) == 44 and R.limit(4, 0.8) == 6
    assert not R.survives(4, 0.5, 8) and R.survives(4, 0.5, 9) and not R.survives(6, 0.75, 8) and R.survives(600, 0.5, R.NONE)


def test_header_functions_in_a_sanitized_host_program(tmp_path):
    exe = str(tmp_path / "ratio_other_host_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tod_amd", "csrc"),
                    os.path.join(ROOT, "tests", "ratio_other_host_test.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    said = out.stdout.split("\n")[:-1]
    assert said == ["predicate", "limit 0.5", "limit 0.75", "limit 0.8", "limit 1", "limit extremes", "clamp", "ok"]


NEW_CALLS = ("todhip_other_object_min_device", "todhip_ratio_other_apply_device", "todhip_ratio_other_device", "todhip_set_ratio_test_other")


def test_header_declares_the_entry_points_and_states_the_definition():
    """The four calls are a part of include/todhip.h kept in include/todhip_ratio_other.h, which todhip.h includes at its end."""
    main = open(os.path.join(ROOT, "include", "todhip.h")).read()
    assert re.search(r'^#include "todhip_ratio_other.h"$', re.sub(r"/\*.*?\*/", "", main, flags=re.S), flags=re.M)
    text = open(os.path.join(ROOT, "include", "todhip_ratio_other.h")).read()
    comments = " ".join(" ".join(re.findall(r"/\*.*?\*/", text + main, flags=re.S)).replace("*", " ").split())
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(capi.RATIO_OTHER_EXPORTS) == sorted(NEW_CALLS)
    for name in NEW_CALLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in comments
    for said in ("other == NONE || (float)d1 < ratio (float)other", "do not belong to object o", "EVERY word of d_min is written",
                 "A query that fails gets counts[q] = 0", "slots at or behind the old counts[q] are not written",
                 "A query with counts[q] == 0 is left alone", "independent of todhip_set_ratio_test", "The LSH mode does not enter",
                 "the other SELECTED objects", "todhip_set_db_bit_order is honoured", "element-wise minimum over the ranks",
                 "the least integer with (float)d1 < ratio (float)L", "in front of the cross-check", "no launch is added",
                 "the setting does not change", "_set_ratio_test_other", "with no setter of the pipeline's own"):
        assert said in comments, said
    for method in (capi.Context.other_object_min_device, capi.Context.ratio_other_apply_device, capi.Context.ratio_other_device,
                   capi.Context.set_ratio_test_other):
        assert method.__doc__
    # a C99 host gets the calls from either header
    for first in ("todhip.h", "todhip_ratio_other.h"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-",
                        "-fsyntax-only"], check=True, text=True,
                       input='#include "%s"\nint main(void) { return todhip_set_ratio_test_other(0, 0.f) + todhip_version(); }\n' % first)


def test_entry_points_refuse_without_a_device():
    L = capi.lib()
    for name in NEW_CALLS:
        assert hasattr(L, name)
    assert L.todhip_other_object_min_device(None, 1, 1, 1, None, 0, 1) == capi.EINVAL
    assert L.todhip_ratio_other_apply_device(None, 0.8, 1, 1, 1, 1, 1) == capi.EINVAL
    assert L.todhip_ratio_other_device(None, 1, 1, 0.8, 1, 1, 1) == capi.EINVAL
    assert L.todhip_set_ratio_test_other(None, 0.8) == capi.EINVAL


@pytest.mark.parametrize("width", RC.WIDTHS)
def test_gpu_inputs_are_not_vacuous(width):
    db = RC.make_db(width)
    q = RC.make_queries(width, 1100)
    bits = 8 * width
    counts, m, D = RC.search_ref(db, q, 2, 35)
    obj = R.row_objects(db["off"])
    assert (counts > 0).all() and (counts == 2).any()
    excl, _ = R.limits_of(counts, m, 2, 0.8)
    o = R.other(D, db["off"], excl)
    # the planted equalities
    d1 = m.reshape(-1, 2)[:, 0]["distance"]
    assert (d1[0], o[0], excl[0]) == (4, 8, 2) and (d1[1], o[1], excl[1]) == (4, 9, 2) and (d1[2], o[2], excl[2]) == (6, 8, 5)
    assert not R.survives(4, 0.5, o[0]) and R.survives(4, 0.5, o[1]) and not R.survives(6, 0.75, o[2])
    # the other-object neighbour IS the confuser at lo - 1 / hi, and a nearer row of the query's own object (the duplicates at lo and
    # hi - 1 among them) exists and does not count
    off = db["off"].astype(np.int64)
    at_edge = strictly = 0
    for i in range(1100):
        rows = np.nonzero((D[i] == o[i]) & (obj != excl[i]))[0]
        assert len(rows) >= 1
        lo, hi = off[excl[i]], off[excl[i] + 1]
        if (rows == lo - 1).any() or (rows == hi).any():
            at_edge += 1
            own = D[i][lo:hi]
            assert own.min() == d1[i] and own.min() <= o[i]
            home = i % 10 < 9 and RC.CLUSTERS[i % 10][0] == excl[i]    # (not: a confuser is the nearest row, by an exact tie)
            if home and i % 10 in (0, 2, 4, 6):                  # clusters at an object's first row
                assert D[i][lo] <= o[i]
                strictly += D[i][lo] < o[i]
            if home and i % 10 in (1, 3, 5):                     # ... and at its last
                assert D[i][hi - 1] <= o[i]
                strictly += D[i][hi - 1] < o[i]
    assert at_edge > 400 and strictly > 300
    assert (excl == 1).sum() > 50                                 # queries whose nearest row is the 1-row object
    assert (o > bits // 4).any() and (o <= 12).any()              # others far away (no confuser) and close
    # every ratio drops some and keeps some; the classic test is another filter
    for ratio in RC.RATIOS:
        got = R.ratio_other(counts, m, 2, ratio, D, db["off"])
        assert got["dropped"] >= 10 and got["kept"] >= 10, ratio
        classic = R.classic_ratio_keeps(D, ratio)
        # (at 1.0 both drop exactly the ties between the two nearest rows, which here are ties between two objects)
        assert ratio == 1.0 or (classic != (got["counts"] > 0)).sum() >= 10, ratio
    # limits on both sides of the truth change the primitive's answer exactly where they are below it
    exact = R.other(D, db["off"], excl)
    lim = np.where(np.arange(1100) % 2 == 0, exact + 3, np.maximum(exact, 2) - 2).astype(np.uint32)
    got = R.other_min(D, db["off"], excl, lim)
    assert np.array_equal(got, np.minimum(exact, lim)) and (got < exact).any() and (got == exact).any()
    # a single-object DB: everything survives
    one = RC.single_object_db(width)
    q1 = RC.make_queries(width, 70)
    D1 = R.hamming(q1, one["desc"])
    assert (R.other(D1, one["off"], np.zeros(70, np.int64)) == R.NONE).all()
