"""The cross-check filter without a GPU: the numpy definition (tests/cross_check_ref.py) against a triple-loop statement; the one
statement of the predicate (tod_amd/csrc/cross_check.h) in a stand-alone host program built with -fsanitize=address,undefined; what the
header declares and says; and the inputs of tests/test_cross_check_gpu.py pinned on the reference alone, so that the GPU test cannot
pass vacuously: in every case the filter removes some matches and keeps some, and the index tie decides at least one.

One shape is exempt by the definition itself: a single frame of Q = 1 holds one query, which is the nearest valid query to every row
it names, so nothing can be removed there (asserted as such)."""
import os
import re
import subprocess

import numpy as np
import pytest

import cross_check_cases as CC
import cross_check_ref as R
from tod_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def toy():
    """3 frames of Q = 4 over 10 queries (the last frame is short), a 12-row DB in 3 objects, stride 3."""
    rng = np.random.Generator(np.random.PCG64(5))
    db = rng.integers(0, 256, (12, 32), dtype=np.uint8)
    off = np.array([0, 5, 6, 12], np.uint32)
    q = np.stack([CC.flipped(db[r], rng, n) for r, n in ((2, 1), (2, 4), (2, 1), (7, 0), (2, 2), (7, 3), (7, 3), (11, 5), (2, 9), (2, 9))])
    q[9] = q[8]                                                  # byte-identical queries: the index decides
    nq, stride = len(q), 3
    D = R.hamming(q, db)
    m = np.zeros(nq * stride, capi.DMATCH_DTYPE)
    counts = np.array([3, 2, 3, 1, 0, 3, 3, 2, 3, 3], np.uint32)
    for i in range(nq):
        order = np.lexsort((np.arange(12), D[i]))[:stride]
        obj = np.searchsorted(off.astype(np.int64), order, side="right") - 1
        s = slice(i * stride, (i + 1) * stride)
        m["queryIdx"][s], m["trainIdx"][s], m["imgIdx"][s], m["distance"][s] = i, order - off[obj], obj, D[i][order]
    xyz = np.arange(nq * stride * 3, dtype=np.float32).reshape(-1, 3)
    return counts, m, xyz, q, db, off, 4, stride


@pytest.mark.parametrize("frame_nq", [None, [4, 4, 2], [4, 0, 1], [9, 2, 0]])
def test_numpy_definition_equals_the_loops(frame_nq):
    counts, m, xyz, q, db, off, Q, stride = toy()
    got = R.cross_check(counts, m, xyz, q, db, off, Q, stride, frame_nq)
    keep = np.array(R.cross_check_loops(counts, m, q, db, off, Q, stride, frame_nq)).reshape(-1)
    assert np.array_equal(got["keep"], keep)
    assert 0 < got["removed"] < got["total"] == int(counts.sum())
    nq = len(counts)
    for i in range(nq):                                          # the compaction: survivors in order at the front, xyz beside them
        idx = [j for j in range(stride) if keep[i * stride + j]]
        assert got["counts"][i] == len(idx)
        for pos, j in enumerate(idx):
            assert got["matches"][i * stride + pos] == m[i * stride + j]
            assert np.array_equal(got["xyz"][i * stride + pos], xyz[i * stride + j])
        lo, hi = R.valid_range(i // Q, nq, Q, frame_nq)
        assert lo <= i < hi or got["counts"][i] == 0
    if frame_nq is None:
        assert got["tie_decided"] > 0 and got["counts"][9] < got["counts"][8]      # the identical pair: the lower index keeps the rows
    # idempotent
    again = R.cross_check(got["counts"], got["matches"], got["xyz"], q, db, off, Q, stride, frame_nq)
    assert again["removed"] == 0 and np.array_equal(again["counts"], got["counts"]) and np.array_equal(again["matches"], got["matches"])


def test_header_predicate_in_a_sanitized_host_program(tmp_path):
    exe = str(tmp_path / "cross_check_host_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tod_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cross_check_host_test.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    said = out.stdout.split("\n")[:-1]
    assert said[-1] == "ok" and said[-2] == "ties" and len([s for s in said if s.startswith("ranges ")]) == 15


def test_header_declares_the_entry_points_and_states_the_definition():
    text = open(os.path.join(ROOT, "include", "todhip.h")).read()
    comments = " ".join(" ".join(re.findall(r"/\*.*?\*/", text, flags=re.S)).replace("*", " ").split())
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("todhip_cross_check_device", "todhip_set_cross_check", "todhip_pipeline_set_cross_check"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in capi.EXPORTS
    for said in ("crossCheck = true", "obj_off[imgIdx] + trainIdx", "ties to the lower query index", "frame_nq is copied before the call returns",
                 "idempotent", "A query outside V(f) ends with counts[q] = 0", "slots at or behind the old counts[q] are not written",
                 "Selections (todhip_db_select_objects) and the LSH mode do not enter", "sharded and the radius entry points",
                 "ignore the setting", "TODHIP_EBUSY while a ticket is outstanding", "frame_nq = the step's n_kp"):
        assert said in comments, said
    for method in (capi.Context.cross_check_device, capi.Context.set_cross_check, capi.Pipeline.set_cross_check):
        assert method.__doc__


def test_entry_points_refuse_without_a_device():
    L = capi.lib()
    assert hasattr(L, "todhip_cross_check_device")
    assert L.todhip_cross_check_device(None, 1, 1, 1, None, 1, 1, 1, 1) == capi.EINVAL
    assert L.todhip_set_cross_check(None, 4) == capi.EINVAL
    assert L.todhip_pipeline_set_cross_check(None, 1) == capi.EINVAL


def _case_stats(width, q, Q, stride, frame_nq=None):
    db = CC.make_db(width)
    counts, m, xyz = CC.search_ref(db, q, stride, CC.RADIUS)
    return R.cross_check(counts, m, xyz, q, db["desc"], db["off"], Q, stride, frame_nq), counts


@pytest.mark.parametrize("width", CC.WIDTHS)
def test_gpu_inputs_are_not_vacuous(width):
    ties = 0
    for Q in CC.SINGLE_FRAMES:
        q = CC.make_queries(width, Q)
        if Q >= 33:
            assert np.array_equal(q[0], q[Q - 1])                # two byte-identical queries
        for k in CC.KS:
            got, counts = _case_stats(width, q, Q, k)
            if Q == 1:
                assert got["removed"] == 0 < got["total"]        # (one query: by the definition nothing can go)
                continue
            assert 0 < got["removed"] < got["total"], (width, Q, k)
            ties += got["tie_decided"]
            if k >= 2:
                assert (counts >= min(k, 6)).any()               # lists as long as a cluster of 6 rows allows
    assert ties > 0
    # three frames, frame_nq = [33, 0, 7]: the shared descriptors of frames 0 and 2 end alike, the rows behind frame_nq end empty
    # although they would have won
    f3 = CC.FRAMES3
    q = CC.make_frames3(width)
    assert np.array_equal(q[:7], q[66:73])
    for k in (1, 5):
        got, counts = _case_stats(width, q, f3["Q"], k, f3["frame_nq"])
        assert 0 < got["removed"] < got["total"] and got["tie_decided"] > 0
        alone, _ = _case_stats(width, q[:7], 7, k)               # frame 2's valid queries as a frame of their own
        assert np.array_equal(alone["counts"], got["counts"][66:73]) and got["counts"][66:73].sum() > 0
        assert counts[33:66].sum() > 0 and got["counts"][33:66].sum() == 0
        assert counts[73:80].min() > 0 and got["counts"][73:99].sum() == 0
        every = R.cross_check(*CC.search_ref(CC.make_db(width), q, k, CC.RADIUS), q, CC.make_db(width)["desc"], CC.make_db(width)["off"], 33, k)
        assert not np.array_equal(every["counts"][66:73], got["counts"][66:73])      # a filter that ignored frame_nq gives another result
        whole = R.cross_check(*CC.search_ref(CC.make_db(width), q, k, CC.RADIUS), q, CC.make_db(width)["desc"], CC.make_db(width)["off"], 99, k)
        assert not np.array_equal(whole["counts"][66:73], got["counts"][66:73])      # and so does one that let frames compete


def test_radius_strides_fill_and_exceed_a_compaction_chunk():
    """stride 64: a query whose count equals the stride; stride 1024: one whose count exceeds 64, with survivors and removals on
    both sides of slot 64"""
    q = CC.make_queries(32, 70)
    got64, counts64 = _case_stats(32, q, 70, 64)
    assert (counts64 == 64).any() and 0 < got64["removed"] < got64["total"]
    got, counts = _case_stats(32, q, 70, 1024)
    assert counts.max() > 64 and 0 < got["removed"] < got["total"] and got["tie_decided"] > 0
    keep = got["keep"].reshape(70, 1024)
    big = int(np.argmax(counts))
    assert any(keep[i, :64].any() and keep[i, 64:counts[i]].any() and not keep[i, :counts[i]].all() for i in np.nonzero(counts > 64)[0]), big
