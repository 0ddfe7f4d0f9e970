"""The float matcher's two filters without a GPU: the numpy definitions (tests/l2_filters_ref.py) against plain-loop statements; the
inputs of tests/test_l2_filters_gpu.py pinned on the reference alone, so that the GPU tests cannot pass vacuously; the predicates
(tod_amd/csrc/l2_filters.h, cross_check.h on d2 bits) in a stand-alone host program built with -fsanitize=address,undefined; what
the header and the binding declare and say; and the registers of the new kernel."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import cross_check_ref as R
import l2_filters_cases as LC
import l2_filters_ref as F
import l2_radius_cases as RC
from match_l2_radius_ref import d2
from tod_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


# ------------------------------------------------------------------------------------------------ the definitions against the loops
def toy():
    """3 frames of Q = 4 over 10 queries (the last frame is short), a 12-row DB of 8 dimensions in 3 objects, stride 3"""
    rng = np.random.Generator(np.random.PCG64(5))
    db = rng.integers(0, 9, (12, 8)).astype(np.float32)
    off = np.array([0, 5, 6, 12], np.uint32)
    q = np.stack([db[r] + rng.integers(-n, n + 1, 8) for r, n in ((2, 1), (2, 3), (2, 1), (7, 0), (2, 2), (7, 2), (7, 2), (11, 3), (2, 4), (2, 4))])
    q = q.astype(np.float32)
    q[9] = q[8]                                                  # byte-identical queries: the index decides
    nq, stride = len(q), 3
    counts, m, _ = F.ratio_filter(d2(db, q), stride, 1e9, 0.0, off)
    counts = np.minimum(counts, np.array([3, 2, 3, 1, 0, 3, 3, 2, 3, 3], np.uint32))
    xyz = np.arange(nq * stride * 3, dtype=np.float32).reshape(-1, 3)
    return counts, m, xyz, q, db, off, 4, stride


@pytest.mark.parametrize("frame_nq", [None, [4, 4, 2], [4, 0, 1], [9, 2, 0]])
def test_cross_check_definition_equals_the_loops(frame_nq):
    counts, m, xyz, q, db, off, Q, stride = toy()
    got = F.cross_check_l2(counts, m, xyz, q, db, off, Q, stride, frame_nq)
    keep = np.array(F.cross_check_l2_loops(counts, m, q, db, off, Q, stride, frame_nq)).reshape(-1)
    assert np.array_equal(got["keep"], keep)
    assert 0 < got["removed"] < got["total"] == int(counts.sum())
    if frame_nq is None:
        assert got["tie_decided"] > 0 and got["counts"][9] < got["counts"][8]
    again = F.cross_check_l2(got["counts"], got["matches"], got["xyz"], q, db, off, Q, stride, frame_nq)
    assert again["removed"] == 0 and np.array_equal(again["counts"], got["counts"]) and np.array_equal(again["matches"], got["matches"])


def test_ratio_definition_equals_the_loops():
    db, q = LC.ratio_planted()
    dd = d2(db["desc"], q)
    for ratio in (0.5, 0.8, 1.0):
        assert list(F.ratio_passes(dd, ratio)) == F.ratio_passes_loops(db["desc"], q, ratio)
    rng = np.random.Generator(np.random.PCG64(17))
    desc = rng.integers(0, 6, (9, 128)).astype(np.float32)       # small integers: many equal distances
    qq = rng.integers(0, 6, (12, 128)).astype(np.float32)
    for ratio in (0.5, 0.97, 1.0):
        got = F.ratio_passes(d2(desc, qq), ratio)
        assert list(got) == F.ratio_passes_loops(desc, qq, ratio)
    assert F.ratio_passes(d2(desc[:1], qq), 0.5).all() and all(F.ratio_passes_loops(desc[:1], qq[:2], 0.5))      # a one-row DB passes


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs, pinned
def _stats(q, Q, stride, frame_nq=None):
    db = LC.make_db()
    counts, m, xyz = LC.search_ref(db, q, stride, LC.RADIUS)
    return F.cross_check_l2(counts, m, xyz, q, db["desc"], db["off"], Q, stride, frame_nq), counts


def test_db_is_integer_valued_in_range_and_dense_cluster_is_inside_the_radius():
    db = LC.make_db()
    assert db["desc"].shape == (LC.N_ROWS, 128) and np.array_equal(db["desc"], np.round(db["desc"]))
    assert db["desc"].min() >= 20 and db["desc"].max() <= 230 and len(db["dense"]) == LC.DENSE
    dd = d2(db["desc"][db["dense"]], db["desc"][db["dense"]])
    assert np.sqrt(dd.max()) < LC.RADIUS


def test_single_frames_are_not_vacuous():
    for Q in LC.SINGLE_FRAMES:
        q = LC.make_queries(Q)
        if Q >= 33:
            assert np.array_equal(q[0], q[Q - 1])
        for k in LC.KS:
            got, counts = _stats(q, Q, k)
            if Q == 1:
                assert got["removed"] == 0 < got["total"]            # (one query: by the definition nothing can go)
                continue
            assert 0 < got["removed"] < got["total"], (Q, k)
            if Q >= 33:
                assert got["tie_decided"] > 0, (Q, k)
            if Q == 2:
                assert got["tie_decided"] == 0
            if k >= 2:
                assert (counts >= min(k, 6)).any()


def test_three_frames_are_not_vacuous():
    f3 = LC.FRAMES3
    q = LC.make_frames3()
    db = LC.make_db()
    assert np.array_equal(q[:7], q[66:73])
    for k in (1, 5):
        got, counts = _stats(q, f3["Q"], k, f3["frame_nq"])
        assert 0 < got["removed"] < got["total"] and got["tie_decided"] > 0
        alone, _ = _stats(q[:7], 7, k)                               # frame 2's valid queries as a frame of their own
        assert np.array_equal(alone["counts"], got["counts"][66:73]) and got["counts"][66:73].sum() > 0
        assert counts[33:66].sum() == 33 * k and got["counts"][33:66].sum() == 0     # frame 1's 33 / 165 matches all go
        assert counts[73:80].min() > 0 and got["counts"][73:99].sum() == 0
        unfiltered = LC.search_ref(db, q, k, LC.RADIUS)
        every = F.cross_check_l2(*unfiltered, q, db["desc"], db["off"], 33, k)
        assert not np.array_equal(every["counts"][66:73], got["counts"][66:73])      # a filter that ignored frame_nq gives another result
        whole = F.cross_check_l2(*unfiltered, q, db["desc"], db["off"], 99, k)
        assert not np.array_equal(whole["counts"][66:73], got["counts"][66:73])      # and so does one that let frames compete


def test_radius_strides_and_seventy_frames_are_not_vacuous():
    q = LC.make_queries(70)
    got64, counts64 = _stats(q, 70, 64)
    assert (counts64 == 64).any() and 0 < got64["removed"] < got64["total"]
    got, counts = _stats(q, 70, 1024)
    assert 64 < counts.max() <= LC.DENSE and 0 < got["removed"] < got["total"] and got["tie_decided"] > 0
    keep = got["keep"].reshape(70, 1024)
    assert any(keep[i, :64].any() and keep[i, 64:counts[i]].any() and not keep[i, :64].all() and not keep[i, 64:counts[i]].all()
               for i in np.nonzero(counts > 64)[0])
    q70, frame_nq = LC.make_frames70()
    assert R.n_frames(len(q70), 2) == 70 > 64                        # more frames than travel as a kernel argument
    got, counts = _stats(q70, 2, 2, frame_nq)
    assert got["total"] == 280 and 0 < got["removed"] < got["total"] and got["tie_decided"] > 0
    assert got["counts"][71::2].sum() == 0 and got["counts"][1:70:2].sum() > 0      # the second query of a frame behind frame_nq = 1


def test_order_frame_separates_the_summation_orders():
    db, q = LC.order_frame()
    counts, m, xyz = LC.search_ref(db, q, 1, 1e9)
    assert np.array_equal(m["trainIdx"], np.repeat(np.arange(40), 2))                # each pair names its own row
    seq = F.cross_check_l2(counts, m, xyz, q, db["desc"], db["off"], 80, 1)
    assert seq["removed"] == 40 and seq["tie_decided"] < 80                          # one of each pair goes
    winners = seq["counts"].reshape(40, 2)[:, 0]
    for other in (LC.pairwise_bits, LC.float64_bits):
        alt = F.cross_check_l2(counts, m, xyz, q, db["desc"], db["off"], 80, 1, dist=other)
        assert (alt["counts"].reshape(40, 2)[:, 0] != winners).sum() >= 5            # the input separates the definitions


def test_early_exit_trap_in_the_reference():
    db, q, at = LC.trap()
    counts, m, xyz = LC.search_ref(db, q, 1, 1e9)
    dd = d2(db["desc"][:1], q[list(at)])
    assert (dd == 49.0).all() and all(m["imgIdx"][i] == 0 for i in at)
    got = F.cross_check_l2(counts, m, xyz, q, db["desc"], db["off"], len(q), 1)
    assert [int(got["counts"][i]) for i in at] == [1, 0, 0] and got["tie_decided"] >= 3
    assert 0 < got["removed"] < got["total"]


def test_ratio_inputs_are_not_vacuous():
    big = RC.Db(nq=70)
    dd = d2(big.desc, big.q)
    assert [int(F.ratio_passes(dd, r).sum()) for r in (0.5, 0.8, 1.0)] == [60, 60, 70]
    db, q = LC.ratio_planted()
    dd = d2(db["desc"], q)
    for col, ratio in enumerate((0.5, 0.8, 1.0)):
        want = [LC.RATIO_WANT[name][col] for name in LC.RATIO_SCENARIOS]
        assert list(F.ratio_passes(dd, ratio)) == want, ratio
        counts, _, _ = F.ratio_filter(dd, 2, LC.RATIO_RADIUS, ratio, db["off"])
        assert [c > 0 for c in counts] == want
    s = LC.RATIO_SCENARIOS.index("second_beyond_radius_passes")
    assert F.ratio_filter(dd, 2, LC.RATIO_RADIUS, 0.5, db["off"])[0][s] == 1        # the radius cut applies to the survivors
    s = LC.RATIO_SCENARIOS.index("second_beyond_radius_fails")
    assert F.ratio_filter(dd, 2, LC.RATIO_RADIUS, 0.0, db["off"])[0][s] == 1 and F.ratio_filter(dd, 2, LC.RATIO_RADIUS, 0.8, db["off"])[0][s] == 0


# ------------------------------------------------------------------------------------------------ the predicates, the header, the build
def test_predicates_in_a_sanitized_host_program(tmp_path):
    exe = str(tmp_path / "l2_filters_host_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tod_amd", "csrc"),
                    os.path.join(ROOT, "tests", "l2_filters_host_test.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    assert out.stdout.split("\n")[:-1] == ["domain", "predicate", "keys", "bits", "trap", "ok"]


def test_header_declares_the_entry_points_and_states_the_definitions():
    text = open(os.path.join(ROOT, "include", "todhip.h")).read()
    comments = " ".join(" ".join(re.findall(r"/\*.*?\*/", text, flags=re.S)).replace("*", " ").split())
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("todhip_set_l2_ratio_test", "todhip_cross_check_l2_device", "todhip_set_l2_cross_check"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in capi.EXPORTS
    for said in ("keeps its matches iff dist1 < ratio", "one binary32 product", "with one row passes", "Two rows at equal distance fail even at ratio 1",
                 "The radius cut applies to the survivors", "k == 1 searches two rows internally and returns one",
                 "TODHIP_EINVAL for k < 2 while it is on", "and their merges ignore it, as the Hamming radius forms ignore todhip_set_ratio_test",
                 "todhip_set_ratio_test and todhip_set_cross_check do not apply to the float forms",
                 "crossCheck = true", "the IEEE binary32 bits of d2(q, row g)", "not taken from DMatch.distance",
                 "frame_nq is copied before the call returns", "idempotent", "a query outside V(f) ends with counts[q] = 0",
                 "behind the ratio test and the radius cut", "The shard, merge and radius entry points of the float forms ignore it"):
        assert said in comments, said
    for method in (capi.Context.set_l2_ratio_test, capi.Context.cross_check_l2_device, capi.Context.set_l2_cross_check):
        assert method.__doc__
    from tod_amd import sharded
    assert "set_l2_ratio_test" in sharded.GpuOps.__doc__


def test_entry_points_refuse_a_null_context():
    L = capi.lib()
    assert hasattr(L, "todhip_cross_check_l2_device")
    assert L.todhip_cross_check_l2_device(None, 1, 1, 1, None, 1, 1, 1, 1) == capi.EINVAL
    assert L.todhip_set_l2_cross_check(None, 4) == capi.EINVAL
    assert L.todhip_set_l2_ratio_test(None, 0.5) == capi.EINVAL


def test_float_test_kernel_holds_its_row_in_registers_two_waves_per_simd():
    """cross_check_l2_test_kernel (tod_amd/csrc/cross_check_l2.hip) keeps a 128-float DB row per lane: no scratch, at most 256
    registers, two waves per SIMD -- what DESIGN 6o claims. From the compiler's own report, same flags as the Makefile."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    make = open(os.path.join(ROOT, "tod_amd", "csrc", "Makefile")).read()
    assert re.search(r"^cross_check_l2\.o: CXXFLAGS \+= -fno-slp-vectorize$", make, flags=re.M)
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-slp-vectorize", "-c",
                              "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", os.path.join(d, "x.o"),
                              os.path.join(ROOT, "tod_amd", "csrc", "cross_check_l2.hip")], check=True, capture_output=True, text=True, cwd=d)
    blocks = re.split(r"remark: Function Name: ", out.stderr)[1:]
    mine = [b for b in blocks if "cross_check_l2_test_kernel" in b.split("\n")[0]]
    assert len(mine) == 1, [b.split("\n")[0] for b in blocks]

    def number(what):
        return int(re.search(re.escape(what) + r":? (\d+)", mine[0]).group(1))
    assert number("ScratchSize [bytes/lane]") == 0 and number("VGPRs Spill") == 0
    assert 128 < number("VGPRs") + number("AGPRs") <= 256 and number("Occupancy [waves/SIMD]") == 2
    assert number("LDS Size [bytes/block]") <= 32 * 1024                             # two blocks of a CU beside each other
