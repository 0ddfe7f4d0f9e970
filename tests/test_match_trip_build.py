"""Build-time check of the paired split-2 trip of hamming_topk_fp4rows (tod_amd/csrc/match_fp4rows.h; no GPU needed: hipcc
cross-compiles). The loop is bound by vector issue, about 4 cycles per vector instruction ("What bounds the split-block
kernel"), so an instruction on the path that every block but one in two thousand takes is paid in full -- and hipcc adds such
instructions silently: state kept across the loop for a rare path came back as ten v_mov_b32 at every back edge, behind the point
where an earlier count had stopped. tools/k4x_trip_counts.py walks the main loop's fall-through path from its header to the back
branch; a pair's useful work is 4 MFMAs and 9 vector instructions (7 v_or3, v_bitop3, v_cmp)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import k4x_trip_counts as T

FORMS = ((2, 6, 2), (5, 6, 2), (2, 4, 2))


@pytest.fixture(scope="module")
def match_asm():
    if not os.path.exists(T.HIPCC):
        pytest.skip("hipcc not installed")
    return T.compile_asm()


@pytest.mark.parametrize("form", FORMS, ids=lambda f: "k%d_qt%d_mode%d" % f)
def test_paired_trip_carries_only_its_own_work(match_asm, form):
    k, qt, mode = form
    r = T.trip_counts(match_asm, k, qt, mode)
    print(r)
    assert r["pairs"] == qt and r["mfma"] == 4 * qt, r       # two row steps of qt / 2 pairs: the walk found the main loop
    assert r["buffer_loads"] == 4, r                          # two fragments for each of the two steps, nothing else
    assert r["v_mov_b32"] == 0, r
    assert r["valu"] <= 9 * r["pairs"], r
    assert r["scratch_bytes"] == 0, r
    if form == (2, 6, 2):
        # registers are allocated in eights: one step under the 214 of the form that exchanged bounds in the loop (it builds at 196)
        assert r["vgprs"] <= 208, r
