"""Build-time checks on fast_nms_kernel's generated gfx950 code (no GPU needed: hipcc cross-compiles), beside tests/test_orb_build_checks.py.

The kernel runs beside the matcher's two waves per SIMD, so what it may take is fixed: no more registers than before its suppression
moved to the survivor list (58), no more LDS than its five arrays took then (9888 bytes: the scores, the staged pixels, the list, the
histogram and the list's length), and no scratch."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
MAX_VGPR, MAX_LDS_BYTES = 58, 9888


@pytest.fixture(scope="module")
def fast_nms():
    """fast_nms_kernel's metadata block and text, from orb.hip compiled to gfx950 assembly (same compiler, same flags as the Makefile)"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                          "-o", "-", os.path.join(ROOT, "tod_amd", "csrc", "orb.hip")], check=True, capture_output=True, text=True)
    asm = out.stdout
    body = re.search(r"^(_Z\S*fast_nms_kernel\S*):[^\n]*\n(.*?)\n\.Lfunc_end", asm, re.S | re.M)
    meta = next(e for e in re.split(r"\n  - ", asm[asm.index("amdhsa.kernels:"):]) if re.search(r"\.name:\s+%s\b" % re.escape(body.group(1)), e))
    return meta, body.group(2)


def field(entry, key):
    return int(re.search(r"\.%s:\s+(\d+)" % key, entry).group(1))


def test_registers_lds_and_scratch_stay_within_what_the_kernel_took(fast_nms):
    meta, _ = fast_nms
    vgpr, lds, scratch = field(meta, "vgpr_count"), field(meta, "group_segment_fixed_size"), field(meta, "private_segment_fixed_size")
    assert vgpr <= MAX_VGPR and lds <= MAX_LDS_BYTES and scratch == 0, "%d registers, %d bytes of LDS, %d bytes of scratch" % (vgpr, lds, scratch)
    assert field(meta, "vgpr_spill_count") == 0 and field(meta, "sgpr_spill_count") == 0


def test_the_score_runs_on_packed_pairs(fast_nms):
    """pass 2 is one sliding minimum and one sliding maximum on 16-bit pairs; a swap of a pair's halves is an operand selector, not an
    instruction of its own"""
    _, text = fast_nms
    ins = [l.split(";")[0].split() for l in text.split("\n") if l.startswith("\t")]
    n_min = sum(1 for i in ins if i and i[0] == "v_pk_min_i16")
    n_max = sum(1 for i in ins if i and i[0] == "v_pk_max_i16")
    # each polarity: windows of 2, 4, 8 and 9 elements over 8 pairs, and 7 to fold the 8 results
    assert n_min == n_max == 4 * 8 + 7, (n_min, n_max)
