"""Build-time check on the generated gfx950 code of hamming_topk_fp4rows (tod_amd/csrc/match_mfma.h; no GPU needed: hipcc
cross-compiles): the register budget of tests/test_build_checks.py's K4x check, for the DB pass that reads the fp4 copy of the rows."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def test_fp4rows_waves_leave_room_in_the_register_file():
    """The default launch (six query blocks per wave, k <= 2) stays at <= 224 registers per wave and has no scratch, in all four block
    forms: two waves then leave >= 64 of a SIMD's 512 registers free and ORB's and the verifier's kernels start beside the matcher's
    waves, exactly as hamming_topk_mfma's do."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "match.s")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-o", out, os.path.join(ROOT, "tod_amd", "csrc", "match.hip")], check=True, stderr=subprocess.DEVNULL)
        asm = open(out).read()
    seen = 0
    for m in re.finditer(r"\.name:\s+(\S*hamming_topk_fp4rowsILi([12])ELi6ELi([0-3])E\S*)", asm):
        blk = asm[m.start():m.start() + 1500]
        vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
        assert vgpr <= 224 and scratch == 0, "hamming_topk_fp4rows<%s, 6, %s>: %d registers, %d bytes of scratch" % (m.group(2), m.group(3), vgpr, scratch)
        seen += 1
    assert seen == 8, "expected the four block forms of hamming_topk_fp4rows<1 / 2, 6, ...>"
