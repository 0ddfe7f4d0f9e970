"""Build-time checks on the registers of the hypothesis kernel and of the DB pass it runs beside (no GPU needed: hipcc cross-compiles),
beside tests/test_build_checks.py.

Two waves of the headline's DB pass, hamming_topk_fp4rows<2, 6, 2>, hold 2 x 200 of a SIMD's 512 registers. eval_kernel<false, ...>,
one 64-lane workgroup per hypothesis that lives for hundreds of microseconds, starts beside them only if its own allocation
(vgpr_count + agpr_count rounded up to 8) fits the 112 that are left; otherwise it waits for a matcher wave to retire and keeps
that SIMD at one matcher wave for as long as it lives (DESIGN, "What would come next", item 0'; profiles/verify_regs.json)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
FILE_REGS, PASS_MAX = 512, 200
ROOM = FILE_REGS - 2 * PASS_MAX          # 112


def kernels_of(source):
    """{mangled name: metadata entry} of every kernel of a .hip file compiled to gfx950 assembly (same compiler, same flags as the Makefile)"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    asm = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                          "-o", "-", os.path.join(ROOT, "tod_amd", "csrc", source)], check=True, capture_output=True, text=True).stdout
    meta = asm[asm.index("amdhsa.kernels:"):]
    out = {}
    for e in re.split(r"\n  - ", meta)[1:]:
        m = re.search(r"\n    \.name:\s+(\S+)", e)         # (the kernel's own name, not an argument's)
        if m and ".vgpr_count:" in e:
            out[m.group(1)] = e
    return out


@pytest.fixture(scope="module")
def verify_kernels():
    return kernels_of("verify.hip")


@pytest.fixture(scope="module")
def match_kernels():
    return kernels_of("match.hip")


def field(entry, key):
    return int(re.search(r"\.%s:\s+(\d+)" % key, entry).group(1))


def allocation(entry):
    return -(-(field(entry, "vgpr_count") + field(entry, "agpr_count")) // 8) * 8


def test_the_hypothesis_kernel_fits_beside_two_waves_of_the_db_pass(verify_kernels):
    """every eval_kernel<false, ...>: both ways of passing the argument sets, the first pass and the deferred one"""
    seen = []
    for name, e in verify_kernels.items():
        if "eval_kernelILb0E" not in name:
            continue
        seen.append(name)
        regs, scratch = field(e, "vgpr_count") + field(e, "agpr_count"), field(e, "private_segment_fixed_size")
        assert regs <= ROOM and allocation(e) <= ROOM and scratch == 0, "%s: %d registers, %d bytes of scratch" % (name, regs, scratch)
        assert field(e, "vgpr_spill_count") == 0
    assert len(seen) == 4 and sum("SlotsPtr" in n for n in seen) == 2, seen


def test_the_db_pass_leaves_the_room_the_hypothesis_kernel_relies_on(match_kernels):
    seen = [e for name, e in match_kernels.items() if "hamming_topk_fp4rowsILi2ELi6ELi2EE" in name]
    assert len(seen) == 1
    regs, scratch = field(seen[0], "vgpr_count") + field(seen[0], "agpr_count"), field(seen[0], "private_segment_fixed_size")
    assert regs <= PASS_MAX and scratch == 0, "hamming_topk_fp4rows<2, 6, 2>: %d registers, %d bytes of scratch" % (regs, scratch)
