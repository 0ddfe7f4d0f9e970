"""Build-time checks on stage A's generated gfx950 code (no GPU needed: hipcc cross-compiles), modelled on tests/test_build_checks.py.

The matcher's DB pass runs two waves per SIMD at <= 224 registers so that ORB's waves fit into the same SIMDs
(test_build_checks.py: test_k4x_waves_leave_room_in_the_register_file): 512 - 2 x 224 = 64 registers are what is left for them.
A kernel of orb.hip that grows beyond 64 registers, spills, or takes more than 16 KB of LDS per block no longer starts beside the
matcher, and the pipeline loses that silently -- only the generated code can tell."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def orb_kernels():
    """{kernel name: its metadata block} of orb.hip compiled to gfx950 assembly (same compiler, same flags as the Makefile)"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "orb.s")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-o", out, os.path.join(ROOT, "tod_amd", "csrc", "orb.hip")], check=True, stderr=subprocess.DEVNULL)
        asm = open(out).read()
    kernels = {}
    for entry in re.split(r"\n  - ", asm[asm.index("amdhsa.kernels:"):])[1:]:   # one list item per kernel, then other lists
        name = re.search(r"\.name:\s+(\S+)", entry)
        if name is None:
            continue
        name = name.group(1)
        kernels[re.search(r"\d+([a-z_0-9]+_kernel)", name).group(1)] = entry
    return kernels


def field(entry, key):
    return int(re.search(r"\.%s:\s+(\d+)" % key, entry).group(1))


def test_every_kernel_fits_beside_the_matcher(orb_kernels):
    assert {"fast_nms_kernel", "blur_kernel", "resize_kernel", "describe_kernel", "harris_kernel", "rank_tiled_kernel"} <= set(orb_kernels)
    for name, entry in sorted(orb_kernels.items()):
        vgpr, scratch, lds = field(entry, "vgpr_count"), field(entry, "private_segment_fixed_size"), field(entry, "group_segment_fixed_size")
        assert vgpr <= 64 and scratch == 0 and lds <= 16384, "%s: %d registers, %d bytes of scratch, %d bytes of LDS" % (name, vgpr, scratch, lds)


def test_the_blur_is_one_kernel(orb_kernels):
    assert "blur_kernel" in orb_kernels
    assert "blur_h_kernel" not in orb_kernels and "blur_v_kernel" not in orb_kernels
