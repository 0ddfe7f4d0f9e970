"""What can be said about the 64-byte matcher without a GPU: its definition (a numpy statement against the oracle, which is what the
GPU tests hold the kernels to), its documentation, the registers of its kernel, and the adapter's width checks."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import adapter_wide_build
import match_wide_ref as W
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = ("queryIdx", "trainIdx", "imgIdx", "distance")


@pytest.fixture(scope="module")
def db():
    return W.WideDb()


def test_planted_queries_cover_both_halves_the_complement_and_the_last_bit(db):
    n, d = sum(W.ROWS), W.distances(db.desc, db.q[:4]).astype(np.int64)
    lo, hi = W.distances(db.desc[:, :32], db.q[:4, :32]).astype(np.int64), W.distances(db.desc[:, 32:], db.q[:4, 32:]).astype(np.int64)
    assert (lo[0, n - 100], hi[0, n - 100]) == (0, 3) and (lo[1, n - 101], hi[1, n - 101]) == (3, 0)
    assert d[2, n - 102] == 512 and (d[3, n - 7], d[3, n - 300]) == (0, 1)
    assert db.desc[n - 7, 63] ^ db.desc[n - 300, 63] == 0x80 and np.array_equal(db.desc[n - 7, :63], db.desc[n - 300, :63])
    # random 512-bit rows are far apart: without the planted rows nothing would be inside any sensible radius
    assert d[2].min() > 150


@pytest.mark.parametrize("ratio", [0.0, 0.8])
@pytest.mark.parametrize("k", [1, 2, 5, 8])
def test_numpy_definition_equals_the_oracle_at_64_bytes(db, k, ratio):
    for radius in (1, 35, 255, 256, 257, 511, 512, 1000):
        rc, rp, m, xyz = O.match(db.desc, db.off, db.pts, db.q, k, radius, ratio)
        w_rp, w_m, w_xyz = W.match(db.desc, db.off, db.pts, db.q, k, radius, ratio)
        assert rc == 0 and np.array_equal(rp, w_rp) and np.array_equal(xyz, w_xyz), (k, radius, ratio)
        for f in FIELDS:
            assert np.array_equal(m[f], w_m[f]), (k, radius, ratio, f)
        if radius >= 512 and ratio == 0.0:
            assert (np.diff(rp.astype(np.int64)) == k).all()


def test_header_and_binding_document_the_64_byte_db():
    h = open(os.path.join(ROOT, "include", "todhip.h")).read()
    assert "desc_bytes == 64" in h and "todhip_db_desc_bytes" in h
    for word in ("zero-padding", "0 ... 512", "radius >= 512", "todhip_set_matcher_block_split are accepted and have no effect",
                 "todhip_match_radius[_device], todhip_match_l2[_device]", "todhip_set_lsh is enabled", "todhip_pipeline_db_load[_device]"):
        assert word in h, word
    from tod_amd import capi
    assert "u8[N,64]" in capi.Context.db_load.__doc__
    for fn in (capi.Context.match, capi.Context.match_device):
        assert "query width must equal the DB's" in fn.__doc__, fn.__name__
    assert "todhip_db_desc_bytes" in capi.EXPORTS


def test_wide_kernel_stays_two_waves_per_simd_without_scratch():
    """hamming_topk_wide (tod_amd/csrc/match_wide.hip) is launched under __launch_bounds__(kBlock, 2): every instantiation -- k = 1..8,
    two query blocks per wave, four up to k = 3, each with the integer and the float block test -- must stay inside 256 registers
    and use no scratch. Read from the kernel metadata of the generated code (same compiler, same flags as the Makefile)."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    with tempfile.TemporaryDirectory() as d:
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-c", "--cuda-device-only", "-save-temps",
                        "-o", os.path.join(d, "match_wide.o"), os.path.join(ROOT, "tod_amd", "csrc", "match_wide.hip")], check=True,
                       stderr=subprocess.DEVNULL, cwd=d)
        asm = [f for f in os.listdir(d) if f.endswith(".s")]
        assert len(asm) == 1, asm
        text = open(os.path.join(d, asm[0])).read()
    seen = set()
    for m in re.finditer(r"\.name:\s+(\S*hamming_topk_wideILi(\d)ELi(\d)ELb([01])E\S*)", text):
        blk = text[m.start():m.start() + 1500]
        vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
        k, qt, imax = int(m.group(2)), int(m.group(3)), int(m.group(4))
        assert vgpr <= 256 and scratch == 0, "hamming_topk_wide<%d, %d, %d>: %d registers, %d bytes of scratch" % (k, qt, imax, vgpr, scratch)
        seen.add((k, qt, imax))
    want = {(k, 2, i) for k in range(1, 9) for i in (0, 1)} | {(k, 4, i) for k in (1, 2, 3) for i in (0, 1)}
    assert seen == want, sorted(seen ^ want)


def test_adapter_declares_and_refuses_mixed_or_unknown_widths():
    """declare-only: the cell compiles against the test double and declares the reference's names; cpu: load_models throws, naming
    the object, on documents of mixed widths, of 48 columns and of a type that is not CV_8U -- before the library is asked"""
    exe = adapter_wide_build.build()
    out = subprocess.run([exe, tempfile.gettempdir(), "declare-only"], capture_output=True, text=True)
    assert out.returncode == 0 and "declare ok" in out.stdout, out.stderr
    out = subprocess.run([exe, tempfile.gettempdir(), "cpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "cpu ok" in out.stdout, out.stdout + out.stderr
