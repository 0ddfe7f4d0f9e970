"""The float matcher at 64 dimensions (desc_bytes 256) without a GPU: the filter bound against binary64 at this width, the
launch plan at the two widths, the numpy definitions the GPU tests use against the oracle at dim = 64, the compiler's report on the new
kernels, and the header."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import l2_dim64_cases as D
import l2_filters_ref as F
import l2_sharded_ref as S
import match_l2_radius_ref as R
import oracle_lib as O
from tod_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "tod_amd", "csrc")


def _build(src, exe):
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", src), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build("l2_dim64_bound_host_test.cpp", str(tmp_path_factory.mktemp("l2_dim64") / "l2_dim64_bound_host_test"))


# ------------------------------------------------------------------------------------------------------------ the bound
def test_the_bound_holds_at_64_dimensions_with_the_128_wide_constants(exe):
    """|score + |q|^2 - d2| <= eps(q) and the differential form against extended precision, on the worst-case families and seeded
    random cases, the norms summed in l2_prepare_narrow_kernel's order. The largest used fraction of eps is DESIGN 6p's figure."""
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    line = re.compile(r"(worst-case families|random cases): (\d+) pairs, (\d+) ordered row pairs, \(a\) fails (\d+), \(b\) fails (\d+), "
                      r"largest \|error\| / eps ([0-9.]+), largest differential error / 2 eps ([0-9.]+)")
    rows = {m.group(1): m.groups()[1:] for m in map(line.match, out.stdout.splitlines()) if m}
    worst, rnd = rows["worst-case families"], rows["random cases"]
    assert int(worst[0]) == 8820 and int(rnd[0]) == 4800
    assert worst[2:4] == ("0", "0") and rnd[2:4] == ("0", "0")
    assert 0.9 < float(worst[4]) <= 1.0 and 0.9 < float(worst[5]) <= 1.0     # held, and by no unnoticed factor
    assert float(rnd[4]) < float(worst[4])


# ------------------------------------------------------------------------------------------------------------ the plan
def test_plan_at_64_is_the_plan_at_128_with_half_the_query_image(exe, tmp_path):
    out = subprocess.run([exe, "--plan-widths"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    assert int(out.stdout) == 18 * 6 * 8 * 4 * 6                             # tests/l2_plan_host_test.cpp's grid
    # and that program itself, which calls l2_plan without the new argument and knows kDim and kRingSlotBytes, still holds
    old = _build("l2_plan_host_test.cpp", str(tmp_path / "l2_plan_host_test"))
    out = subprocess.run([old], capture_output=True, text=True)
    assert out.returncode == 0 and int(out.stdout) == 18 * 6 * 8 * 4 * 6, out.stdout + out.stderr


# ------------------------------------------------------------------------------------------------------------ the definitions
@pytest.fixture(scope="module")
def small():
    db = D.Db(nq=70)
    return db, R.d2(db.desc, db.q)


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    for f in D.FIELDS:
        assert np.array_equal(got[1][f], want[1][f]), (what, f)
    assert np.array_equal(got[2], want[2]), what


@pytest.mark.parametrize("k", [1, 2, 5, 8])
def test_numpy_definitions_equal_the_oracle_at_64_dimensions(small, k):
    """8 objects of 0 ... 700 rows, 70 queries: the k-NN call is the radius form at max_per_query = k, the keys are l2_knn_keys', the
    ratio filter's k-NN output (ratio off) is l2_match's."""
    db, dd = small
    assert db.desc.shape == (1059, 64) and db.q.shape == (70, 64)
    n_cut = 0
    for radius in D.RADII:
        rc, rp, m, xyz = O.l2_match(db.desc, db.off, db.pts, db.q, k, radius)
        assert rc == 0
        _same(R.match_l2_radius(db.desc, db.off, db.pts, db.q, radius, k, dd)[:3], (rp, m, xyz), (k, radius))
        counts, fm, fx = F.ratio_filter(dd, k, radius, 0.0, db.off, db.pts)
        keep = np.arange(k)[None, :] < counts[:, None].astype(np.int64)
        assert np.array_equal(np.diff(rp.astype(np.int64)), counts) and fm.reshape(-1, k)[keep].tobytes() == m.tobytes()
        assert np.array_equal(fx.reshape(-1, k, 3)[keep], xyz)
        n_cut += int((counts < k).sum())
    assert n_cut > 0
    keys = O.l2_knn_keys(db.desc, db.q, k)
    assert np.array_equal(S.shard_keys_knn(db.desc, db.off, db.q, k, np.arange(1059), dd), keys)


def test_radius_form_and_its_inclusive_boundary_at_64_dimensions(small):
    db, dd = small
    for radius in D.RADII[:4]:
        for mpq in (1, 8, 64):
            want = R.match_l2_radius(db.desc, db.off, db.pts, db.q, radius, mpq, dd)
            rc, rp, m, xyz = O.l2_match(db.desc, db.off, db.pts, db.q, mpq, radius)
            assert rc == 0
            _same(want[:3], (rp, m, xyz), (radius, mpq))
            assert np.array_equal(want[3], (~(np.sqrt(dd) > np.float32(radius))).sum(axis=1))
    desc, off, pts, q, radius = D.boundary()
    assert desc.shape[1] == 64
    assert [float(R.d2(desc[r:r + 1], q[:1])[0, 0]) for r in (40, 41, 42)] == [3600.0, 3601.0, 3597.0]
    rp, m, xyz, in_radius = R.match_l2_radius(desc, off, pts, q, radius, 8)
    rc, o_rp, o_m, o_xyz = O.l2_match(desc, off, pts, q, 8, float(radius))
    assert rc == 0
    _same((rp, m, xyz), (o_rp, o_m, o_xyz), "boundary")
    glob = off[m["imgIdx"]].astype(np.int64) + m["trainIdx"]
    assert list(glob[:2]) == [42, 40] and m["distance"][1] == 60.0 and list(in_radius) == [2, 2, 2]   # d2 = 3600 is inside, 3601 is not
    assert list(glob[2:4]) == [104, 102]                                     # the same under a norm of 8e5


# ------------------------------------------------------------------------------------------------------------ the compiler's report
def _report(unit, extra=()):
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", *extra, "-c", "--cuda-device-only",
                              "-Rpass-analysis=kernel-resource-usage", "-o", os.path.join(d, "x.o"), os.path.join(CSRC, unit)],
                             check=True, capture_output=True, text=True, cwd=d)
    blocks = {}
    for b in re.split(r"remark: Function Name: ", out.stderr)[1:]:
        name = subprocess.run(["c++filt", b.split()[0]], capture_output=True, text=True, check=True).stdout.strip()
        blocks[name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]] = b
    return blocks


def _number(block, what):
    return int(re.search(re.escape(what) + r":? (\d+)", block).group(1))


def test_new_kernels_have_no_scratch_and_the_gemm_keeps_two_waves_per_simd():
    """From the compiler's own report, the Makefile's flags: every 64-wide kernel of l2.hip without scratch or spills, its four GEMM forms
    at no fewer than the two waves per SIMD their launch bound asks for, with half the ring (34 816 bytes of LDS a block)."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    blocks = _report("l2.hip")
    narrow = {n: b for n, b in blocks.items() if n.endswith("64u>") or n == "l2_prepare_narrow_kernel"}
    assert sorted(narrow) == sorted(["l2_prepare_narrow_kernel", "l2_gemm_kernel<1, 1u, 64u>", "l2_gemm_kernel<1, 4u, 64u>",
                                     "l2_gemm_kernel<1, 8u, 64u>", "l2_gemm_kernel<2, 4u, 64u>", "l2_rerank_kernel<64u>",
                                     "l2_exact_scan_kernel<64u>", "l2_radius_threshold_kernel<64u>", "l2_radius_refine_kernel<64u>",
                                     "l2_radius_scan_kernel<64u>"]), sorted(blocks)
    for name, b in narrow.items():
        print(name, _number(b, "VGPRs"), _number(b, "SGPRs"), _number(b, "Occupancy [waves/SIMD]"), _number(b, "LDS Size [bytes/block]"))
        assert _number(b, "ScratchSize [bytes/lane]") == 0 and _number(b, "VGPRs Spill") == 0 and _number(b, "SGPRs Spill") == 0, name
        if "gemm" in name:
            assert _number(b, "Occupancy [waves/SIMD]") >= 2 and _number(b, "VGPRs") + _number(b, "AGPRs") <= 256, name
            assert _number(b, "LDS Size [bytes/block]") == 4 * 2 * (32 * 64 * 2 + 256), name
    # the 128-wide forms are there beside them, under the names with the width
    assert all("l2_gemm_kernel<%s, 128u>" % f in blocks for f in ("1, 1u", "1, 4u", "1, 8u", "2, 4u"))


def test_the_narrow_cross_check_kernel_holds_its_row_in_registers():
    """cross_check_l2_narrow_kernel: a 64-float row per lane, at most 192 registers, at least two waves per SIMD, no scratch; and the
    128-wide kernel is still the one function of its name."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    blocks = _report("cross_check_l2.hip", ("-fno-slp-vectorize",))
    assert [n for n in blocks if "cross_check_l2_test_kernel" in n] == ["cross_check_l2_test_kernel"]
    b = blocks["cross_check_l2_narrow_kernel"]
    assert _number(b, "ScratchSize [bytes/lane]") == 0 and _number(b, "VGPRs Spill") == 0 and _number(b, "SGPRs Spill") == 0
    assert 64 < _number(b, "VGPRs") + _number(b, "AGPRs") <= 192 and _number(b, "Occupancy [waves/SIMD]") >= 2
    assert _number(b, "LDS Size [bytes/block]") <= 16 * 1024


# ------------------------------------------------------------------------------------------------------------ the header, the binding
def test_header_compiles_as_c_and_names_the_two_widths():
    text = open(os.path.join(ROOT, "include", "todhip.h"), encoding="utf-8").read()
    assert "dim = desc_bytes / 4 ∈ {64, 128}" in text and "desc_bytes == 256" in text
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write('#include "todhip.h"\nint (*p_load)(todhip_ctx*, const todhip_object*, uint32_t, uint32_t, uint32_t, uint32_t, float*) = todhip_db_load;\n')
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src, "-o",
                        os.path.join(d, "t.o")], check=True)


def test_a_256_byte_load_with_a_null_context_is_einval_and_the_binding_documents_the_width():
    L = capi.lib()
    spans = np.zeros(1, np.float32)
    assert L.todhip_db_load(None, None, C.c_uint32(0), C.c_uint32(256), C.c_uint32(0), C.c_uint32(1), spans.ctypes.data_as(C.c_void_p)) == capi.EINVAL
    assert "256" in capi.Context.desc_bytes.__doc__ and "f32[N,64]" in capi.Context.db_load.__doc__
    assert "64" in capi.Context.match_l2.__doc__ and "64" in capi.Context.cross_check_l2_device.__doc__
    from tod_amd import sharded, synth
    assert "desc_bytes=256" in sharded.__doc__
    desc, pts, off = synth.make_sift_db(2, per_object=10, dim=64)
    assert desc.shape == (20, 64) and desc.dtype == np.float32
