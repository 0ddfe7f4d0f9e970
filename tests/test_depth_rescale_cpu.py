"""The one statement of rescale_depth's arithmetic (tod_amd/csrc/depth_rescale.h) without a GPU: a stand-alone host program, built with
-fsanitize=address,undefined, writes rescaled_depth_at for every pixel of small geometries (tests/depth_rescale_host_test.cpp), and
the result must equal the CPU restatement (oracle_lib.train_rescale_depth) bit for bit, NaN positions included. The same file holds
the refusals of the new entry points that need no device, and that the header documents them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import depth_cases as DC
import oracle_lib as O
from tod_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_reference_accepts_and_refuses_the_geometries():
    for (dH, dW, H, W), _ in DC.GEOMETRIES:
        for nearest in (False, True):
            assert O.train_rescale_depth(DC.source(dH, dW, False), H, W, nearest) is not None, (dH, dW, H, W)
    dH, dW, H, W = DC.REFUSED
    for u16 in (False, True):
        for nearest in (False, True):
            assert O.train_rescale_depth(DC.source(dH, dW, u16), H, W, nearest) is None


def test_header_arithmetic_equals_the_cpu_restatement(tmp_path):
    exe = str(tmp_path / "depth_rescale_host_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tod_amd", "csrc"),
                    os.path.join(ROOT, "tests", "depth_rescale_host_test.cpp"), "-o", exe], check=True)
    lines = []
    for i, case in enumerate(DC.CASES):
        (dH, dW, H, W), u16, nearest = case
        src, _ = DC.reference(case)
        src.tofile(str(tmp_path / ("src%d" % i)))
        lines.append("%d %d %d %d %d %d %s %s" % (u16, dH, dW, H, W, nearest, tmp_path / ("src%d" % i), tmp_path / ("out%d" % i)))
    for nearest in (0, 1):                                      # the refused geometry: no source is read
        lines.append("0 %d %d %d %d %d none none" % (DC.REFUSED + (nearest,)))
    (tmp_path / "cases").write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(tmp_path / "cases")], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    said = out.stdout.split("\n")[:-1]
    assert len(said) == len(DC.CASES) + 2 and said[-2:] == ["refused", "refused"]
    band = False
    for i, case in enumerate(DC.CASES):
        (dH, dW, H, W), u16, nearest = case
        _, want = DC.reference(case)
        ok, sub_rows, mode = said[i].split()
        got = np.fromfile(str(tmp_path / ("out%d" % i)), np.float32).reshape(H, W)
        assert ok == "ok" and DC.same_bits(got, want), DC.case_id(case)
        # the geometry itself: which path ran, and the NaN band below the resized rows
        if (dH, dW) == (H, W):
            assert int(mode) == 0 and int(sub_rows) == H
        elif (dH, dW) == (20, 28) and not nearest:
            assert int(mode) == 3
        else:
            assert int(mode) == (1 if nearest else 2)
        assert np.isnan(got[int(sub_rows):]).all() and not np.isnan(got[:int(sub_rows)]).all()
        band = band or int(sub_rows) < H
    assert band                                                 # (4 x 8 -> 12 x 16 leaves rows 8-11 without depth)
    # bilinear and nearest are different results wherever there is a resize
    for g, _ in DC.GEOMETRIES[:5]:
        assert not DC.same_bits(DC.reference((g, False, False))[1], DC.reference((g, False, True))[1]), g


def _fake(n=1 << 16):
    """zeroed memory that stands for an object the call must refuse before it looks at it"""
    return C.create_string_buffer(n)


def test_new_entry_points_refuse_without_a_device():
    L = capi.lib()
    buf = _fake()
    x = C.addressof(buf)                                        # any non-null pointer: every call returns before reading it
    n_out = (C.c_uint32 * 4)()
    K9 = (C.c_float * 9)(525, 0, 8, 0, 525, 6, 0, 0, 1)
    prm = capi.VerifyParams(8, 100, 0.01)
    rng = capi.rng_new(1)
    n_p, n_i, pose_ptr = C.c_uint32(0), C.c_uint32(0), (C.c_uint32 * 3)()

    def orb(ctx=x, gray=x, mask=x, n_frames=2, fs=64 * 64, stride=64, out=n_out):
        return L.todhip_orb_batch_device_masked(ctx, gray, mask, n_frames, fs, 64, 64, stride, 100, 1, 1.2, None, x, x, x, 100, out)
    assert orb(ctx=None) == capi.EINVAL and orb(gray=None) == capi.EINVAL and orb(out=None) == capi.EINVAL
    assert orb(n_frames=0) == capi.EINVAL and orb(stride=63) == capi.EINVAL and orb(fs=64 * 64 - 1) == capi.EINVAL

    def single(ctx=x, depth=x, K=K9, dH=4, dW=8, H=12, W=16):
        return L.todhip_verify_device_depth_rescaled(ctx, x, 10, depth, 0, dH, dW, 0, H, W, K, x, x, x, 5, x, 1, C.byref(prm), C.byref(rng),
                                                     None, C.byref(n_p), None, C.byref(n_i))

    def batch(ctx=x, depth=x, K=K9, dH=4, dW=8, H=12, W=16, pp=pose_ptr):
        return L.todhip_verify_batch_device_depth_rescaled(ctx, 2, x, 10, depth, 0, dH, dW, 0, H, W, K, x, x, x, 5, x, 1, C.byref(prm),
                                                           C.byref(rng), None, C.byref(n_p), pp, None, C.byref(n_i))
    rdH, rdW, rH, rW = DC.REFUSED
    for call in (single, batch):
        assert call(ctx=None) == capi.EINVAL and call(depth=None) == capi.EINVAL and call(K=None) == capi.EINVAL
        assert call(dH=0) == capi.EINVAL and call(dW=0) == capi.EINVAL
        assert call(dH=rdH, dW=rdW, H=rH, W=rW) == capi.EINVAL      # with a context: refused before any device work
    assert batch(pp=None) == capi.EINVAL
    assert rng.draws == 0

    kp, z = (C.c_float * 2)(1, 1), (C.c_float * 1)(7)

    def hook(ctx=x, depth=x, kpp=kp, zz=z, n=1, dH=4, dW=8, H=12, W=16):
        return L.todhip_test_depth_lookup(ctx, depth, 0, dH, dW, 0, H, W, kpp, n, zz)
    assert hook(ctx=None) == capi.EINVAL and hook(depth=None) == capi.EINVAL and hook(kpp=None) == capi.EINVAL
    assert hook(zz=None) == capi.EINVAL and hook(n=0) == capi.EINVAL and hook(dH=rdH, dW=rdW, H=rH, W=rW) == capi.EINVAL
    assert z[0] == 7

    t = C.c_uint64(0)
    assert L.todhip_pipeline_set_depth_size(None, 240, 320, 0) == capi.EINVAL
    assert L.todhip_pipeline_submit_masked(None, x, x, x, 1, C.byref(t)) == capi.EINVAL
    assert L.todhip_pipeline_submit_masked_device(None, x, x, x, 1, C.byref(t)) == capi.EINVAL


def test_params_struct_is_unchanged():
    """todhip_pipeline_params did not grow: the depth size and the masks came as calls (its size is checked by todhip_pipeline_create)"""
    assert C.sizeof(capi.PipelineParams) == 112
    p = capi.PipelineParams()
    assert capi.lib().todhip_pipeline_default_params(C.byref(p)) == capi.OK and p.struct_size == 112


def test_header_documents_the_new_calls():
    text = open(os.path.join(ROOT, "include", "todhip.h")).read()
    comments = " ".join(re.findall(r"/\*.*?\*/", text, flags=re.S))
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("todhip_orb_batch_device_masked", "todhip_verify_device_depth_rescaled", "todhip_verify_batch_device_depth_rescaled",
                 "todhip_test_depth_lookup", "todhip_pipeline_set_depth_size", "todhip_pipeline_submit_masked",
                 "todhip_pipeline_submit_masked_device"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in capi.EXPORTS
    for said in ("todhip_pipeline_set_depth_size", "todhip_pipeline_submit_masked[_device]", "todhip_rescale_depth_device",
                 "todhip_orb_batch_device_masked", "todhip_verify_batch_device_depth_rescaled", "NaN band"):
        assert said in comments, said
