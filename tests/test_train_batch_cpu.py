"""todhip_model_add_observations_device without a GPU: the declaration (exported, plain C, the binding's argument types are the
header's), the refusals (all of them come before any device work, so zeroed memory stands for the context and the model), and the one
statement of a training view's per-keypoint arithmetic (tod_amd/csrc/train_validate.h) in a stand-alone host program built with
-fsanitize=address,undefined (tests/train_validate_host_test.cpp). The program checks the eroded pixel at every pixel of small images,
borders included, against four 3 x 3 erosions, and the rescue against a brute-force statement of its tie rule, on keypoints at k,
k + 0.5 and up to 1.5 pixels outside every border; what it writes is compared here with tests/train_ref.py (erode4, validate,
backproject) on the same inputs. This observes the erosion at the image border and the clamps of the rescue window, which no keypoint
of the ORB stage reaches (tests/test_train_edges_gpu.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import train_ref as TR
from tod_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "todhip_model_add_observations_device"


def _declaration():
    text = open(os.path.join(ROOT, "include", "todhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % NAME, code, flags=re.S)
    assert m, "include/todhip.h does not declare " + NAME
    return [" ".join(p.split()) for p in m.group(1).split(",")], text


def test_symbol_is_declared_exported_and_documented():
    params, text = _declaration()
    assert len(params) == 22
    assert NAME in capi.EXPORTS and hasattr(capi.lib(), NAME)
    comments = " ".join(" ".join(re.sub(r"\n \*", " ", c).split()) for c in re.findall(r"/\*.*?\*/", text, flags=re.S))
    for said in ("byte for byte the model after this sequence", "todhip_rescale_depth(view v's depth", "capacity cut",
                 "n_views == 0 or > 64", "exactly one of dH, dW zero", "before any device work"):
        assert said in comments, said


def test_header_declares_it_in_plain_c(tmp_path):
    """C99 with the prototype written out: another parameter list is an incompatible pointer, which -Werror refuses"""
    src = tmp_path / "t.c"
    src.write_text('#include "todhip.h"\n'
                   "typedef int (*fn)(todhip_ctx*, todhip_model*, const void*, uint64_t, uint32_t, const void*, const void*, int, uint32_t,\n"
                   "                  uint32_t, int, uint32_t, uint32_t, uint32_t, const float*, const float*, const float*, uint32_t, uint32_t,\n"
                   "                  float, const int8_t*, uint32_t*);\n"
                   "fn the_call = %s;\n" % NAME)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "t.o")], check=True)


def test_binding_argument_types_are_the_headers():
    params, _ = _declaration()

    def ctype(p):
        if "*" in p:
            return C.c_void_p
        return {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int": C.c_int, "float": C.c_float}[p.split()[0]]
    want = [ctype(p) for p in params]
    assert capi.ADD_OBSERVATIONS_DEVICE_ARGTYPES == want
    f = getattr(capi.lib(), NAME)
    assert list(f.argtypes) == want and f.restype is C.c_int


def test_refusals_come_before_any_device_work():
    L = capi.lib()
    buf = C.create_string_buffer(1 << 16)                       # zeroed memory: every call returns before it reads any of it
    x = C.addressof(buf)
    cams = (C.c_float * (9 * 64))()
    n_added = (C.c_uint32 * 64)(*([7] * 64))

    def call(ctx=x, model=x, gray=x, fs=64 * 64, stride=64, mask=x, depth=x, dH=0, dW=0, n_views=2, H=64, W=64, K=cams, R=cams, T=cams,
             n_features=100, n_levels=1, sf=1.2):
        return getattr(L, NAME)(ctx, model, gray, fs, stride, mask, depth, 0, dH, dW, 0, n_views, H, W, K, R, T, n_features, n_levels, sf,
                                None, n_added)
    # what the single-view call refuses
    for kw in (dict(ctx=None), dict(model=None), dict(gray=None), dict(depth=None), dict(K=None), dict(R=None), dict(T=None),
               dict(H=7, fs=7 * 64), dict(W=7, stride=7), dict(n_features=0), dict(n_levels=0), dict(n_levels=17), dict(sf=1.0)):
        assert call(**kw) == capi.EINVAL, kw
    # the batch's own
    for kw in (dict(mask=None), dict(n_views=0), dict(n_views=65), dict(stride=63), dict(fs=64 * 64 - 1), dict(stride=80, fs=64 * 80 - 1),
               dict(dH=32), dict(dW=32), dict(dH=64, dW=16), dict(dH=1, dW=1024)):       # (64 x 16 -> 64 columns: 256 rows; 1 x 1024: none)
        assert call(**kw) == capi.EINVAL, kw
    assert call(n_views=1, fs=0, ctx=None) == capi.EINVAL
    assert list(n_added) == [7] * 64 and buf.raw == bytes(1 << 16)


SIZES = ((1, 1), (3, 20), (9, 9), (13, 40), (37, 41))


def _inputs():
    """(tag, mask, keypoints, depth) per case: masks with sparse holes (about two thirds of the eroded pixels stay open), all open
    and all closed; keypoints on every half-integer from 1.5 pixels outside the image on, plus seeded fractional ones; depth with
    every special value of cv::isValidDepth"""
    rng = np.random.Generator(np.random.PCG64(41))
    out = []
    for H, W in SIZES:
        masks = [("holes", np.where(rng.random((H, W)) < 1.0 / 120.0, 0, 255).astype(np.uint8)), ("open", np.full((H, W), 255, np.uint8))]
        if (H, W) == (1, 1):
            masks = [("open", np.full((1, 1), 255, np.uint8)), ("closed", np.zeros((1, 1), np.uint8))]
        if (H, W) == (9, 9):
            corner = np.full((9, 9), 255, np.uint8); corner[8, 0] = 0
            masks.append(("corner", corner))
        if (H, W) == (37, 41):
            masks.append(("comb", TR.comb_mask(H, W)))
        xs, ys = np.arange(-1.5, W + 1.0, 0.5), np.arange(-1.5, H + 1.0, 0.5)
        grid = np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2)
        frac = rng.uniform(-2.0, 2.0, (300, 2)) + rng.integers(0, (W, H), (300, 2))
        kp = np.concatenate([grid, frac]).astype(np.float32)
        z, _ = TR.special_depth(11 + H, H, W)
        for tag, mask in masks:
            out.append(("%dx%d_%s" % (H, W, tag), mask, kp, z))
    return out


def test_header_arithmetic_on_the_host_under_sanitizers(tmp_path):
    exe = str(tmp_path / "train_validate_host_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tod_amd", "csrc"),
                    os.path.join(ROOT, "tests", "train_validate_host_test.cpp"), "-o", exe], check=True)
    cases = _inputs()
    K, R, T = TR.camera(320), TR.general_matrix(), TR.T
    np.concatenate([[K[0, 0], K[1, 1], K[0, 2], K[1, 2]], R.reshape(9), T]).astype(np.float32).tofile(str(tmp_path / "cam"))
    lines = []
    for tag, mask, kp, z in cases:
        mask.tofile(str(tmp_path / (tag + ".mask"))); kp.tofile(str(tmp_path / (tag + ".kp"))); z.tofile(str(tmp_path / (tag + ".z")))
        lines.append("%d %d %d %s %s %s %s %s" % (mask.shape + (len(kp),) + tuple(str(tmp_path / (tag + e)) for e in (".mask", ".kp", ".z")) +
                                                   (str(tmp_path / "cam"), str(tmp_path / tag))))
    (tmp_path / "cases").write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(tmp_path / "cases")], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr[:4000]
    assert out.stdout.split("\n")[:-1] == ["ok %d %d %d" % (mask.shape + (len(kp),)) for _, mask, kp, _ in cases]
    seen = np.zeros(4, np.int64)
    border_rescues = ties = 0
    for tag, mask, kp, z in cases:
        H, W = mask.shape
        er = np.fromfile(str(tmp_path / (tag + ".er")), np.uint8).reshape(H, W)
        res = np.fromfile(str(tmp_path / (tag + ".res")), np.int32).reshape(-1, 3)
        pts = np.fromfile(str(tmp_path / (tag + ".pts")), np.float32).reshape(-1, 3)
        assert np.array_equal(er, TR.erode4(mask)), tag
        cls, pix = TR.validate(kp, mask, z)
        assert np.array_equal(res[:, 0], cls) and np.array_equal(res[:, 1:], pix), tag
        src = np.flatnonzero((cls == TR.DIRECT) | (cls == TR.RESCUED))
        want = TR.backproject(pix[src], z[pix[src, 1], pix[src, 0]], K, R, T)
        assert TR.same_points(pts[src], want), tag
        assert not pts[np.setdiff1d(np.arange(len(kp)), src)].any(), tag
        seen += np.bincount(cls, minlength=4)
        resc = cls == TR.RESCUED
        border_rescues += int((resc & ((pix[:, 0] < 2) | (pix[:, 0] >= W - 2) | (pix[:, 1] < 2) | (pix[:, 1] >= H - 2))).sum())
        ties += int((resc & (kp[:, 0] * 2 == np.rint(kp[:, 0] * 2)) & (kp[:, 1] * 2 == np.rint(kp[:, 1] * 2))).sum())
    # the inputs reach what they are for: every class, rescues that end within 2 pixels of a border, rescues of half-integer keypoints
    assert (seen >= 50).all() and border_rescues >= 50 and ties >= 200, (seen, border_rescues, ties)
