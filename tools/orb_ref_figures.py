"""The figures of profiles/orb_ref.json as one JSON document on stdout: how far the C restatement (oracle/orb_oracle.c) and, with
--gpu, the library are from tests/orb_ref.py, the float64 / int64 statement of stage A, on every case of orb_ref.CASES -- the largest
response error in units of u M, the largest angle error in degrees and the share of bits the half-integer guard leaves out, per input
-- and how far the fixed-point resize and blur are from float64 bilinear interpolation and a float64 Gaussian. The bounds beside them
are the ones the tests assert. Usage: python tools/orb_ref_figures.py [--gpu] > profiles/orb_ref.json"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import oracle_lib as O      # noqa: E402
import orb_ref as R         # noqa: E402


def per_case(run, names):
    out, worst = {}, {}
    for name in names:
        img, nf, nl, sf, kw = R.case_args(name)
        s = R.compare(run(img, nf, nl, sf, **kw), R.case_ref(name))
        out[name] = dict(keypoints=s["n"], response_err_uM=round(s["response_err"], 3), angle_err_deg=float("%.3g" % s["angle_err"]),
                         left_out_share=round(s["left_out"], 6))
        R.merge_stats(worst, s)
    return dict(max_response_err_uM=round(worst["response_err"], 3), max_angle_err_deg=float("%.3g" % worst["angle_err"]),
                max_left_out_share=round(worst["left_out"], 6), cases=out)


def fixed_point():
    rng = np.random.Generator(np.random.PCG64(1))
    resize, blur = {}, {}
    for src, dst in (((160, 200), (133, 167)), ((100, 100), (50, 50)), ((1, 200), (1, 167))):
        for kind, img in (("noise", rng.integers(0, 256, src, dtype=np.uint8)), ("rect", R.padded_to(R.image("rect"), 200, 200)[:src[0], :src[1]])):
            dev = np.abs(R.resize_fixed(img, *dst).astype(np.float64) - R.resize_float64(img, *dst)).max()
            resize["%dx%d->%dx%d %s" % (src + dst + (kind,))] = round(float(dev), 3)
    for name in ("rect", "noise", "lattice", "tiny63"):
        blur[name] = round(float(np.abs(R.blur_fixed(R.image(name)).astype(np.float64) - R.blur_float64(R.image(name))).max()), 3)
    return dict(resize_max_grey_levels=max(resize.values()), resize_bound=1.0, resize=resize, blur_max_grey_levels=max(blur.values()),
                blur_bound=round(2 * (255 * 2.22 / 256 + 0.5), 2), blur=blur)


doc = dict(what="distance of stage A from tests/orb_ref.py (float64 responses, angles and steering; int64 everything else)",
           bounds=dict(response_err_uM=R.RESPONSE_TOL, angle_err_deg=R.ANGLE_TOL, left_out_share=R.LEFT_OUT_LIMIT),
           ambiguous_selection_boundaries={k: R.case_ref(k).ambiguous for k in R.CASES if R.case_ref(k).ambiguous},
           restatement=per_case(O.orb, sorted(R.CASES)), fixed_point_stages=fixed_point())
if "--gpu" in sys.argv[1:]:
    from tod_amd import capi
    ctx = capi.Context(0)
    doc["library_gfx950"] = per_case(ctx.orb, list(R.GPU_CASES))
    a, b = (ctx.orb(*R.case_args(k)[:4]) for k in ("rect_all_1", "rect_T_all_1"))
    doc["library_gfx950"]["transposed_angle_err_deg"] = float("%.3g" % R.transposition_holds(a, b, R.case_ref("rect_all_1")))
    ctx.close()
else:
    doc["library_gfx950"] = "not measured"
a, b = (O.orb(*R.case_args(k)[:4]) for k in ("rect_all_1", "rect_T_all_1"))
doc["restatement"]["transposed_angle_err_deg"] = float("%.3g" % R.transposition_holds(a, b, R.case_ref("rect_all_1")))
json.dump(doc, sys.stdout, indent=1)
print()
