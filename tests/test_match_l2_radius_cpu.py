"""todhip_match_l2_radius without a GPU: the numpy statement of its definition (tests/match_l2_radius_ref.py) against the oracle --
l2_match(k = max_per_query, radius) defines the matches, a count over l2_knn_keys(k = n_rows) defines in_radius -- bit for bit, and
the boundary: libtodhip.so exports both entry points, include/todhip.h declares them with the expected C signatures, and
tod_amd/capi.py binds them in the header's argument order."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import l2_radius_cases as K
import match_l2_radius_ref as R
import oracle_lib as O
from tod_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle(desc, off, pts, q, radius, mpq, keys=None):
    """the definition through the oracle: (row_ptr, matches, xyz, in_radius)"""
    rc, rp, m, xyz = O.l2_match(desc, off, pts, q, mpq, radius)
    assert rc == 0
    keys = O.l2_knn_keys(desc, q, len(desc)) if keys is None else keys
    d2 = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return rp, m, xyz, (~(np.sqrt(d2) > np.float32(radius))).sum(axis=1).astype(np.uint32)


def same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), what
    for f in K.FIELDS:
        assert np.array_equal(got[1][f], want[1][f]), (what, f)
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), what


@pytest.fixture(scope="module")
def small():
    db = K.Db(nq=70)
    return db, O.l2_knn_keys(db.desc, db.q, len(db.desc))


@pytest.mark.parametrize("max_per_query", [1, 5, 64, 1024])
@pytest.mark.parametrize("radius", K.RADII)
def test_reference_equals_the_oracle(small, radius, max_per_query):
    db, keys = small
    got = R.match_l2_radius(db.desc, db.off, db.pts, db.q, radius, max_per_query)
    same(got, oracle(db.desc, db.off, db.pts, db.q, radius, max_per_query, keys), (radius, max_per_query))
    n = len(db.desc)
    if radius == K.RADII[0]:
        assert not got[3].any()
    elif radius == K.RADII[-1]:
        assert (got[3] == n).all()
    else:
        assert 0 < got[3].max() < n and (radius != K.RADII[2] or got[3].min() > 64)     # 1150: every query is cut at 64


def test_a_row_exactly_on_the_radius_is_inside_and_one_ulp_less_puts_it_outside():
    desc, off, pts, q, radius = K.boundary()
    for qi, on, nearer, beyond in ((0, 40, 42, 41), (1, 102, 104, 103), (2, 40, 42, 41)):
        d2 = R.d2(desc, q[qi:qi + 1])[0]
        assert d2[on] == 3600 and d2[nearer] == 3597 and d2[beyond] == 3601 and (np.delete(d2, [on, nearer, beyond]) > 3601).all()
    for r, inside in ((radius, 2), (np.nextafter(radius, np.float32(0)), 1)):
        got = R.match_l2_radius(desc, off, pts, q, r, 5)
        same(got, oracle(desc, off, pts, q, r, 5), float(r))
        assert list(got[3]) == [inside] * 3
    rows = off[got[1]["imgIdx"]].astype(np.int64) + got[1]["trainIdx"]
    assert list(rows) == [42, 104, 42]


# ---------------------------------------------------------------------------------------------------- the boundary
SIGNATURES = {
    "todhip_match_l2_radius": "todhip_ctx*, const float*, uint32_t, float, uint32_t, uint32_t*, todhip_dmatch*, float*, uint32_t*, uint32_t*",
    "todhip_match_l2_radius_device": "todhip_ctx*, const void*, uint32_t, float, uint32_t, void*, void*, void*, void*",
}
NAMES = {
    "todhip_match_l2_radius": ["", "q_desc", "nq", "radius", "max_per_query", "row_ptr", "matches", "matches_xyz", "n_matches", "in_radius"],
    "todhip_match_l2_radius_device": ["", "d_q_desc", "nq", "radius", "max_per_query", "d_counts", "d_matches", "d_matches_xyz", "d_in_radius"],
}


def _header_params(name):
    """[(type, parameter name)] of a function as include/todhip.h declares it"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "todhip.h")).read(), flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, name + " is not declared in include/todhip.h"
    out = []
    for p in m.group(1).split(","):
        t = re.match(r"\s*(.*?[\s*])([a-z_0-9]*)\s*$", p, flags=re.S)
        out.append((t.group(1).strip(), t.group(2)))
    return out


def test_library_exports_and_capi_binds_both_entry_points():
    L = capi.lib()
    for name in SIGNATURES:
        assert hasattr(L, name), "libtodhip.so does not export " + name
        assert name in capi.EXPORTS
        params = _header_params(name)
        assert [n for _, n in params] == NAMES[name]
        want = [C.c_void_p if "*" in t else {"uint32_t": C.c_uint32, "float": C.c_float}[t] for t, _ in params]
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == want, name
    assert callable(capi.Context.match_l2_radius) and callable(capi.Context.match_l2_radius_device)


def test_header_declares_the_expected_c_signatures():
    """a three-line C file: assigning the functions to pointers of the expected type compiles without a warning only when the
    header's parameter types and order are these"""
    lines = ['#include "todhip.h"'] + ["int (*p_%s)(%s) = %s;" % (n, sig, n) for n, sig in SIGNATURES.items()]
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write("\n".join(lines) + "\n")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-c", src, "-o", os.path.join(d, "t.o")], check=True)
