"""todhip_match_radius without a GPU: the numpy statement of its definition (tests/match_radius_ref.py) against the oracle, and the
boundary -- libtodhip.so exports both entry points, include/todhip.h declares them with the expected C signatures, and
tod_amd/capi.py binds them in the header's argument order."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import match_radius_ref as R
import oracle_lib as O
from tod_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("queryIdx", "trainIdx", "imgIdx", "distance")


@pytest.fixture(scope="module")
def small():
    """600 rows in 8 objects (one empty), 40 queries: rows with 0..20 flipped bits, every fifth random"""
    rng = np.random.Generator(np.random.PCG64(7))
    rows = [100, 0, 1, 33, 200, 64, 2, 200]
    off = np.concatenate([[0], np.cumsum(rows)]).astype(np.uint32)
    desc = rng.integers(0, 256, (600, 32), dtype=np.uint8)
    desc[300:320] = desc[10]                                           # ties: twenty copies of one row
    pts = rng.standard_normal((600, 3)).astype(np.float32)
    q = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    for i in range(40):
        if i % 5 != 4:
            bits = np.unpackbits(desc[int(rng.integers(0, 600))])
            bits[rng.choice(256, int(rng.integers(0, 21)), replace=False)] ^= 1
            q[i] = np.packbits(bits)
    q[0] = desc[10]
    return desc, off, pts, q


@pytest.mark.parametrize("max_per_query", [1, 5, 64])
@pytest.mark.parametrize("radius", [1, 35, 128, 256])
def test_reference_equals_the_oracle(small, radius, max_per_query):
    desc, off, pts, q = small
    rp, m, xyz, in_radius = R.match_radius(desc, off, pts, q, radius, max_per_query)
    rc, o_rp, o_m, o_xyz = O.match(desc, off, pts, q, max_per_query, radius)
    assert rc == 0 and np.array_equal(rp, o_rp) and np.array_equal(xyz, o_xyz)
    for f in FIELDS:
        assert np.array_equal(m[f], o_m[f]), f
    keys = O.knn_keys(desc, q, len(desc))
    assert np.array_equal(in_radius, ((keys >> np.uint64(32)) <= np.uint64(radius)).sum(axis=1))
    if radius == 256:
        assert (in_radius == 600).all()
    if radius == 1:
        assert in_radius[0] == 21 and rp[1] == min(21, max_per_query)       # the ties, lowest rows first
        assert list(off[m["imgIdx"][:rp[1]]] + m["trainIdx"][:rp[1]]) == ([10] + list(range(300, 320)))[:max_per_query]


def test_reference_on_a_subset_of_the_rows(small):
    """rows=: what a shard or a selection searches -- the oracle on the subset DB with the rows mapped back"""
    desc, off, pts, q = small
    rows = np.arange(off[3], off[6])
    rp, m, xyz, in_radius = R.match_radius(desc, off, pts, q, 40, 5, rows=rows)
    rc, o_rp, o_m, o_xyz = O.match(desc[rows], off[3:7] - off[3], pts[rows], q, 5, 40)
    assert rc == 0 and np.array_equal(rp, o_rp) and np.array_equal(xyz, o_xyz)
    assert np.array_equal(m["imgIdx"], o_m["imgIdx"] + 3) and np.array_equal(m["trainIdx"], o_m["trainIdx"])
    assert np.array_equal(in_radius, (R.distances(desc[rows], q) <= 40).sum(axis=1))


def test_capacity_formula():
    assert [capi.radius_capacity(m) for m in (1, 5, 8, 32, 33, 64, 1024)] == [64, 64, 64, 64, 128, 128, 2048]


# ---------------------------------------------------------------------------------------------------- the boundary
SIGNATURES = {
    "todhip_match_radius": "todhip_ctx*, const uint8_t*, uint32_t, uint32_t, uint32_t, uint32_t*, todhip_dmatch*, float*, uint32_t*, uint32_t*",
    "todhip_match_radius_device": "todhip_ctx*, const void*, uint32_t, uint32_t, uint32_t, void*, void*, void*, void*",
}
NAMES = {
    "todhip_match_radius": ["", "q_desc", "nq", "radius", "max_per_query", "row_ptr", "matches", "matches_xyz", "n_matches", "in_radius"],
    "todhip_match_radius_device": ["", "d_q_desc", "nq", "radius", "max_per_query", "d_counts", "d_matches", "d_matches_xyz", "d_in_radius"],
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
        want = [C.c_void_p if "*" in t else {"uint32_t": C.c_uint32}[t] for t, _ in params]
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == want, name
    assert callable(capi.Context.match_radius) and callable(capi.Context.match_radius_device)


def test_header_declares_the_expected_c_signatures():
    """a three-line C file: assigning the functions to pointers of the expected type compiles without a warning only when the
    header's parameter types and order are these"""
    lines = ['#include "todhip.h"'] + ["int (*p_%s)(%s) = %s;" % (n, sig, n) for n, sig in SIGNATURES.items()]
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write("\n".join(lines) + "\n")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-c", src, "-o", os.path.join(d, "t.o")], check=True)
