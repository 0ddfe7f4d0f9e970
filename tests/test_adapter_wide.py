"""The DescriptorMatcher cell of adapter/ecto_cells.hpp on 64-byte descriptors, through the mini_ecto test double
(tests/adapter_wide_test.cpp): the width comes from the documents, the cell's matches equal the C ABI's on the same data, and a query
matrix of another width throws instead of being read at the wrong stride."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import adapter_wide_build

pytestmark = pytest.mark.gpu


def test_wide_frame_through_the_cell_equals_c_abi():
    from tod_amd import capi, synth
    exe = adapter_wide_build.build()
    desc, pts, off = synth.make_db_ragged([3000, 0, 10, 2500], desc_bytes=64, seed=5)
    fr = synth.make_frame(desc, pts, off, 500, frame=3, visible_object=3)
    with tempfile.TemporaryDirectory() as d:
        for name, arr in (("desc", desc), ("pts", pts), ("obj_off", off.astype(np.uint32)), ("q_desc", fr["q_desc"])):
            np.ascontiguousarray(arr).tofile(os.path.join(d, name + ".bin"))
        out = subprocess.run([exe, d], capture_output=True, text=True)       # exit 7: the 32-column query did not throw
        assert out.returncode == 0 and "adapter wide ok" in out.stdout, out.stdout + out.stderr
        m = np.fromfile(os.path.join(d, "out_matches.bin"), np.int32).reshape(-1, 3)
        dist = np.fromfile(os.path.join(d, "out_dist.bin"), np.float32)
        xyz = np.fromfile(os.path.join(d, "out_xyz.bin"), np.float32).reshape(-1, 3)
    ctx = capi.Context(0)
    try:
        ctx.db_load(desc, pts, off)
        row_ptr, gm, gxyz = ctx.match(fr["q_desc"], 5, 70)                   # the cell's k is 5 (DescriptorMatcher.cpp:211)
    finally:
        ctx.close()
    assert len(gm) > 100 and gm["distance"].max() > 20
    assert np.array_equal(m[:, 0], gm["queryIdx"]) and np.array_equal(m[:, 1], gm["trainIdx"])
    assert np.array_equal(m[:, 2], gm["imgIdx"]) and np.array_equal(dist, gm["distance"]) and np.array_equal(xyz, gxyz)
