"""CPU checks of the pipeline's boundary (todhip_pipeline_*): parameters are validated before any device work, the ctypes
structs have the library's layout, creation fails loudly without a GPU, and the C++ example builds against the header."""
import ctypes as C
import os
import subprocess

import pytest

from tod_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _create(p):
    h = C.c_void_p()
    rc = capi.lib().todhip_pipeline_create(C.c_int(0), C.byref(p), C.byref(h))
    if h:
        capi.lib().todhip_pipeline_destroy(h)
    return rc


def test_params_struct_size_matches_the_library():
    p = capi.pipeline_params()
    assert p.struct_size == C.sizeof(capi.PipelineParams)
    assert (p.frames_per_step, p.n_features, p.k, p.radius, p.ring_depth) == (32, 1000, 5, 55, 4)
    assert C.sizeof(capi.PipelineStats) == 9 * 8
    assert (capi.EBUSY, capi.ETIMEOUT) == (-8, -9)


@pytest.mark.parametrize("field,value", [("struct_size", 4), ("frames_per_step", 0), ("frames_per_step", 65), ("ring_depth", 2),
                                         ("ring_depth", 1), ("k", 0), ("k", 9), ("radius", 0), ("frame_format", 3), ("W", 0)])
def test_bad_parameters_are_rejected_before_device_work(field, value):
    """EINVAL, with or without a GPU (without one, anything that reached the device would be EHIP). ring_depth 2 with the default
    2 verifier workers: ring_depth <= verify_workers."""
    p = capi.pipeline_params(**{field: value})
    assert _create(p) == capi.EINVAL


def test_null_arguments():
    L = capi.lib()
    assert L.todhip_pipeline_create(C.c_int(0), None, C.byref(C.c_void_p())) == capi.EINVAL
    assert L.todhip_pipeline_create(C.c_int(0), C.byref(capi.pipeline_params()), None) == capi.EINVAL
    assert L.todhip_pipeline_default_params(None) == capi.EINVAL
    assert L.todhip_pipeline_get_stats(None, None) == capi.EINVAL
    assert L.todhip_pipeline_matcher(None) is None
    L.todhip_pipeline_destroy(None)


def test_create_without_a_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    assert _create(capi.pipeline_params()) == capi.EHIP
    with pytest.raises(capi.TodError):
        capi.Pipeline(0)


def test_example_host_compiles_and_links(tmp_path):
    """examples/pipeline_host.cpp against include/ and the built library: todhip.h and the standard library only. Not run."""
    capi.lib()
    src = os.path.join(ROOT, "examples", "pipeline_host.cpp")
    text = open(src).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert '"todhip.h"' in includes and all(i == '"todhip.h"' or i.startswith("<") for i in includes)
    assert "hip/" not in text and "torch" not in text
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), src,
                    "-L", os.path.join(ROOT, "tod_amd"), "-ltodhip", "-Wl,-rpath," + os.path.join(ROOT, "tod_amd"),
                    "-Wl,--allow-shlib-undefined", "-o", str(tmp_path / "pipeline_host")], check=True)
