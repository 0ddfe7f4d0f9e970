"""CPU checks of the drop-in boundary: libtodhip.so loads and exports every function that
include/todhip.h declares (no compute calls without a GPU)."""
import ctypes
import os
import re

import pytest

from tod_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "todhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(todhip_[a-z_0-9]+)\s*\(", text)))


def test_library_loads_and_exports_every_declared_symbol():
    L = capi.lib()
    names = _declared()
    assert len(names) >= 15
    for n in names:
        assert hasattr(L, n), "libtodhip.so does not export " + n
    assert sorted(capi.EXPORTS) == names
    assert L.todhip_version() == 1


SCALARS = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "int": ctypes.c_int, "float": ctypes.c_float}


def _header_prototype(code, name):
    """(restype, argtypes) that the header's declaration of `name` asks of a ctypes binding: this file's own reading of the text"""
    m = re.search(r"(\w+)\s*(\*?)\s*\b%s\s*\((.*?)\)\s*;" % name, code, flags=re.S)
    assert m, "include/todhip.h does not declare " + name
    ret, star, params = m.groups()
    restype = ctypes.c_void_p if star else {"void": None, "int": ctypes.c_int}[ret]
    argtypes = []
    for p in [" ".join(p.replace("const ", "").split()) for p in params.split(",")]:
        if p != "void":
            argtypes.append(ctypes.c_void_p if "*" in p or "[" in p else SCALARS[p.split()[0]])
    return restype, argtypes


def test_every_prototype_is_the_headers():
    """argtypes and restype of each of the declared functions, as the loader set them, against the header's text"""
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "todhip.h")).read(), flags=re.S)
    L = capi.lib()
    names = _declared()
    assert len(names) >= 105
    for name in names:
        restype, argtypes = _header_prototype(code, name)
        f = getattr(L, name)
        assert list(f.argtypes) == argtypes, name
        assert f.restype is restype, name
    assert L.todhip_stream.restype is ctypes.c_void_p and L.todhip_pipeline_matcher.restype is ctypes.c_void_p
    assert L.todhip_rng_seed.restype is None and L.todhip_rng_seed.argtypes == [ctypes.c_void_p, ctypes.c_uint32]
    assert L.todhip_version.argtypes == [] and L.todhip_set_ratio_test.argtypes == [ctypes.c_void_p, ctypes.c_float]


def test_wrong_kind_of_argument_is_refused_at_the_call():
    """The point of the prototypes: a wrapper of another type than the header's, or a numpy scalar for a pointer, raises; nothing is
    truncated. (Both calls would return EINVAL for their NULL context if they went through.)"""
    import numpy as np
    L = capi.lib()
    with pytest.raises(ctypes.ArgumentError):
        L.todhip_set_matcher_engine(None, ctypes.c_uint32(1))               # the header says int
    with pytest.raises(ctypes.ArgumentError):
        L.todhip_db_bit_order(None, np.uint64(1 << 40))                     # the header says a pointer
    assert L.todhip_set_matcher_engine(None, np.int64(1)) == capi.EINVAL and L.todhip_set_matcher_engine(None, True) == capi.EINVAL


def test_unknown_parameter_type_makes_the_loader_raise(tmp_path):
    """The loader's reading of the header (capi._prototypes, what the import and lib() use): a declaration whose parameter is none
    of pointer, array, uint32_t, uint64_t, int, float is named and nothing is guessed; neither is a declaration skipped whose
    parameter list it cannot split (parentheses of its own)"""
    text = open(os.path.join(ROOT, "include", "todhip.h")).read()
    old = "int todhip_set_ratio_test(todhip_ctx*, float ratio);"
    assert text.count(old) == 1
    assert capi._prototypes(capi.HEADER_PATH) == capi._PROTOTYPES and list(capi._PROTOTYPES) == capi.EXPORTS
    altered = tmp_path / "todhip.h"
    for new in ("int todhip_set_ratio_test(todhip_ctx*, double ratio);", "int todhip_set_ratio_test(todhip_ctx*, todhip_verify_params p);",
                "int todhip_set_ratio_test(todhip_ctx*, float (*ratio)(void));"):
        altered.write_text(text.replace(old, new))
        with pytest.raises(RuntimeError, match="todhip_set_ratio_test"):
            capi._prototypes(str(altered))


def test_struct_layouts_match_header():
    assert ctypes.sizeof(capi.Pose) == 4 + 36 + 12 + 8
    assert capi.DMATCH_DTYPE.itemsize == 16          # == sizeof(cv::DMatch)
    assert ctypes.sizeof(capi.Rng) == 144               # 33 x u32, 4 pad, u64
    assert ctypes.sizeof(capi.VerifyParams) == 12


def test_no_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(capi.TodError):
        capi.Context(0)


def test_product_does_not_reference_oracle():
    """The product path must never route through the CPU oracle."""
    for dirpath, _, files in os.walk(os.path.join(ROOT, "tod_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".hpp")):
                src = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "oracle" not in src.lower(), f


def test_header_is_plain_c():
    """The boundary is a C ABI: include/todhip.h must compile as C99 (no C++ types in the signatures)."""
    import subprocess, tempfile
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write('#include "todhip.h"\nint main(void) { todhip_rng r; todhip_rng_seed(&r, 1); return 0; }\n')
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-c", src, "-o", os.path.join(d, "t.o")], check=True)
