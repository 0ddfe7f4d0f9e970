"""The binding of include/todhip_ratio_other.h without a GPU, as tests/test_abi.py and tests/test_capi_marshal_cpu.py check the binding
of include/todhip.h: the library exports every function the header declares, the loader's argtypes and restype are the header's text
read by this file's own parser, a wrong kind of argument is refused at the call, and every wrapper marshals what the header declares
-- a stand-in takes the place of the loaded library, checks count and kind of the arguments against the real prototype and records
the name; the recorded names must be all of the header's."""
import ctypes as C
import inspect
import os
import re

import pytest

from tod_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int": C.c_int, "float": C.c_float}
D = 0x7F0000001000                                            # a device pointer as tensor.data_ptr() gives it: never read here


def _code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "todhip_ratio_other.h")).read(), flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(todhip_[a-z_0-9]+)\s*\(", _code())))


def test_library_exports_every_declared_symbol_with_the_headers_prototype():
    L = capi.lib()
    names = _declared()
    assert len(names) == 4 and sorted(capi.RATIO_OTHER_EXPORTS) == names
    assert not set(names) & set(capi.EXPORTS)                 # declared once: here, not in todhip.h's own text
    for name in names:
        m = re.search(r"(\w+)\s*(\*?)\s*\b%s\s*\((.*?)\)\s*;" % name, _code(), flags=re.S)
        assert m and m.group(1) == "int" and not m.group(2), name
        argtypes = [C.c_void_p if "*" in p or "[" in p else SCALARS[p.replace("const ", "").split()[0]] for p in m.group(3).split(",")]
        f = getattr(L, name)
        assert list(f.argtypes) == argtypes and f.restype is C.c_int, name
    assert L.todhip_set_ratio_test_other.argtypes == [C.c_void_p, C.c_float]
    assert L.todhip_other_object_min_device.argtypes == [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    import numpy as np
    with pytest.raises(C.ArgumentError):
        L.todhip_other_object_min_device(None, np.uint64(1 << 40), 1, None, None, 0, None)     # the header says a pointer
    with pytest.raises(C.ArgumentError):
        L.todhip_ratio_other_device(None, None, 1.5, 0.8, 2, None, None)                        # a float for nq


def test_every_wrapper_marshals_what_the_header_declares(monkeypatch):
    real, called = capi.lib(), []

    class StandIn:
        pass
    s = StandIn()
    for name in capi.RATIO_OTHER_EXPORTS:
        def call(*args, _name=name, _argtypes=list(getattr(real, name).argtypes)):
            assert len(args) == len(_argtypes), "%s takes %d arguments, got %d" % (_name, len(_argtypes), len(args))
            for i, (t, a) in enumerate(zip(_argtypes, args)):
                try:
                    t.from_param(a)
                except (TypeError, C.ArgumentError) as e:
                    raise AssertionError("%s, argument %d: %r is no %s (%s)" % (_name, i + 1, a, t.__name__, e))
            called.append(_name)
            return 0
        setattr(s, name, call)
    monkeypatch.setattr(capi, "_lib", s)
    ctx = capi._Borrowed(1)
    done = set()
    for name, args in (("other_object_min_device", (D, 2, D, D)), ("other_object_min_device", (D, 2, D, D, D, 44)),
                       ("other_object_min_device", (D, 2, D, D, None, 0xFFFFFFFF)), ("ratio_other_apply_device", (0.8, 2, 2, D, D, D)),
                       ("ratio_other_device", (D, 2, 0.8, 2, D, D)), ("set_ratio_test_other", (0.8,)), ("set_ratio_test_other", (0,))):
        getattr(ctx, name)(*args)
        done.add(name)
    public = {n for n, f in vars(capi._RatioOtherCalls).items() if not n.startswith("_") and inspect.isfunction(f)}
    assert done == public and issubclass(capi.Context, capi._RatioOtherCalls)
    assert set(called) == set(capi.RATIO_OTHER_EXPORTS)
    with pytest.raises(AssertionError):
        ctx.ratio_other_device(D, 2.5, 0.8, 2, D, D)          # the stand-in refuses what ctypes would
