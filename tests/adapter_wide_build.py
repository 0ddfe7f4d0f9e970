"""Builds tests/adapter_wide_test.cpp (the DescriptorMatcher cell on 64-byte descriptors against the mini_ecto test double), as
tests/test_adapter.py builds adapter_test.cpp. Shared by test_match_wide_cpu.py and test_adapter_wide.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "adapter_wide_test")
SRC = os.path.join(ROOT, "tests", "adapter_wide_test.cpp")


def build():
    deps = [SRC, os.path.join(ROOT, "adapter", "ecto_cells.hpp"), os.path.join(ROOT, "include", "todhip.h")]
    if os.path.exists(EXE) and os.path.getmtime(EXE) >= max(os.path.getmtime(f) for f in deps):
        return EXE
    cmd = ["g++", "-std=c++11", "-O1", "-Wall", "-o", EXE, SRC, "-L" + os.path.join(ROOT, "tod_amd"), "-ltodhip",
           "-Wl,-rpath," + os.path.join(ROOT, "tod_amd"), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True)
    return EXE
