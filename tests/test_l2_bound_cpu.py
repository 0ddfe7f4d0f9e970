"""The float matcher's filter bound (tod_amd/csrc/l2_bound.h: the bf16 rounding and eps(q)) without a GPU: a stand-alone host program,
built with -fsanitize=address,undefined, holds |score + |q|^2 - d2| <= eps(q) and the differential form the k-NN threshold needs
against extended precision on worst-case families and seeded random cases (tests/l2_bound_host_test.cpp). The same program with eps
as it stood before the correction must FAIL on the worst-case families: that is what makes them worst cases."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_host_test(exe):
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tod_amd", "csrc"),
                    os.path.join(ROOT, "tests", "l2_bound_host_test.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_host_test(str(tmp_path_factory.mktemp("l2_bound") / "l2_bound_host_test"))


LINE = re.compile(r"(worst-case families|random cases): (\d+) pairs, (\d+) ordered row pairs, \(a\) fails (\d+), \(b\) fails (\d+), "
                  r"largest \|error\| / eps ([0-9.]+), largest differential error / 2 eps ([0-9.]+)")


def parse(stdout):
    rows = {m.group(1): (int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5)), float(m.group(6)), float(m.group(7)))
            for m in map(LINE.match, stdout.splitlines()) if m}
    assert set(rows) == {"worst-case families", "random cases"}, stdout
    return rows["worst-case families"], rows["random cases"]


def test_the_bound_holds_and_is_tight(exe):
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    worst, rnd = parse(out.stdout)
    assert worst[0] == 8820 and rnd[0] == 4800                               # pairs: the families' sweep, 600 random cases of 8 rows
    assert worst[2:4] == (0, 0) and rnd[2:4] == (0, 0)                       # (a), (b)
    assert 0.9 < worst[4] <= 1.0 and 0.9 < worst[5] <= 1.0                   # (c): single-row and differential
    assert rnd[4] < worst[4]                                                 # random roundings cancel: never the binding case


def test_the_constant_before_the_correction_fails_on_the_worst_cases(exe):
    """2^-7 (1 + 2^-6) |q| Rmax + 2^-14 (|q| + Rmax)^2 allowed half the error bf16 rounding can make."""
    out = subprocess.run([exe, "--old-constant"], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 1 and "(a) fails" in out.stderr and "(b) fails" in out.stderr, out.stdout + out.stderr
    worst, rnd = parse(out.stdout)
    assert worst[2] > 0 and worst[3] > 0 and 1.8 < worst[4] < 2.0 and 1.8 < worst[5] < 2.0
    assert rnd[2:4] == (0, 0)                                                # which is why no test on random data ever noticed


def test_eps_flag_prints_the_library_formula(exe):
    out = subprocess.run([exe, "--eps", "1", "1", "4", "9"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = [float.fromhex(s) for s in out.stdout.split()]
    assert got[0] == 2.0 ** -6 * (1 + 2.0 ** -6) + 2.0 ** -14 * 4            # exact in binary32
    assert got[1] == 2.0 ** -6 * (1 + 2.0 ** -6) * 6 + 2.0 ** -14 * 25
