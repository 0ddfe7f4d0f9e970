"""The float matcher's launch plan (tod_amd/csrc/l2_plan.h) without a GPU: a stand-alone host program, built with
-fsanitize=address,undefined, compares every field of l2_plan, the buffer sizes included, with the expressions of tod_l2_db_prepare,
l2_pass_begin and l2_keys as they stood, and checks that the chunks cover the DB, none is empty, the sample lies inside the DB and the
counter array covers what the query preparation zeroes (tests/l2_plan_host_test.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_equals_the_old_inline_expressions(tmp_path):
    exe = str(tmp_path / "l2_plan_host_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tod_amd", "csrc"),
                    os.path.join(ROOT, "tests", "l2_plan_host_test.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    # DB sizes x query counts x k x CU counts x (knobs unset, chunk rounds 3, sample tiles 512, seed chunks 7 and 10^6, no candidates)
    assert int(out.stdout) == 18 * 6 * 8 * 4 * 6
