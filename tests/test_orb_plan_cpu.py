"""Stage A's launch plan (tod_amd/csrc/orb_plan.h) without a GPU: a stand-alone host program, built with
-fsanitize=address,undefined, compares OrbPlan field by field with the expressions of orb.hip it replaced (the pyramid's level table,
the argument checks, the buffer capacities, the control block's layout, every grid extent) over a sweep of geometries, and asserts
the documented rules of the level table and of the statuses, check_pattern included: which points it refuses, and that a point it
accepts stays within 30 pixels of the keypoint when steered in float (tests/orb_plan_host_test.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_equals_the_expressions_it_replaced(tmp_path):
    exe = str(tmp_path / "orb_plan_host_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tod_amd", "csrc"),
                    os.path.join(ROOT, "tests", "orb_plan_host_test.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    plans, refused = (int(x) for x in out.stdout.split())
    sweep = 13 * 13 * 7 * 6 * 5 * 5 * 3                                     # H, W, n_levels, scale_factor, n_features, F, cap
    # accepted: both sides >= 8, a factor > 1, features, the 11 (n_levels in 1..16, F) pairs within 65535, a capacity
    assert plans == 12 * 12 * 5 * 4 * 11 * 2 + 5 * 2                        # and 5 of the 10 n_levels * F cases, two capacities each
    assert plans + refused == sweep + 10 * 3
