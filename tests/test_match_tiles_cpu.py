"""The tile size and the launch plan of the matrix-core searches (tod_amd/csrc/match_tiles.h) without a GPU: a stand-alone host
program, built with -fsanitize=address,undefined, compares mfma_tile_rows with the expressions of the three launchers it replaced
and tile_plan with finish_tiling's, launch_wide's and launch_collect's as they stood (tests/match_tiles_host_test.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tile_rows_equal_the_three_launchers_old_expressions(tmp_path):
    exe = str(tmp_path / "match_tiles_host_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tod_amd", "csrc"),
                    os.path.join(ROOT, "tests", "match_tiles_host_test.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    assert int(out.stdout) == 70000 * (1 + 18 * 7) * 2                      # each tile size, then the plan it gives
