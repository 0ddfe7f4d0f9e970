"""Stage A's table- and word-based arithmetic without a GPU (tests/orb_diet_host_test.cpp): a stand-alone host program, built with
-fsanitize=address,undefined, compares resize_taps (tod_amd/csrc/orb_plan.h) with the per-pixel expressions of the resize, compass4
(orb_compass.h) with fast_compass position by position, and row_moments (orb_moments.h) with the byte loop of patch_moments.
-ffp-contract=off as in the library's build: the resize's float expressions must stay as written."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tables_and_words_equal_the_per_pixel_forms(tmp_path):
    exe = str(tmp_path / "orb_diet_host_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tod_amd", "csrc"),
                    os.path.join(ROOT, "tests", "orb_diet_host_test.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    taps, positions, rows = (int(x) for x in out.stdout.split())
    assert taps == 533 + 444 + 400 + 333 + 1600 + 900 + 7 + 8 + 53 + sum(src - 1 for src in range(8, 81))
    # 256 centres x 10^4 ring combinations and 10^6 random windows, four positions each; 200 staged tiles of 66 x 18 positions
    assert positions == 4 * (256 * 10 ** 4 + 10 ** 6) + 200 * 66 * 18
    assert rows == (2000 + 2) * 31
