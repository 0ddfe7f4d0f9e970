"""The layout and the bit assignment of the resident fp4 copy of the DB rows (tod_amd/csrc/fp4_rows.h) without a GPU: a stand-alone host
program, built with -fsanitize=address,undefined, checks every (row, bit) of 32, 33, 63 and 4113 rows against the definition
(tests/fp4_rows_host_test.cpp). That the device's expand_word writes the same copy is the GPU test's business
(tests/test_match_fp4_rows_gpu.py: bit for bit the vector engine's matches)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_bit_of_the_fp4_copy_is_where_the_layout_says(tmp_path):
    exe = str(tmp_path / "fp4_rows_host_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tod_amd", "csrc"),
                    os.path.join(ROOT, "tests", "fp4_rows_host_test.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    padded = sum((n + 31) // 32 * 32 for n in (32, 33, 63, 4113))            # whole steps: the rows past the end are expanded too
    assert int(out.stdout) == padded * 256
