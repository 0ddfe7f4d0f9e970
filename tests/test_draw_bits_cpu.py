"""The lane-per-position draw table's bit arithmetic without a GPU (tests/draw_bits_host_test.cpp): a stand-alone host program, built
with -fsanitize=address,undefined, compares nth_set_bit, count_bits and clear_bit of tod_amd/csrc/verify_draw_bits.h at 2 and 8
words with a bit-by-bit walk: every n below the popcount for words that are empty, full, bit 0 or bit 63 alone, or random; the
target in the first word, in the last, and behind empty predecessors."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_nth_set_bit_equals_the_bit_by_bit_walk(tmp_path):
    exe = str(tmp_path / "draw_bits_host_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tod_amd", "csrc"),
                    os.path.join(ROOT, "tests", "draw_bits_host_test.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    selections, removals = (int(x) for x in out.stdout.split())
    # every set bit of every case is selected once by its rank and removed once; 4000 eight-word cases of ~200 bits are the bulk
    assert selections == removals and selections > 500000
