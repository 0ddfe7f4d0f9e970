"""The plain C++ of fast_nms_kernel's score and survivor list without a GPU (tests/orb_nms_host_test.cpp): a stand-alone host program,
built with -fsanitize=address,undefined, compares fast_score_pairs (tod_amd/csrc/orb_arc.h: both polarities from one sliding minimum
and one sliding maximum over 16-bit pairs) with the score's definition arc by arc, and walks nms_entry over every position of a tile."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_packed_score_and_list_entries_equal_their_definitions(tmp_path):
    exe = str(tmp_path / "orb_nms_host_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tod_amd", "csrc"),
                    os.path.join(ROOT, "tests", "orb_nms_host_test.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    rings, entries = (int(x) for x in out.stdout.split())
    # 256 centres x (arcs of 7..16 pixels x 16 starts x 6 contrasts x 2 polarities + 3 constant rings) and 10^6 random rings
    assert rings == 256 * (10 * 16 * 6 * 2 + 3) + 10 ** 6
    assert entries == 66 * 18
