"""The packing of two split blocks into one f32 accumulator (tod_amd/csrc/match_pair_pack.h) without a GPU: a stand-alone host program,
built with -fsanitize=address,undefined, emulates magic + dA + 2048 dB in `float` for every cut in 1 .. 64 and every even dA, dB in
[-128, 128] and checks that the sum is exact, that bit 9 is set exactly when dA > thrp and bit 20 exactly when dB > thrp, that no other
bit of the mask and no neighbouring bit is ever set, and that the fields unpack to dA and dB (tests/pair_pack_host_test.cpp). That the
matrix cores compute the same sum is the GPU test's business (tests/test_match_pairs_gpu.py) and tools/mfma_valu_overlap.hip's."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_pair_of_dot_products_packs_exactly_and_flags_its_threshold(tmp_path):
    exe = str(tmp_path / "pair_pack_host_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tod_amd", "csrc"),
                    os.path.join(ROOT, "tests", "pair_pack_host_test.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    assert int(out.stdout) == 64 * 129 * 129
