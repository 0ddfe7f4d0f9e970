"""The host side of todhip_set_db_bit_order without a GPU: tod_amd/csrc/db_bitorder.h (plain C++) is compiled into a stand-alone
driver (tests/bit_order_host_test.cpp) with the host compiler and -fsanitize=address,undefined, run as its own process on
statistics files, and compared with the definition restated in tests/bit_order_ref.py. Statistics come from real 0/1 matrices, so the
header's u64 bounds (v <= 2^30, c^2 <= v[a] v[b]) are what the library meets too."""
import os
import subprocess

import numpy as np
import pytest

import bit_order_ref as R
from tod_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bit_order") / "bit_order_host_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tod_amd", "csrc"),
                    os.path.join(ROOT, "tests", "bit_order_host_test.cpp"), "-o", exe], check=True)
    return exe


def run_driver(exe, tmp_path, S, ones, both):
    path = str(tmp_path / "stats.txt")
    with open(path, "w") as f:
        f.write("%d\n" % S)
        f.write(" ".join(str(int(x)) for x in ones) + "\n")
        np.savetxt(f, np.asarray(both, np.int64), fmt="%d")
    out = subprocess.run([exe, path], check=True, capture_output=True, text=True)
    assert out.stderr == ""                                   # no sanitizer report
    rank, src_of = [np.array([int(x) for x in line.split()]) for line in out.stdout.strip().split("\n")]
    return rank, src_of


def bits_random(rng, S):
    """biased bits (p from 0.02 to 0.98), some of them noisy copies of others (correlations either side of 1/2)"""
    X = (rng.random((S, 256)) < np.linspace(0.02, 0.98, 256)[rng.permutation(256)]).astype(np.uint8)
    for b, a, flip in ((10, 200, 0.05), (11, 200, 0.20), (12, 200, 0.30), (77, 3, 0.25), (78, 3, 0.26), (140, 141, 0.10)):
        X[:, b] = X[:, a] ^ (rng.random(S) < flip)
    return X


def bits_constant(rng, S):
    return np.tile((rng.random(256) < 0.5).astype(np.uint8), (S, 1))


def bits_duplicates(rng, S):
    X = (rng.random((S, 256)) < 0.5).astype(np.uint8)
    X[:, 128:192] = X[:, 0:64]                                # exact copies ...
    X[:, 192:256] = 1 - X[:, 64:128]                          # ... and exact complements: |correlation| = 1
    return X


def bits_ties(rng, S):
    """every bit set in exactly S / 2, S / 4 or 3 S / 4 rows: two values of v, ties broken by the index alone"""
    X = np.zeros((S, 256), np.uint8)
    for b in range(256):
        X[rng.permutation(S)[:(S // 2, S // 4, 3 * S // 4)[b % 3]], b] = 1
    return X


def bits_full_sample(rng, S):
    """S = 65536 with the extreme counts: exact halves that are exactly independent (the 16 bits of the row index), their
    complements and copies (c = 2^30, 4 c^2 = 2^62 = 4 v v), counts 1, S - 1, 0 and S"""
    assert S == 65536
    i = np.arange(S)
    X = (rng.random((S, 256)) < 0.5).astype(np.uint8)
    for b in range(16):
        X[:, b] = (i >> b) & 1
        X[:, 16 + b] = 1 - X[:, b]
        X[:, 32 + b] = X[:, b]
    X[:, 48] = i == 0
    X[:, 49] = i != 0
    X[:, 50] = 0
    X[:, 51] = 1
    return X


CASES = [("random", bits_random, 1000), ("random-odd", bits_random, 77), ("constant", bits_constant, 300),
         ("duplicates", bits_duplicates, 4096), ("ties", bits_ties, 64), ("one-row", bits_random, 1),
         ("two-rows", bits_random, 2), ("full-sample", bits_full_sample, 65536)]


@pytest.mark.parametrize("name,make,S", CASES, ids=[c[0] for c in CASES])
def test_host_order_equals_the_definition(driver, tmp_path, name, make, S):
    rng = np.random.default_rng(len(name) * 1000 + S)
    S_, ones, both = R.stats_of_bits(make(rng, S))
    rank, src_of = run_driver(driver, tmp_path, S_, ones, both)
    want_rank, want_src = R.order_from_stats(S_, ones, both)
    assert sorted(rank.tolist()) == list(range(256)) and sorted(src_of.tolist()) == list(range(256))
    assert rank.tolist() == want_rank
    assert np.array_equal(src_of, want_src)
    v = ones * (S_ - ones)
    if name in ("constant", "one-row"):                       # nothing varies: everything rejected, candidate order by index
        assert rank.tolist() == list(range(256))
    if name == "duplicates":                                  # the second of each pair is rejected: 128 accepted at the most
        assert set(rank[:128].tolist()) == set(range(128))
    if name == "ties":
        assert len(set(v.tolist())) == 2
    if name == "full-sample":
        assert v.max() == 2 ** 30 and set(rank[-2:].tolist()) == {50, 51}
        first = rank.tolist().index
        assert all(first(b) < first(16 + b) and first(b) < first(32 + b) for b in range(16))


def test_layout_follows_the_matrix_engines_evaluation_order():
    """rank r sits at position 32 E[r // 32] + r % 32: ranks 0-63 in dwords 0 and 4, 64-127 in dwords 1 and 5, ..."""
    _, src_of = R.order_from_stats(1, [0] * 256, np.zeros((256, 256), np.int64))   # rank = identity
    pos_of_rank = np.argsort(src_of)
    assert [int(pos_of_rank[32 * g]) // 32 for g in range(8)] == [0, 4, 1, 5, 2, 6, 3, 7]


def test_null_pointers_are_refused_without_a_device():
    L = capi.lib()
    buf = np.zeros(256, np.uint8)
    assert L.todhip_set_db_bit_order(None, 1) == capi.EINVAL
    assert L.todhip_db_bit_order(None, buf.ctypes.data) == capi.EINVAL
