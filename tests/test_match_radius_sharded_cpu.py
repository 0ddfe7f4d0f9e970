"""The radius search over a sharded DB without a GPU: the identity the device merge rests on (the merge of what the shards send
equals the unsharded search) in numpy, the boundary (exports, C signatures, bindings, the header's advice), and
tod_amd/sharded.py::ShardedMatcher(max_per_query=...) over gloo with the numpy functions as its compute."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import match_radius_ref as R
import sharded_radius_ref as S
from tod_amd import capi, sharded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("queryIdx", "trainIdx", "imgIdx", "distance")
WORLDS = (1, 2, 3, 4, 8)


def same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), what
    for f in FIELDS:
        assert np.array_equal(got[1][f], want[1][f]), (what, f)
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), what


def shards_of(off, world):
    return [np.arange(lo, hi) for _, _, lo, hi in (sharded.shard_bounds(off, r, world) for r in range(world))]


def test_the_db_is_cut_where_the_cases_need_it():
    _, off, _, _ = S.make_db()
    assert int(off[-1]) == 1059
    cuts = {w: [int(s[0]) if len(s) else None for s in shards_of(off, w)][1:] for w in WORLDS}
    assert cuts[2] == [590] and cuts[3] == [590, 922]
    assert all(len(s) > 0 for s in shards_of(off, 4))
    assert sorted(len(s) > 0 for s in shards_of(off, 8)) == [False] * 2 + [True] * 6
    assert (S.TIE_ROWS < 590).sum() == 195 and (S.TIE_ROWS >= 590).sum() == 105


@pytest.mark.parametrize("world", WORLDS)
def test_merge_of_the_shards_answers_equals_the_unsharded_search(world):
    """the identity: every case has hits; the over-full ones cut inside the 300-way tie that straddles the boundary at row 590"""
    desc, off, pts, q = S.make_db()
    rows = shards_of(off, world)
    assert sum(len(r) for r in rows) == len(desc)
    n_over = 0
    for radius in (1, 35, 128, 256):
        for mpq in (1, 5, 64, 1024):
            want = R.match_radius(desc, off, pts, q, radius, mpq)
            keys = np.stack([S.shard_keys(desc, off, pts, q, radius, mpq, r) for r in rows])
            assert keys.shape == (world, len(q), mpq + 1)
            same(S.merge(keys, off, pts, mpq), want, (world, radius, mpq))
            assert int(want[0][-1]) > 0
            n_over += bool((want[3] > mpq).any())
            if mpq < 300:                                   # the tie is cut: lowest rows first, over the shard boundary when it reaches it
                got = (off[want[1]["imgIdx"]].astype(np.int64) + want[1]["trainIdx"])[:want[0][1]]
                assert list(got) == ([100] + list(S.TIE_ROWS))[:mpq]
    assert n_over == 13                                     # all 16 but max_per_query 1024 at radius 1, 35 and 128 (301, 301 and about 550 rows inside)


# ---------------------------------------------------------------------------------------------------- the boundary
SIGNATURES = {
    "todhip_match_radius_shard_device": "todhip_ctx*, const void*, uint32_t, uint32_t, uint32_t, void*",
    "todhip_merge_radius_shards_device": "todhip_ctx*, const void*, uint32_t, uint32_t, uint32_t, void*, void*, void*, void*",
    "todhip_merge_radius_shards_device_on": "todhip_ctx*, void*, const void*, uint32_t, uint32_t, uint32_t, void*, void*, void*, void*",
}
NAMES = {
    "todhip_match_radius_shard_device": ["", "d_q_desc", "nq", "radius", "max_per_query", "d_keys"],
    "todhip_merge_radius_shards_device": ["", "d_keys_all", "n_shards", "nq", "max_per_query", "d_counts", "d_matches", "d_matches_xyz",
                                          "d_in_radius"],
    "todhip_merge_radius_shards_device_on": ["", "hip_stream", "d_keys_all", "n_shards", "nq", "max_per_query", "d_counts", "d_matches",
                                             "d_matches_xyz", "d_in_radius"],
}


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "todhip.h")).read(), flags=re.S)


def _header_params(name):
    """[(type, parameter name)] of a function as include/todhip.h declares it"""
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, _header_text())
    assert m, name + " is not declared in include/todhip.h"
    out = []
    for p in m.group(1).split(","):
        t = re.match(r"\s*(.*?[\s*])([a-z_0-9]*)\s*$", p, flags=re.S)
        out.append((t.group(1).strip(), t.group(2)))
    return out


def test_library_exports_the_three_entry_points():
    L = capi.lib()
    for name in SIGNATURES:
        assert hasattr(L, name), "libtodhip.so does not export " + name
        assert name in capi.EXPORTS


def test_header_declares_the_expected_c_signatures():
    """assigning the functions to pointers of the expected type compiles without a warning only when the header's parameter types
    and order are these"""
    lines = ['#include "todhip.h"'] + ["int (*p_%s)(%s) = %s;" % (n, sig, n) for n, sig in SIGNATURES.items()]
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write("\n".join(lines) + "\n")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-c", src, "-o", os.path.join(d, "t.o")], check=True)
    for name in SIGNATURES:
        assert [n for _, n in _header_params(name)] == NAMES[name]


def test_capi_binds_them_in_the_headers_argument_order():
    L = capi.lib()
    for name in SIGNATURES:
        want = [C.c_void_p if "*" in t else {"uint32_t": C.c_uint32}[t] for t, _ in _header_params(name)]
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == want, name
    for name in ("match_radius_shard_device", "merge_radius_shards_device", "merge_radius_shards_device_on"):
        assert callable(getattr(capi.Context, name))


def test_header_points_to_the_device_merge():
    text = open(os.path.join(ROOT, "include", "todhip.h")).read()
    assert "concatenating and sorting" not in text
    assert "inside the union of the" in " ".join(text.split()) and "per-shard first max_per_query" in " ".join(text.split())


# ---------------------------------------------------------------------------------------------------- the choreography over gloo
NQ, B, STEPS, RADIUS = 12, 2, 4, 35


def _worker(rank, world, port, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        desc, off, pts, _ = S.make_db()
        _, _, row_lo, row_hi = sharded.shard_bounds(off, rank, world)
        rows = np.arange(row_lo, row_hi)
        # frame (step, rank, b): every step shows other queries, so a stale buffer cannot go unnoticed
        frames = {(i, b): S.make_queries(desc, NQ, 1000 * i + 10 * rank + b) for i in range(STEPS) for b in range(B)}
        ok, logs, n_matches, n_over = True, [], 0, 0
        for mpq in (5, 64):
            want = {(i, b): R.match_radius(desc, off, pts, frames[(i, b)], RADIUS, mpq) for i in range(STEPS) for b in range(B)}
            for exchange in ("all_to_all", "all_gather"):
                for overlap in (True, False):
                    ops = sharded.HostOps(
                        dist, lambda q_all: torch.from_numpy(S.shard_keys(desc, off, pts, q_all.numpy(), RADIUS, mpq, rows).view(np.int64)),
                        lambda keys_mine: S.merge(keys_mine.numpy(), off, pts, mpq), two_streams=overlap)
                    sm = sharded.ShardedMatcher(ops, world, rank, B, NQ, 2, exchange=exchange, overlap=overlap, max_per_query=mpq)
                    assert sm.overlap == overlap and sm.keys[0].shape == (world * B * NQ, mpq + 1)
                    sm.begin(STEPS, lambda i: (torch.from_numpy(np.stack([frames[(i, b)] for b in range(B)])), None))
                    for i in range(STEPS):
                        out = {}
                        sm.step(i, out)
                        rp, m, xyz, in_radius = out["result"]   # B * NQ queries: frame b owns [b * NQ, (b + 1) * NQ)
                        for b in range(B):
                            w = want[(i, b)]
                            lo, hi = int(rp[b * NQ]), int(rp[(b + 1) * NQ])
                            mine = m[lo:hi].copy()
                            mine["queryIdx"] -= b * NQ
                            ok = ok and np.array_equal(rp[b * NQ:(b + 1) * NQ + 1] - rp[b * NQ], w[0])
                            ok = ok and all(np.array_equal(mine[f], w[1][f]) for f in FIELDS)
                            ok = ok and np.array_equal(xyz[lo:hi], w[2]) and np.array_equal(in_radius[b * NQ:(b + 1) * NQ], w[3])
                            n_matches += hi - lo
                            n_over += int((w[3] > mpq).sum())
                    logs.append(list(ops.log))
        ret[rank] = (bool(ok), n_matches, n_over, logs)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_matcher_radius_steps_equal_unsharded(world):
    """max_per_query 5 and 64, both exchanges, overlapped and serial, 4 steps each, in one process group per world"""
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, 29560 + world, ret), nprocs=world, join=True)
    assert len(ret) == world
    for r in range(world):
        ok, n_matches, n_over, logs = ret[r]
        assert ok, "rank %d differs from the unsharded result" % r
        assert n_matches > 8 * STEPS * B * 5 and n_over > 0
        assert logs == ret[0][3], "rank %d issued its collectives in another order than rank 0" % r
    logs = ret[0][3]
    assert len(logs) == 8
    for n_log, mpq in zip(range(0, 8, 4), (5, 64)):
        a2a, ag = logs[n_log], logs[n_log + 2]                 # overlapped all-to-all, overlapped all-gather
        assert a2a.count("all_to_all%d" % (world * B * NQ * (mpq + 1))) == STEPS     # one collective per exchange, rows mpq + 1 wide
        assert ag.count("all_gather%d" % (world * B * NQ * (mpq + 1))) == STEPS
        assert [w for w in a2a if w.startswith("all_gather")] == ["all_gather%d" % (B * NQ * 32)] * STEPS
        assert a2a[:2] == ["all_gather%d" % (B * NQ * 32)] * 2                       # the descriptor gather runs one step ahead
