"""The float searches over a sharded DB without a GPU: the identity the device merges rest on (the merge of what the shards send
equals the unsharded search: the oracle's k-NN, tests/match_l2_radius_ref.py's radius search) in numpy, the boundary (exports, C
signatures, bindings), and tod_amd/sharded.py::ShardedMatcher(desc_bytes=512) over gloo with the numpy functions as its compute."""
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

import l2_sharded_ref as S
import match_l2_radius_ref as R
import oracle_lib as O
from tod_amd import capi, sharded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("queryIdx", "trainIdx", "imgIdx", "distance")
WORLDS = (1, 2, 3, 8)


def same(got, want, what=""):
    assert len(got) == len(want)
    assert np.array_equal(got[0], want[0]), what
    for f in FIELDS:
        assert np.array_equal(got[1][f], want[1][f]), (what, f)
    for a, b in zip(got[2:], want[2:]):
        assert np.array_equal(a, b), what


def shards_of(off, world):
    return [np.arange(lo, hi) for _, _, lo, hi in (sharded.shard_bounds(off, r, world) for r in range(world))]


@pytest.fixture(scope="module")
def db():
    desc, off, pts, q = S.make_db()
    return desc, off, pts, q, R.d2(desc, q)


def test_the_db_is_cut_where_the_cases_need_it(db):
    desc, off, _, q, dd = db
    assert int(off[-1]) == 1059 and 280 <= len(S.TIE_ROWS) <= 300 and S.TIE_SRC not in S.TIE_ROWS
    for world in WORLDS:
        rows = shards_of(off, world)
        assert sum(len(r) for r in rows) == 1059
        assert all(np.isin(S.TIE_ROWS, r).sum() >= 8 for r in rows if len(r) > 32)       # a full list of ties in every real shard
    assert sorted(len(r) > 0 for r in shards_of(off, 8)) == [False] * 2 + [True] * 6    # empty shards among them
    assert (dd[0::6] .min(axis=1) == 0).all() and (dd[0::3].min(axis=1) == 0).all()     # exact copies: d2 = 0
    assert ((dd[0::6] == 0).sum(axis=1) == len(S.TIE_ROWS) + 1).all()                   # ... every other one of them of the tie's row
    lo, on, mid, far = S.radii(desc, q)
    tie = np.sqrt(dd[1, S.TIE_ROWS])
    assert (tie == np.float32(on)).all() and lo < on and (np.sqrt(dd[1]) >= np.float32(on)).all()
    assert 0 < (np.sqrt(dd) <= np.float32(mid)).sum() < dd.size / 2 and np.sqrt(dd).max() < far


@pytest.mark.parametrize("world", WORLDS)
def test_merge_of_the_shards_knn_keys_equals_the_oracle(db, world):
    desc, off, pts, q, dd = db
    rows = shards_of(off, world)
    n_cut = n_full = 0
    for k in (1, 2, 5, 8):
        keys = np.stack([S.shard_keys_knn(desc, off, q, k, r, dd) for r in rows])
        assert keys.shape == (world, len(q), k)
        for r, ks in zip(rows, keys):
            assert ((ks != S.PAD).sum(axis=1) == min(k, len(r))).all()
        for radius in S.radii(desc, q):
            rc, rp, m, xyz = O.l2_match(desc, off, pts, q, k, radius)
            assert rc == 0
            same(S.merge_knn(keys, off, pts, k, radius), (rp, m, xyz), (world, k, radius))
            n_cut += int((np.diff(rp.astype(np.int64)) < k).sum())
            n_full += int((np.diff(rp.astype(np.int64)) == k).sum())
        # the tie is cut by k: lowest rows first, over the shard boundaries
        got = S.merge_knn(keys, off, pts, k, 1.0e9)
        mine = (off[got[1]["imgIdx"]].astype(np.int64) + got[1]["trainIdx"])[:got[0][1]]
        assert list(mine) == sorted(np.concatenate([[S.TIE_SRC], S.TIE_ROWS]))[:k]
    assert n_cut > 0 and n_full > 0


@pytest.mark.parametrize("world", WORLDS)
def test_merge_of_the_shards_radius_keys_equals_the_unsharded_search(db, world):
    desc, off, pts, q, dd = db
    rows = shards_of(off, world)
    n_over = n_under = 0
    for radius in S.radii(desc, q):
        for mpq in (1, 5, 64):
            want = R.match_l2_radius(desc, off, pts, q, radius, mpq, dd)
            keys = np.stack([S.shard_keys_radius(desc, off, q, radius, mpq, r, dd) for r in rows])
            assert keys.shape == (world, len(q), mpq + 1)
            same(S.merge_radius(keys, off, pts, mpq), want, (world, radius, mpq))
            n_over += int((want[3] > mpq).sum())
            n_under += int((want[3] < mpq).sum())
    assert n_over > 0 and n_under > 0


def test_a_shards_keys_do_not_depend_on_the_precomputed_distances(db):
    desc, off, pts, q, dd = db
    rows = shards_of(off, 3)[1]
    assert np.array_equal(S.shard_keys_knn(desc, off, q[:5], 5, rows), S.shard_keys_knn(desc, off, q[:5], 5, rows, dd[:5]))
    assert np.array_equal(S.shard_keys_radius(desc, off, q[:5], 900.0, 5, rows), S.shard_keys_radius(desc, off, q[:5], 900.0, 5, rows, dd[:5]))


# ---------------------------------------------------------------------------------------------------- the boundary
SIGNATURES = {
    "todhip_match_l2_shard_device": "todhip_ctx*, const void*, uint32_t, uint32_t, void*",
    "todhip_merge_l2_shards_device": "todhip_ctx*, const void*, uint32_t, uint32_t, uint32_t, float, void*, void*, void*",
    "todhip_merge_l2_shards_device_on": "todhip_ctx*, void*, const void*, uint32_t, uint32_t, uint32_t, float, void*, void*, void*",
    "todhip_match_l2_radius_shard_device": "todhip_ctx*, const void*, uint32_t, float, uint32_t, void*",
    "todhip_merge_l2_radius_shards_device": "todhip_ctx*, const void*, uint32_t, uint32_t, uint32_t, void*, void*, void*, void*",
    "todhip_merge_l2_radius_shards_device_on": "todhip_ctx*, void*, const void*, uint32_t, uint32_t, uint32_t, void*, void*, void*, void*",
}
NAMES = {
    "todhip_match_l2_shard_device": ["", "d_q_desc", "nq", "k", "d_keys"],
    "todhip_merge_l2_shards_device": ["", "d_keys_all", "n_shards", "nq", "k", "radius", "d_counts", "d_matches", "d_matches_xyz"],
    "todhip_merge_l2_shards_device_on": ["", "hip_stream", "d_keys_all", "n_shards", "nq", "k", "radius", "d_counts", "d_matches",
                                         "d_matches_xyz"],
    "todhip_match_l2_radius_shard_device": ["", "d_q_desc", "nq", "radius", "max_per_query", "d_keys"],
    "todhip_merge_l2_radius_shards_device": ["", "d_keys_all", "n_shards", "nq", "max_per_query", "d_counts", "d_matches", "d_matches_xyz",
                                             "d_in_radius"],
    "todhip_merge_l2_radius_shards_device_on": ["", "hip_stream", "d_keys_all", "n_shards", "nq", "max_per_query", "d_counts", "d_matches",
                                                "d_matches_xyz", "d_in_radius"],
}


def _header_params(name):
    """[(type, parameter name)] of a function as include/todhip.h declares it"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "todhip.h")).read(), flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, name + " is not declared in include/todhip.h"
    out = []
    for p in m.group(1).split(","):
        t = re.match(r"\s*(.*?[\s*])([a-z_0-9]*)\s*$", p, flags=re.S)
        out.append((t.group(1).strip(), t.group(2)))
    return out


def test_library_exports_the_six_entry_points():
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
        want = [C.c_void_p if "*" in t else {"uint32_t": C.c_uint32, "float": C.c_float}[t] for t, _ in _header_params(name)]
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == want, name
    for name in ("match_l2_shard_device", "merge_l2_shards_device", "match_l2_radius_shard_device", "merge_l2_radius_shards_device"):
        assert callable(getattr(capi.Context, name))


def test_header_states_the_definition():
    text = " ".join(open(os.path.join(ROOT, "include", "todhip.h")).read().replace("\n *", "\n").split())
    assert "(IEEE binary32 bits of d2) << 32 | row of the full DB" in text
    assert "stay TODHIP_EINVAL on a context that holds one shard of several" in text
    assert "(128 x f32 per row, one device)" in text          # the unsharded calls' paragraph stands as it was


# ---------------------------------------------------------------------------------------------------- the choreography over gloo
NQ, B, STEPS, K, MPQ = 9, 2, 3, 5, 64


def _worker(rank, world, port, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        desc, off, pts, q0 = S.make_db()
        _, on_tie, mid, _ = S.radii(desc, q0)
        _, _, row_lo, row_hi = sharded.shard_bounds(off, rank, world)
        rows = np.arange(row_lo, row_hi)
        # frame (step, rank, b): every step shows other queries, so a stale buffer cannot go unnoticed
        frames = {(i, b): S.make_queries(desc, NQ, 1000 * i + 10 * rank + b) for i in range(STEPS) for b in range(B)}
        floats = lambda t: np.ascontiguousarray(t.numpy()).view(np.float32).reshape(-1, 128)      # the queries travel as bytes
        ok, logs, n_matches = True, [], 0
        for mpq, radius in ((None, mid), (MPQ, on_tie)):
            if mpq is None:
                want = {key: O.l2_match(desc, off, pts, f, K, radius)[1:] for key, f in frames.items()}
                shard = lambda q_all: torch.from_numpy(S.shard_keys_knn(desc, off, floats(q_all), K, rows).view(np.int64))
                merge = lambda keys_mine: S.merge_knn(keys_mine.numpy(), off, pts, K, radius)
            else:
                want = {key: R.match_l2_radius(desc, off, pts, f, radius, mpq) for key, f in frames.items()}
                shard = lambda q_all: torch.from_numpy(S.shard_keys_radius(desc, off, floats(q_all), radius, mpq, rows).view(np.int64))
                merge = lambda keys_mine: S.merge_radius(keys_mine.numpy(), off, pts, mpq)
            width = K if mpq is None else mpq + 1
            for exchange in ("all_to_all", "all_gather"):
                for overlap in (True, False):
                    ops = sharded.HostOps(dist, shard, merge, two_streams=overlap)
                    sm = sharded.ShardedMatcher(ops, world, rank, B, NQ, K, desc_bytes=512, exchange=exchange, overlap=overlap, max_per_query=mpq)
                    assert sm.overlap == overlap and sm.keys[0].shape == (world * B * NQ, width) and sm.q_all[0].shape[-1] == 512
                    sm.begin(STEPS, lambda i: (torch.from_numpy(np.stack([frames[(i, b)] for b in range(B)]).view(np.uint8)), None))
                    for i in range(STEPS):
                        out = {}
                        sm.step(i, out)
                        res = out["result"]                     # B * NQ queries: frame b owns [b * NQ, (b + 1) * NQ)
                        rp, m, xyz = res[:3]
                        for b in range(B):
                            w = want[(i, b)]
                            lo, hi = int(rp[b * NQ]), int(rp[(b + 1) * NQ])
                            mine = m[lo:hi].copy()
                            mine["queryIdx"] -= b * NQ
                            ok = ok and np.array_equal(rp[b * NQ:(b + 1) * NQ + 1] - rp[b * NQ], w[0])
                            ok = ok and all(np.array_equal(mine[f], w[1][f]) for f in FIELDS)
                            ok = ok and np.array_equal(xyz[lo:hi], w[2])
                            if mpq is not None:
                                ok = ok and np.array_equal(res[3][b * NQ:(b + 1) * NQ], w[3])
                            n_matches += hi - lo
                    logs.append(list(ops.log))
        ret[rank] = (bool(ok), n_matches, logs)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_matcher_float_steps_equal_unsharded(world):
    """k-NN rows (k = 5 wide) and radius rows (64 + 1 wide), both exchanges, overlapped and serial, 3 steps each, float queries as
    512-byte rows, in one process group per world"""
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, 29570 + world, ret), nprocs=world, join=True)
    assert len(ret) == world
    for r in range(world):
        ok, n_matches, logs = ret[r]
        assert ok, "rank %d differs from the unsharded result" % r
        assert n_matches > 8 * STEPS * B * 3
        assert logs == ret[0][2], "rank %d issued its collectives in another order than rank 0" % r
    logs = ret[0][2]
    assert len(logs) == 8
    for n_log, width in ((0, K), (4, MPQ + 1)):
        a2a, ag = logs[n_log], logs[n_log + 2]                 # overlapped all-to-all, overlapped all-gather
        assert a2a.count("all_to_all%d" % (world * B * NQ * width)) == STEPS
        assert ag.count("all_gather%d" % (world * B * NQ * width)) == STEPS
        assert [w for w in a2a if w.startswith("all_gather")] == ["all_gather%d" % (B * NQ * 512)] * STEPS
