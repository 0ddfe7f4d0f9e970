"""todhip_db_select_objects without a GPU: the exported symbols, the header as C99, the null-context statuses, the Python wrappers,
the host side of the selection (tod_amd/csrc/db_select.h: sorting, de-duplication, prefix tables, the view row -> global row search)
in a stand-alone program built with -fsanitize=address,undefined, and ShardedMatcher.select_objects over gloo at world 2."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tod_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

NEW = ("todhip_db_select_objects", "todhip_db_selection", "todhip_pipeline_select_objects")


def test_symbols_are_exported_and_declared():
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "todhip.h")).read()
    for n in NEW:
        assert hasattr(L, n), n
        assert n + "(" in header and n in capi.EXPORTS


def test_header_with_the_new_calls_is_plain_c(tmp_path):
    """as tests/test_abi.py compiles it, with a caller of the three new functions"""
    src = tmp_path / "t.c"
    src.write_text('#include "todhip.h"\n'
                   "int f(todhip_ctx* c, todhip_pipeline* p) {\n"
                   "  uint32_t ids[2] = {3, 1}, n = 0; uint64_t rows = 0, shard_rows = 0;\n"
                   "  int rc = todhip_db_select_objects(c, ids, 2) + todhip_db_select_objects(c, NULL, 0);\n"
                   "  rc += todhip_db_selection(c, &n, &rows, &shard_rows) + todhip_pipeline_select_objects(p, ids, 2);\n"
                   "  return rc + (int)n + (int)rows + (int)shard_rows;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "t.o")], check=True)


def test_null_contexts_are_invalid_arguments():
    L = capi.lib()
    ids = np.array([0, 1], np.uint32)
    assert L.todhip_db_select_objects(None, ids.ctypes.data, 2) == capi.EINVAL
    assert L.todhip_db_select_objects(None, None, 0) == capi.EINVAL
    n, rows = capi.C.c_uint32(7), capi.C.c_uint64(7)
    assert L.todhip_db_selection(None, capi.C.byref(n), capi.C.byref(rows), None) == capi.EINVAL
    assert (n.value, rows.value) == (7, 7)
    assert L.todhip_pipeline_select_objects(None, ids.ctypes.data, 2) == capi.EINVAL


def test_python_wrappers_exist():
    for cls in (capi.Context, capi.Pipeline):
        assert callable(getattr(cls, "select_objects"))
    assert callable(capi.Context.selection)
    p, n, keep = capi._ids_in(None)
    assert p is None and n == 0
    p, n, keep = capi._ids_in([])
    assert p.value and n == 0                                           # an empty list is not "all objects"
    p, n, keep = capi._ids_in([7, 3, 3])
    assert n == 3 and keep.dtype == np.uint32 and keep.tolist() == [7, 3, 3]


# ---------------------------------------------------------------------------------------------------- the host tables
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("db_select") / "db_select_host_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "tod_amd", "csrc"),
                    os.path.join(ROOT, "tests", "db_select_host_test.cpp"), "-o", exe], check=True)
    return exe


def run_driver(exe, rows, ids, shard=None):
    off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    first, n = (0, int(off[-1])) if shard is None else shard
    out = subprocess.run([exe, str(first), str(n), "--"] + [str(r) for r in rows] + ["--"] + [str(i) for i in ids],
                         check=True, capture_output=True, text=True)
    assert out.stderr == ""                                             # no sanitizer report
    if out.stdout.strip() == "EINVAL":
        return None
    lines = out.stdout.split("\n")
    objs = [int(x) for x in lines[0].split()]
    sel_rows, view_rows = (int(x) for x in lines[1].split())
    segs = [tuple(int(v) for v in x.split(":")) for x in lines[2].split()]
    return dict(objs=objs, selected_rows=sel_rows, view_rows=view_rows, segs=segs, to_global=[int(x) for x in lines[3].split()],
                seg_of=[int(x) for x in lines[4].split()])


def expect(rows, ids, shard=None):
    off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    first, n = (0, int(off[-1])) if shard is None else shard
    objs = sorted(set(ids))
    segs, to_global, seg_of = [], [], []
    for o in objs:
        if rows[o] and first <= off[o] < first + n:
            segs.append((o, len(to_global), int(off[o])))
            to_global += list(range(int(off[o]), int(off[o + 1])))
            seg_of += [len(segs) - 1] * rows[o]
    return dict(objs=objs, selected_rows=int(sum(rows[o] for o in objs)), view_rows=len(to_global), segs=segs, to_global=to_global,
                seg_of=seg_of)


ROWS = [0, 1, 31, 32, 33, 257, 5, 700]


@pytest.mark.parametrize("ids", [[6], [1], [2, 4], [7, 3, 3], [0], [], list(range(8)), [7, 6, 5, 4, 3, 2, 1, 0, 0, 7], [5, 0, 6]])
def test_host_tables(driver, ids):
    assert run_driver(driver, ROWS, ids) == expect(ROWS, ids)


def test_host_tables_of_shards_and_many_short_objects(driver):
    rows = [700, 0, 1, 31, 32, 33, 257, 5]
    for shard in ((0, 700), (700, 97), (797, 262), (1059, 0)):
        for ids in ([0, 2, 6], [7, 5, 5, 1], [1], list(range(8))):
            assert run_driver(driver, rows, ids, shard) == expect(rows, ids, shard), (shard, ids)
    rng = np.random.Generator(np.random.PCG64(3))
    many = [int(x) for x in rng.integers(0, 9, 300)]                      # several segments inside one 128-row group
    ids = [int(x) for x in rng.permutation(300)[:200]] + [5, 5]
    assert run_driver(driver, many, ids) == expect(many, ids)


def test_host_tables_refuse_an_index_beyond_the_objects(driver):
    assert run_driver(driver, ROWS, [3, 8]) is None
    assert run_driver(driver, ROWS, [4294967295]) is None
    assert run_driver(driver, [], [0]) is None


# ---------------------------------------------------------------------------------------------------- ShardedMatcher over gloo
K, RADIUS, NQ, B = 3, 60, 64, 1


def _worker(rank, world, port, ret):
    import torch
    import torch.distributed as dist
    import oracle_lib as O
    from tod_amd import sharded, synth
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rows = [700, 40, 0, 900, 350, 5, 610]
        desc, pts, off = synth.make_db_ragged(rows, seed=123)
        lo, hi, row_lo, row_hi = sharded.shard_bounds(off, rank, world)
        state = dict(ids=None, calls=[])
        none = np.uint64(0xFFFFFFFFFFFFFFFF)

        def select(ids):                                                # the rank's context: keeps what it was told
            state["calls"].append(None if ids is None else list(ids))
            state["ids"] = None if ids is None else sorted(set(ids))

        def match_shard(q_all):                                         # CPU restatement: the shard's selected rows, global keys
            mine = range(lo, hi) if state["ids"] is None else [o for o in state["ids"] if lo <= o < hi]
            g = np.concatenate([np.arange(off[o], off[o + 1]) for o in mine] + [np.zeros(0, np.int64)]).astype(np.int64)
            if len(g) == 0:
                return torch.from_numpy(np.full((q_all.shape[0], K), none, np.uint64).view(np.int64))
            keys = O.knn_keys(desc[g], q_all.numpy(), K)
            real = keys != none
            keys[real] = (keys[real] >> np.uint64(32) << np.uint64(32)) | g[(keys[real] & np.uint64(0xFFFFFFFF)).astype(np.int64)].astype(np.uint64)
            return torch.from_numpy(keys.view(np.int64))

        def merge(keys_mine):
            k = np.sort(keys_mine.numpy().view(np.uint64).transpose(1, 0, 2).reshape(NQ * B, -1), axis=1)[:, :K]
            return k

        ops = sharded.HostOps(dist, match_shard, merge, two_streams=True, select_objects=select)
        sm = sharded.ShardedMatcher(ops, world, rank, B, NQ, K)
        frames = [synth.make_frame(desc, pts, off, NQ, frame=10 * rank + i, visible_object=(3, 0, 4)[i])["q_desc"] for i in range(3)]
        ok = True
        for i, ids in enumerate(([4, 0, 4], [5], None)):
            sm.select_objects(ids)
            sm.begin(1, lambda _i: (torch.from_numpy(frames[i][None]), None))
            out = {}
            sm.step(0, out)
            sel = range(len(rows)) if ids is None else sorted(set(ids))
            g = np.concatenate([np.arange(off[o], off[o + 1]) for o in sel]).astype(np.int64)
            want = O.knn_keys(desc[g], frames[i], K)
            want = (want >> np.uint64(32) << np.uint64(32)) | g[(want & np.uint64(0xFFFFFFFF)).astype(np.int64)].astype(np.uint64)
            ok = ok and np.array_equal(out["result"], want)
        ret[rank] = (bool(ok), state["calls"], list(ops.log))
    finally:
        dist.destroy_process_group()


def test_sharded_matcher_forwards_the_selection_to_every_rank():
    import torch.multiprocessing as mp
    world = 2
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(world, 29577, ret), nprocs=world, join=True)
    assert len(ret) == world
    for r in range(world):
        ok, calls, log = ret[r]
        assert calls == [[4, 0, 4], [5], None], "rank %d was told %r" % (r, calls)
        assert ok, "rank %d: the merged keys differ from the search over the selected objects" % r
        assert log == ret[0][2] and log.count("select_objects") == 3
