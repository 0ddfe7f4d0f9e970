"""Every wrapper of tod_amd/capi.py marshals what include/todhip.h declares, without a GPU and without the library's code: a stand-in
takes the place of the loaded library. Each todhip_* attribute of it checks the argument count against the real prototype, converts
each argument with the prototype's from_param as ctypes would at the call, records its name, writes nothing and returns 0. Every
public method of Context, Model, PatternLearner and Pipeline and every module-level function is then called once on the smallest
inputs; the recorded names must be the header's minus the few exports the binding never calls.

GpuOps (tod_amd/sharded.py) is checked the same way one level up: around a context that records method calls, its table must pick,
for the four search families and both merge streams, the calls and the argument order written out below."""
import ctypes as C
import inspect
import types

import numpy as np
import pytest

from tod_amd import capi, sharded

# exports that capi.py never calls
NEVER_CALLED = {"todhip_version", "todhip_last_hip_error", "todhip_stream_destroy", "todhip_orb"}


class StandIn:
    def __init__(self, real):
        self.called = []
        for name in capi.EXPORTS:
            setattr(self, name, self._function(name, list(getattr(real, name).argtypes)))

    def _function(self, name, argtypes):
        def call(*args):
            assert len(args) == len(argtypes), "%s takes %d arguments, got %d" % (name, len(argtypes), len(args))
            for i, (t, a) in enumerate(zip(argtypes, args)):
                try:
                    t.from_param(a)
                except (TypeError, C.ArgumentError) as e:
                    raise AssertionError("%s, argument %d: %r is no %s (%s)" % (name, i + 1, a, t.__name__, e))
            self.called.append(name)
            return 0
        return call


@pytest.fixture
def standin(monkeypatch):
    s = StandIn(capi.lib())
    monkeypatch.setattr(capi, "_lib", s)
    return s


def _public(cls):
    return {n for n, f in vars(cls).items() if not n.startswith("_") and inspect.isfunction(f)}


D = 0x7F0000001000                                            # a device pointer as tensor.data_ptr() gives it: never read here
K = np.array([[525.0, 0, 1.0], [0, 525.0, 1.0], [0, 0, 1]])


def test_every_wrapper_marshals_what_the_header_declares(standin):
    desc, pts, off = np.zeros((2, 32), np.uint8), np.zeros((2, 3), np.float32), [0, 2]
    q, qf = np.zeros((2, 32), np.uint8), np.zeros((2, 128), np.float32)
    img, depth = np.zeros((2, 2), np.uint8), np.ones((2, 2), np.float32)
    kp, rp, m, xyz = np.zeros((2, 2), np.float32), np.zeros(3, np.uint32), np.zeros(1, capi.DMATCH_DTYPE), np.zeros((1, 3), np.float32)
    spans, pattern = np.ones(1, np.float32), np.zeros((256, 4), np.int8)
    done = {}                                                 # class or module name -> the public names called below

    def each(owner, obj, calls):
        for name, args in calls:
            args, kw = (args[:-1], args[-1]) if args and isinstance(args[-1], dict) else (args, {})
            getattr(obj, name)(*args, **kw)
            done.setdefault(owner, set()).add(name)

    rng, rngs = capi.rng_new(1), (capi.Rng * 2)()
    ctx = capi.Context(0)
    model = capi.Model(ctx, capacity_rows=4)
    each("Context", ctx, [
        ("synchronize", ()), ("counters", ()), ("set_matcher_engine", ("mfma",)), ("set_matcher_block_split", (-1,)),
        ("set_ratio_test", (0.8,)), ("set_lsh", (2,)), ("set_db_bit_order", (1,)), ("db_bit_order", ()), ("set_kernel_timing", (True,)),
        ("db_load", (desc, pts, off)), ("db_load_models", ([model],)), ("db_info", ()), ("desc_bytes", ()), ("select_objects", ([0],)),
        ("selection", ()), ("match", (q, 2, 35)), ("match_radius", (q, 35, 4)), ("match_radius_device", (D, 2, 35, 4, D, D, D)),
        ("match_radius_shard_device", (D, 2, 35, 4, D)), ("merge_radius_shards_device", (D, 1, 2, 4, D, D, D, D)),
        ("merge_radius_shards_device", (D, 1, 2, 4, D, D, D, D, dict(stream=D))), ("merge_radius_shards_device_on", (D, D, 1, 2, 4, D, D, D)),
        ("match_l2", (qf, 2, 0.5)), ("match_l2_device", (D, 2, 2, 0.5, D, D, D)), ("match_l2_radius", (qf, 0.5, 4)),
        ("match_l2_radius_device", (D, 2, np.float32(0.5), 4, D, D, D, D)), ("match_l2_shard_device", (D, 2, 2, D)),
        ("merge_l2_shards_device", (D, 1, 2, 2, 0.5, D, D, D)), ("merge_l2_shards_device", (D, 1, 2, 2, 0.5, D, D, D, dict(stream=D))),
        ("match_l2_radius_shard_device", (D, 2, 0.5, 4, D)), ("merge_l2_radius_shards_device", (D, 1, 2, 4, D, D, D)),
        ("merge_l2_radius_shards_device", (D, 1, 2, 4, D, D, D, D, dict(stream=D))), ("match_device", (D, np.int64(2), 2, 35, D, D, D)),
        ("cross_check_device", (D, 2, 2, 2, D, D, D, [2])), ("set_cross_check", (2,)), ("set_l2_ratio_test", (0.8,)),
        ("cross_check_l2_device", (D, 2, 2, 2, D, D, D)), ("set_l2_cross_check", (2,)), ("match_shard_device", (D, 2, 2, 35, D)),
        ("merge_shards_device", (D, 1, 2, 2, 35, D, D, D)), ("merge_shards_device", (D, 1, 2, 2, 35, D, D, D, dict(stream=D))),
        ("merge_shards_device_on", (D, D, 1, 2, 2, 35, D, D, D)),
        ("verify", (kp, np.zeros((2, 2, 3), np.float32), rp, m, xyz, spans, 8, 10, 0.01, rng, 2)),
        ("verify_2d", (kp, K, rp, m, xyz, spans, 8, 10, 3.0, rng, 2)), ("verify_2d_device", (D, 2, K, D, D, D, 2, spans, 8, 10, 3.0, rng, 2)),
        ("verify_2d_batch_device", (2, D, 2, K, D, D, D, 2, spans, 8, 10, 3.0, rngs, 2)),
        ("verify_device", (D, 2, D, 2, 2, D, D, D, 2, spans, 8, 10, 0.01, rng, 2)),
        ("verify_device_depth", (D, 2, D, True, 2, 2, K, D, D, D, 2, spans, 8, 10, 0.01, rng, 2)),
        ("verify_batch_device", (2, D, 2, D, 2, 2, D, D, D, 2, spans, 8, 10, 0.01, rngs, 2)),
        ("verify_batch_device", (2, D, 2, None, 2, 2, D, D, D, 2, spans, 8, 10, 0.01, rngs, 2, (D, False, K))),
        ("verify_device_depth_rescaled", (D, 2, D, False, 1, 1, True, 2, 2, K, D, D, D, 2, spans, 8, 10, 0.01, rng, 2)),
        ("verify_batch_device_depth_rescaled", (2, D, 2, D, False, 1, 1, False, 2, 2, K, D, D, D, 2, spans, 8, 10, 0.01, rngs, 2)),
        ("test_depth_lookup", (D, False, 1, 1, False, 2, 2, kp)), ("verify_trace", (2,)),
        ("test_adjacency", (pts, pts, kp, 1.0, 0.01)), ("test_consensus", (pts, pts, kp, 1.0, 0.01, [[0, 1, 1]])),
        ("test_consensus", (pts, pts, kp, 1.0, 0.01, [[0, 1, 1]], 1, 4)),
        ("test_draw_table", (np.zeros((2, 1), np.uint64), np.zeros(1, np.uint64), 2, np.zeros(4, np.uint32), 2)),
        ("test_kabsch", (np.zeros((1, 3, 3)), np.zeros((1, 6)))), ("test_clique", (2, [[0, 1]])), ("test_clique", (2, [[0, 1]], 2, True)),
        ("orb", (img, 4, 1, 1.2)), ("orb", (img, 4, 1, 1.2, pattern, img)), ("orb", (img, 4, 1, 1.2, None, img, 2, 2, 2)),
        ("orb_device", (D, 2, 2, 2, 4, 1, 1.2, D, D, D, 4, pattern)), ("orb_batch_device", (D, 2, 4, 2, 2, 2, 4, 1, 1.2, D, D, D, 4)),
        ("orb_batch_device_masked", (D, 0, 2, 4, 2, 2, 2, 4, 1, 1.2, D, D, D, 4, pattern)),
        ("rescale_depth", (np.ones((1, 1), np.uint16), 2, 2)), ("rescale_depth_device", (D, True, 1, 1, D, 2, 2, True)),
    ])
    assert ctx.stream == 0 or ctx.stream is None
    done["Context"].add("stream")
    each("Model", model, [
        ("add_observation", (img, img, depth, K, np.eye(3), np.zeros(3), 4, 1)),
        ("add_observation", (img, img, np.ones((1, 1), np.float32), K, np.eye(3), np.zeros(3), 4, 1, 1.2, pattern)),
        ("add_observations_device", (D, D, D, 2, 2, 2, K, np.zeros((2, 3, 3)), np.zeros((2, 3)))),
        ("add_observations_device", (D, 0, D, 1, 2, 2, K, np.eye(3), np.zeros(3), dict(depth_is_u16=True, depth_size=(1, 1), pattern=pattern))),
        ("add_rows", (desc, pts)), ("add_rows", (desc[:0], pts[:0])), ("compact", (0.01,)), ("compact", (0.01, 10, True)), ("device", ()),
        ("finish", ()),
    ])
    learner = capi.PatternLearner(ctx, 8)
    capi.PatternLearner(ctx, 8, np.zeros((4, 4), np.int8))
    each("PatternLearner", learner, [("add_view", (img,)), ("add_view", (img, img, 4, 1)), ("add_view_device", (D, None, 2, 2, 2)),
                                     ("finish", ()), ("responses", (0, 1))])
    pipe = capi.Pipeline(0, K=K, n_features=4)
    each("Pipeline", pipe, [
        ("matcher", ()), ("db_load", (desc, pts, off)), ("db_load_models", ([model],)), ("set_pattern", (pattern,)), ("set_pattern", (None,)),
        ("set_cross_check", (True,)), ("select_objects", (None,)), ("submit", (img[None], depth[None])), ("set_depth_size", (1, 1, True)),
        ("submit_masked", (img[None], img[None], depth[None])), ("submit_masked", (img[None], None, depth[None], 1)),
        ("submit_masked_device", (D, 0, D, 1)), ("submit_device", (D, D, 1)), ("wait", (0,)), ("wait", (0, 5, 1, 1, False)), ("stats", ()),
    ])
    each("capi", capi, [("pipeline_params", ()), ("bgr_to_gray_device", (ctx, D, 3, 2, 2, 6, D, 2)), ("set_cu_partition", (0,)),
                        ("stream_create", (0, True)), ("rng_new", (7,)), ("radius_capacity", (4,))])
    # close() frees only a handle the library has written: the stand-in writes none
    for owner, obj in (("Model", model), ("PatternLearner", learner), ("Pipeline", pipe), ("Context", ctx)):
        obj._h = C.c_void_p(1)
        obj.close()
        assert not obj._h
        done[owner].add("close")

    # nothing public was left out above ...
    for cls in (capi.Context, capi.Model, capi.PatternLearner, capi.Pipeline):
        assert done[cls.__name__] == _public(cls) | ({"stream"} if cls is capi.Context else set()), cls.__name__
    functions = {n for n, f in vars(capi).items() if isinstance(f, types.FunctionType) and not n.startswith("_") and f.__module__ == capi.__name__}
    assert done["capi"] == functions - {"build", "lib"}
    # ... and together the wrappers reach every declared function but the four
    assert NEVER_CALLED == {"todhip_version", "todhip_last_hip_error", "todhip_stream_destroy", "todhip_orb"}
    assert set(standin.called) == set(capi.EXPORTS) - NEVER_CALLED


def test_stream_argument_selects_the_on_form(standin):
    """Context's four merges: stream=None is the plain call, a stream the _on call with the stream behind the context"""
    seen = []
    for name in capi.EXPORTS:
        setattr(standin, name, lambda *a, _n=name: seen.append((_n,) + a[1:]) or 0)
    ctx = capi._Borrowed(1)
    ctx.merge_shards_device(D, 3, 2, 5, 35, 11, 12, 13)
    ctx.merge_shards_device(D, 3, 2, 5, 35, 11, 12, 13, stream=77)
    ctx.merge_shards_device_on(77, D, 3, 2, 5, 35, 11, 12, 13)
    ctx.merge_radius_shards_device(D, 3, 2, 4, 11, 12, 13, 14, stream=77)
    ctx.merge_radius_shards_device_on(77, D, 3, 2, 4, 11, 12, 13)
    ctx.merge_l2_shards_device(D, 3, 2, 5, 0.5, 11, 12, 13, stream=77)
    ctx.merge_l2_radius_shards_device(D, 3, 2, 4, 11, 12, 13, stream=77)
    assert seen == [("todhip_merge_shards_device", D, 3, 2, 5, 35, 11, 12, 13),
                    ("todhip_merge_shards_device_on", 77, D, 3, 2, 5, 35, 11, 12, 13),
                    ("todhip_merge_shards_device_on", 77, D, 3, 2, 5, 35, 11, 12, 13),
                    ("todhip_merge_radius_shards_device_on", 77, D, 3, 2, 4, 11, 12, 13, 14),
                    ("todhip_merge_radius_shards_device_on", 77, D, 3, 2, 4, 11, 12, 13, None),
                    ("todhip_merge_l2_shards_device_on", 77, D, 3, 2, 5, 0.5, 11, 12, 13),
                    ("todhip_merge_l2_radius_shards_device_on", 77, D, 3, 2, 4, 11, 12, 13, None)]


def test_a_status_other_than_ok_raises_with_the_functions_own_name(standin):
    """_call names the function it called: the two messages that named another one (the depth batch form, the clique gate)"""
    for name in capi.EXPORTS:
        setattr(standin, name, lambda *a: capi.EINVAL)
    ctx = capi._Borrowed(1)
    with pytest.raises(capi.TodError, match="todhip_verify_batch_device_depth failed with todhip_status -1") as e:
        ctx.verify_batch_device(1, D, 2, None, 2, 2, D, D, D, 2, np.ones(1, np.float32), 8, 10, 0.01, (capi.Rng * 1)(), 2, (D, False, K))
    assert e.value.status == capi.EINVAL
    with pytest.raises(capi.TodError, match="todhip_test_clique_gate failed"):
        ctx.test_clique(2, [[0, 1]], gate=True)
    with pytest.raises(capi.TodError, match="todhip_test_clique failed"):
        ctx.test_clique(2, [[0, 1]])
    pipe = object.__new__(capi.Pipeline)                                    # (no create: it raises on this stand-in)
    pipe._h, pipe._n = C.c_void_p(1), {}
    try:                                                                     # a status that is an answer comes back as it is
        assert pipe.set_cross_check(True) == capi.EINVAL and pipe.submit_device(D, D, 1) == (capi.EINVAL, 0) and pipe._n == {}
    finally:
        pipe._h = C.c_void_p()


class _Tensor:
    def __init__(self, ptr, shape=(4, 512), element_size=1):
        self.ptr, self.shape, self._es = ptr, shape, element_size

    def data_ptr(self):
        return self.ptr

    def element_size(self):
        return self._es


class _RecordingContext:
    def __init__(self):
        self.calls = []

    def desc_bytes(self):
        return 512

    def __getattr__(self, name):
        return lambda *a, **kw: self.calls.append((name, a, kw))


@pytest.mark.parametrize("metric, mpq, shard, merge", [
    ("hamming", None, ("match_shard_device", (100, 8, 5, 35, 200)), ("merge_shards_device", (300, 3, 8, 5, 35, 1, 2, 3))),
    ("hamming", 4, ("match_radius_shard_device", (100, 8, 35, 4, 200)), ("merge_radius_shards_device", (300, 3, 8, 4, 1, 2, 3, 4))),
    ("l2", None, ("match_l2_shard_device", (100, 8, 5, 200)), ("merge_l2_shards_device", (300, 3, 8, 5, 35, 1, 2, 3))),
    ("l2", 4, ("match_l2_radius_shard_device", (100, 8, 35, 4, 200)), ("merge_l2_radius_shards_device", (300, 3, 8, 4, 1, 2, 3, 4))),
])
def test_gpuops_table_picks_the_family(monkeypatch, metric, mpq, shard, merge):
    """What GpuOps.match_shard and GpuOps.merge call on the context: the shard call on (q, n, the family's settings, keys), the merge
    on (keys, n_shards, n, the family's settings, counts, matches, xyz[, in_radius]) -- on the context's stream when it is the
    compute stream, otherwise on that stream's handle (stream=: what reaches the library then is the _on function with the handle
    behind the context, test_stream_argument_selects_the_on_form)"""
    import sys
    dist = types.SimpleNamespace(get_world_size=lambda: 3)
    monkeypatch.setitem(sys.modules, "torch", types.SimpleNamespace(distributed=dist))
    monkeypatch.setitem(sys.modules, "torch.distributed", dist)
    ctx = _RecordingContext()
    compute, comm = types.SimpleNamespace(cuda_stream=66), types.SimpleNamespace(cuda_stream=77)
    ops = sharded.GpuOps(ctx, compute, comm, "nccl", 5, 35, max_per_query=mpq, metric=metric)
    out = dict(counts=_Tensor(1), matches=_Tensor(2), xyz=_Tensor(3), in_radius=_Tensor(4))
    ops.match_shard(_Tensor(100), 8, _Tensor(200))
    ops.merge(_Tensor(300), 3, 8, out, compute)
    ops.merge(_Tensor(300), 3, 8, out, comm)
    assert ctx.calls == [shard + ({},), merge + (dict(stream=None),), merge + (dict(stream=77),)]
    if metric == "l2":
        with pytest.raises(ValueError):
            ops.match_shard(_Tensor(100, (4, 256)), 8, _Tensor(200))
