"""ctypes binding of libtodhip.so (include/todhip.h).

The shared library is the product; this module only loads it and marshals numpy / torch
buffers to plain pointers. There is no CPU fallback: if the library or the GPU is missing,
loading or context creation raises.

Every prototype comes from include/todhip.h (and the part of it kept in include/todhip_ratio_other.h): the header is parsed when this module is imported (the import fails without it, or on a
declaration it cannot read) and lib() sets argtypes and restype of each function it declares, so a signature is written once, there. An argument of the wrong kind -- a ctypes wrapper of another type than the header's, a float for an
integer, a numpy scalar for a pointer -- therefore raises ctypes.ArgumentError at the call; it is never truncated or reinterpreted.
Plain Python and numpy integers, bool, None (NULL), byref(...), ctypes arrays and instances of the header's own type pass.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "todhip.h")
# the part of the C ABI that todhip.h includes at its end: the ratio test against another object
RATIO_OTHER_HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "todhip_ratio_other.h")
# TODHIP_LIB_PATH: another build of the same library (the diagnostics builds of tools/*_ablate.sh, an A/B against HEAD) -- loaded
# instead of, never copied over, the product file
LIB_PATH = os.environ.get("TODHIP_LIB_PATH") or os.path.join(_PKG, "libtodhip.so")

OK, EINVAL, ENODB, EHIP, ECAPACITY, ERANGE, ENOMEM, ESCRATCH, EBUSY, ETIMEOUT = 0, -1, -2, -3, -4, -5, -6, -7, -8, -9
FRAME_GRAY8, FRAME_BGR8, FRAME_BGRA8 = 0, 1, 2
PATTERN_ORDER_RANK, PATTERN_ORDER_MATCHER = 0, 1

DMATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])


class TodObject(C.Structure):
    _fields_ = [("desc", C.c_void_p), ("pts_xyz", C.c_void_p), ("n", C.c_uint32)]


class Rng(C.Structure):
    _fields_ = [("s", C.c_uint32 * 31), ("f", C.c_uint32), ("b", C.c_uint32), ("draws", C.c_uint64)]


class VerifyParams(C.Structure):
    _fields_ = [("min_inliers", C.c_uint32), ("n_ransac_iterations", C.c_uint32), ("sensor_error", C.c_float)]


class Pose(C.Structure):
    _fields_ = [("object", C.c_uint32), ("R", C.c_float * 9), ("t", C.c_float * 3),
                ("inlier_begin", C.c_uint32), ("inlier_end", C.c_uint32)]


class RoundTrace(C.Structure):
    _fields_ = [("object", C.c_uint32), ("iterations", C.c_uint32), ("best_iteration", C.c_uint32),
                ("best_count", C.c_int32), ("draws_before", C.c_uint64), ("draws_after", C.c_uint64),
                ("n_inlier_kp", C.c_uint32), ("accepted", C.c_uint32)]


class Counters(C.Structure):
    _fields_ = [("db_rows", C.c_uint64), ("db_objects", C.c_uint64), ("last_nq", C.c_uint32), ("last_k", C.c_uint32),
                ("last_matches", C.c_uint32), ("last_objects_verified", C.c_uint32), ("last_rounds", C.c_uint32),
                ("last_hypotheses", C.c_uint32), ("last_gate_calls", C.c_uint32), ("last_poses", C.c_uint32),
                ("last_match_kernel_ms", C.c_double), ("sum_match_kernel_ms", C.c_double),
                ("n_match_kernel_launches", C.c_uint64), ("last_sprint_launches", C.c_uint32), ("last_sprint_rounds", C.c_uint32),
                ("last_verify_ticks", C.c_uint32), ("last_block_split", C.c_uint32), ("k4x_half_blocks", C.c_uint64),
                ("k4x_half_blocks_completed", C.c_uint64), ("last_fp4_rows", C.c_uint32), ("fp4_rows_builds", C.c_uint32)]


class PipelineParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("frames_per_step", C.c_uint32), ("H", C.c_uint32), ("W", C.c_uint32),
                ("frame_format", C.c_int), ("depth_is_u16", C.c_int), ("K9", C.c_float * 9), ("n_features", C.c_uint32),
                ("n_levels", C.c_uint32), ("scale_factor", C.c_float), ("k", C.c_uint32), ("radius", C.c_uint32),
                ("verify", VerifyParams), ("rng_seed", C.c_uint32), ("orb_workers", C.c_uint32), ("verify_workers", C.c_uint32),
                ("ring_depth", C.c_uint32), ("max_poses_per_frame", C.c_uint32)]


class PipelineStats(C.Structure):
    _fields_ = [("steps", C.c_uint64), ("frames", C.c_uint64), ("keypoints", C.c_uint64), ("poses", C.c_uint64),
                ("orb_s", C.c_double), ("match_issue_s", C.c_double), ("verify_s", C.c_double),
                ("sum_match_kernel_ms", C.c_double), ("n_match_kernel_launches", C.c_uint64)]


class PatternStats(C.Structure):
    _fields_ = [("n_keypoints", C.c_uint32), ("n_candidates", C.c_uint32), ("accepted_in_round", C.c_uint32 * 6)]


_SCALARS = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int": C.c_int, "float": C.c_float}
_DECLARATION = re.compile(r"\b(\w+\s*\**)\s*\b(todhip_\w+)\s*\(([^()]*)\)\s*;")


def _prototypes(path):
    """{name: (restype, argtypes)} of every function the header at `path` declares, in its order. A pointer or an array is c_void_p,
    the scalars are _SCALARS; a parameter of any other type raises (it would have to be guessed)."""
    with open(path) as f:
        code = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    protos = {}
    for ret, name, params in _DECLARATION.findall(code):
        argtypes = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            words = [w for w in p.split() if w != "const"]
            if "*" in p or "[" in p:
                argtypes.append(C.c_void_p)
            elif words and words[0] in _SCALARS:
                argtypes.append(_SCALARS[words[0]])
            else:
                raise RuntimeError("%s: %s declares a parameter '%s' of a type the binding does not know" % (path, name, " ".join(p.split())))
        protos[name] = (C.c_void_p if "*" in ret else None if ret.strip() == "void" else C.c_int, argtypes)
    unread = set(re.findall(r"\b(todhip_\w+)\s*\(", code)) - set(protos)      # e.g. a parameter list with parentheses of its own
    if unread:
        raise RuntimeError("%s: the binding cannot read the declaration of %s" % (path, ", ".join(sorted(unread))))
    return protos


# the header is read once, when this module is imported (the tree carries it beside the package; without it the import fails)
_PROTOTYPES = _prototypes(HEADER_PATH)
# every symbol include/todhip.h declares, in its order (tests/test_abi.py checks them and their prototypes against the header text)
EXPORTS = list(_PROTOTYPES)
# ... and those of include/todhip_ratio_other.h, read the same way (tests/test_ratio_other_binding_cpu.py checks them as test_abi.py
# and test_capi_marshal_cpu.py check the list above)
_RATIO_OTHER_PROTOTYPES = _prototypes(RATIO_OTHER_HEADER_PATH)
RATIO_OTHER_EXPORTS = list(_RATIO_OTHER_PROTOTYPES)

MAX_TRAIN_BATCH_VIEWS = 64

# todhip_model_add_observations_device's arguments in the header's order: kept as a name for callers of earlier versions, read from the header
ADD_OBSERVATIONS_DEVICE_ARGTYPES = _PROTOTYPES["todhip_model_add_observations_device"][1]

MAX_PER_QUERY_LIMIT = 1024


def radius_capacity(max_per_query):
    """C of todhip_match_radius: the keys a query's candidate buffer holds (2 * max_per_query rounded up to a power of two, at least
    64). A query with more rows than that inside the radius is answered by the ordered second pass."""
    c = 64
    while c < 2 * max_per_query:
        c *= 2
    return c


# Model.compact's default descriptor bound: the setting of DESIGN 6f's end-to-end check, well inside the matcher's radius (35 or 55)
DEFAULT_COMPACT_HAMMING = 24

_lib = None


def build():
    """Compile libtodhip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    subprocess.run(["make", "-C", os.path.join(_PKG, "csrc"), "-s", "-j4"], check=True)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libtodhip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        # PyTorch ships its own HIP runtime; when both live in one process (tests, bench) torch must bring
        # the runtime up first, otherwise its later initialisation finds no device.
        try:
            import torch
            if torch.cuda.is_available():
                torch.cuda.init()
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in list(_PROTOTYPES.items()) + list(_RATIO_OTHER_PROTOTYPES.items()):
            f = getattr(L, name, None)            # TODHIP_LIB_PATH may name a build of an older commit: what it lacks stays an AttributeError
            if f is not None:
                f.restype, f.argtypes = restype, argtypes
        _lib = L
    return _lib


class TodError(RuntimeError):
    def __init__(self, status, what):
        super().__init__("%s failed with todhip_status %d" % (what, status))
        self.status = status


def _call(name, *args):
    """The library's function `name` on args; a status other than OK raises TodError(status, name)."""
    rc = getattr(lib(), name)(*args)
    if rc != OK:
        raise TodError(rc, name)


def _np_ptr(a):
    """The pointer of a numpy array; None (an optional array that is absent) stays None: NULL"""
    return None if a is None else C.c_void_p(a.ctypes.data)


def _opt(a, dtype):
    """An optional array (pattern, mask) as a contiguous one of dtype, or None"""
    return None if a is None else np.ascontiguousarray(a, dtype)


def _objects(desc, pts, obj_off):
    """(TodObject[n_obj], n_obj, bytes per row) of DB rows in host memory: desc [N, width], pts f32[N, 3], both contiguous and held
    by the caller during the call; rows of object o are obj_off[o]:obj_off[o+1]"""
    obj_off = np.asarray(obj_off, np.int64)
    n_obj = len(obj_off) - 1
    B = (desc.shape[1] if desc.ndim == 2 else 32) * desc.itemsize
    objs = (TodObject * max(n_obj, 1))()
    for o in range(n_obj):
        lo, hi = int(obj_off[o]), int(obj_off[o + 1])
        objs[o].desc, objs[o].pts_xyz, objs[o].n = desc.ctypes.data + lo * B, pts.ctypes.data + lo * 12, hi - lo
    return objs, n_obj, B


def _model_objects(models):
    """(TodObject[len(models)], obj_off u32[len(models) + 1]) of trained models (capi.Model) in device memory"""
    objs = (TodObject * len(models))()
    off = [0]
    for i, m in enumerate(models):
        objs[i].desc, objs[i].pts_xyz, objs[i].n = m.device()
        off.append(off[-1] + objs[i].n)
    return objs, np.asarray(off, np.uint32)


def _frame_limits(frame_nq, nq, frame_queries, what):
    """frame_nq of a cross-check as u32[ceil(nq / frame_queries)] (None stays None); another length is TodError(EINVAL)"""
    fn = _opt(frame_nq, np.uint32)
    if fn is not None and len(fn) != (nq + frame_queries - 1) // max(frame_queries, 1):
        raise TodError(EINVAL, "%s (frame_nq of %d entries for %d queries in frames of %d)" % (what, len(fn), nq, frame_queries))
    return fn


def _ids_in(ids):
    """(pointer, count, array to keep alive) of an object-index list for the select_objects calls; None -> (NULL, 0): all objects.
    An empty list is a real, non-null pointer: it selects nothing."""
    if ids is None:
        return None, 0, None
    a = np.ascontiguousarray(ids, np.uint32).reshape(-1)
    keep = a if a.size else np.zeros(1, np.uint32)
    return _np_ptr(keep), int(a.size), keep


def _strided_rows(a, stride, W=None):
    """(array, H, W) of a 2-D u8 array whose row pitch is `stride` bytes and whose first W columns (default: all) are the image"""
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 2 or (a.shape[0] > 1 and a.strides[0] != stride) or a.strides[1] != 1:
        raise ValueError("need a 2-D uint8 array of row pitch %d" % stride)
    W = a.shape[1] if W is None else W
    if not 0 < W <= min(a.shape[1], stride):
        raise ValueError("W outside the rows")
    return a, a.shape[0], W


def _k9(K):
    return np.ascontiguousarray(K, np.float32).reshape(9)


def _pose_out(max_poses, n_kp, n_frames=None, cache=None):
    """Output arrays of one verify* call: room for max_poses poses (per frame, with a pose_ptr, when n_frames is given) and their
    inlier keypoints. cache: the Context that keeps the inlier array between calls (a megabyte per batch otherwise; results are
    copied out of it). Returns (poses, n_poses, inl, n_inl, pose_ptr)."""
    cap_p = max_poses if n_frames is None else max_poses * n_frames
    cap = max(n_kp, 1) * cap_p
    if cache is None:
        inl = np.zeros(cap, np.uint32)
    else:
        if getattr(cache, "_inl_cap", 0) < cap:
            cache._inl = np.zeros(cap, np.uint32)
            cache._inl_cap = cap
        inl = cache._inl
    return (Pose * cap_p)(), C.c_uint32(cap_p), inl, C.c_uint32(cap), None if n_frames is None else (C.c_uint32 * (n_frames + 1))()


def _pose_list(poses, lo, hi, inl):
    return [dict(object=int(poses[i].object), R=np.array(poses[i].R[:], np.float32).reshape(3, 3), t=np.array(poses[i].t[:], np.float32),
                 inliers=inl[poses[i].inlier_begin:poses[i].inlier_end].copy()) for i in range(lo, hi)]


class _RatioOtherCalls:
    """The calls of include/todhip_ratio_other.h on a context: a base of Context, so that a borrowed context (the pipeline's matcher)
    has them too."""

    def other_object_min_device(self, d_q, nq, d_excl_obj, d_min, d_limit=None, limit_cap=0xFFFFFFFF):
        """d_min[q] = min(the least Hamming distance from query q to a searched row outside object d_excl_obj[q], d_limit[q],
        limit_cap), u32, 0xFFFFFFFF where there is no such row and no limit (todhip_other_object_min_device). Device pointers; every
        word of d_min is written. Runs on any context, also on one shard: the element-wise minimum over the ranks is the whole DB's."""
        _call("todhip_other_object_min_device", self._h, d_q, nq, d_excl_obj, d_limit, limit_cap, d_min)

    def ratio_other_apply_device(self, ratio, nq, stride, d_other_min, d_counts, d_matches):
        """counts[q] = 0 where a query's nearest kept match (slot 0) fails (float)d1 < ratio * (float)other_min[q]; 0xFFFFFFFF in
        other_min always passes (todhip_ratio_other_apply_device)."""
        _call("todhip_ratio_other_apply_device", self._h, ratio, nq, stride, d_other_min, d_counts, d_matches)

    def ratio_other_device(self, d_q, nq, ratio, stride, d_counts, d_matches):
        """Lowe's ratio test against the nearest searched row of ANOTHER object than the nearest match's, in place on a fixed-stride
        device output of an unsharded context (todhip_ratio_other_device). Asynchronous on the context's stream."""
        _call("todhip_ratio_other_device", self._h, d_q, nq, ratio, stride, d_counts, d_matches)

    def set_ratio_test_other(self, ratio):
        """match() and match_device() run ratio_other_device behind their finalize step, in front of the cross-check (0 = off, the
        default). The sharded, radius and float forms ignore it."""
        _call("todhip_set_ratio_test_other", self._h, ratio)


class Context(_RatioOtherCalls):
    """One HIP device + stream (todhip_ctx)."""

    def __init__(self, device=0, stream=None):
        self._h = C.c_void_p()
        _call("todhip_create", device, stream, C.byref(self._h))

    def close(self):
        if self._h:
            lib().todhip_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self):
        return lib().todhip_stream(self._h)

    def synchronize(self):
        _call("todhip_synchronize", self._h)

    def counters(self):
        c = Counters()
        _call("todhip_get_counters", self._h, C.byref(c))
        return c

    def set_matcher_engine(self, engine):
        """0 auto, 1 vector ALU (K4), 2 matrix cores (K4x): identical results"""
        _call("todhip_set_matcher_engine", self._h, {"auto": 0, "valu": 1, "mfma": 2}.get(engine, engine))

    def set_matcher_block_split(self, split):
        """-1 adaptive (default), 0 whole blocks, 2 / 3: the matrix-core engine's blocks stop after that many of their 4 matrix
        instructions when no partial sum can still reach a threshold: identical results"""
        _call("todhip_set_matcher_block_split", self._h, split)

    def set_ratio_test(self, ratio):
        """Lowe's ratio test on the two nearest neighbours (0 = off, the reference's effective setting)"""
        _call("todhip_set_ratio_test", self._h, ratio)

    def set_lsh(self, n_tables, key_size=16, multi_probe_level=1):
        """LSH-approximate mode of the Hamming matcher (0 tables = the exact search, the default)."""
        _call("todhip_set_lsh", self._h, n_tables, key_size, multi_probe_level)

    def set_db_bit_order(self, mode):
        """0 off (default), 1 informative bits first: the db_load calls that follow store the rows' bit positions in that order and the
        match calls permute their queries alike -- identical results (todhip_set_db_bit_order)"""
        _call("todhip_set_db_bit_order", self._h, mode)

    def db_bit_order(self):
        """u8[256]: stored position p of the resident DB holds original bit src_of[p] (the identity when off / nothing loaded)"""
        src_of = np.zeros(256, np.uint8)
        _call("todhip_db_bit_order", self._h, _np_ptr(src_of))
        return src_of

    def set_kernel_timing(self, enable):
        _call("todhip_set_kernel_timing", self._h, 1 if enable else 0)

    # ---------------------------------------------------------------- stage B
    def db_load(self, desc, pts, obj_off, shard_rank=0, shard_count=1):
        """desc u8[N,32] (256-bit binary: ORB) or u8[N,64] (512-bit binary: BRISK, FREAK; AKAZE's 61 bytes zero-padded to 64), both
        Hamming, or f32[N,128] (float, L2); pts f32[N,3], obj_off u32[n_obj+1] (rows of object o are obj_off[o]:obj_off[o+1]).
        f32[N,64] (SURF, KAZE) is the narrower float DB, desc_bytes 256: every float call serves it as it serves 128.
        The width of desc is the DB's desc_bytes: the match calls take queries of that width."""
        desc = np.ascontiguousarray(desc, np.float32 if np.asarray(desc).dtype == np.float32 else np.uint8)
        pts = np.ascontiguousarray(pts, np.float32)
        objs, n_obj, B = _objects(desc, pts, obj_off)
        spans = np.zeros(max(n_obj, 1), np.float32)
        _call("todhip_db_load", self._h, objs, n_obj, B, shard_rank, shard_count, _np_ptr(spans))
        return spans[:n_obj]

    def db_load_models(self, models, shard_rank=0, shard_count=1):
        """Object DB straight from trained models (capi.Model) in this device's memory: no host copy of descriptors or points
        (todhip_model_device + todhip_db_load_device). Returns (spans, obj_off)."""
        objs, off = _model_objects(models)
        spans = np.zeros(len(models), np.float32)
        _call("todhip_db_load_device", self._h, objs, len(models), 32, shard_rank, shard_count, _np_ptr(spans))
        return spans, off

    def db_info(self):
        tot, first, rows, nobj = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint32()
        _call("todhip_db_info", self._h, C.byref(tot), C.byref(first), C.byref(rows), C.byref(nobj))
        return dict(total_rows=tot.value, shard_first=first.value, shard_rows=rows.value, n_objs=nobj.value)

    def desc_bytes(self):
        """Bytes per row of the resident DB (32, 64 or 512; 0 before the first load): todhip_db_desc_bytes. 256: the float DB of
        64 x f32 rows."""
        b = C.c_uint32()
        _call("todhip_db_desc_bytes", self._h, C.byref(b))
        return b.value

    def _query_rows(self, q_desc, dtype, what):
        """q_desc as contiguous dtype[nq, width]: u8 for a binary DB (32 or 64 bytes a row), f32 for a float DB (64 or 128 a row). A
        query matrix of another width than such a DB's is refused here with TodError(EINVAL): the library sees a pointer and would
        read it at the DB's stride."""
        q = np.ascontiguousarray(q_desc, dtype)
        B, is_float = self.desc_bytes(), q.itemsize == 4
        if B in ((256, 512) if is_float else (32, 64)) and q.ndim == 2 and q.shape[1] * q.itemsize != B:
            raise TodError(EINVAL, "%s (queries of shape %s against a DB of %s descriptors)"
                           % (what, q.shape, "%d x f32" % (B // 4) if is_float else "%d-byte" % B))
        return q

    def select_objects(self, ids):
        """Search only the rows of the listed objects (indices of the last db_load, any order, repeats allowed) from now on; None:
        all objects again, []: nothing. imgIdx and the sharded keys keep the numbering of the full DB (todhip_db_select_objects)."""
        p, n, keep = _ids_in(ids)
        _call("todhip_db_select_objects", self._h, p, n)

    def selection(self):
        """dict(n_objs, rows, shard_rows): the distinct selected objects, their rows in the whole DB and in this context's shard"""
        n, rows, srows = C.c_uint32(), C.c_uint64(), C.c_uint64()
        _call("todhip_db_selection", self._h, C.byref(n), C.byref(rows), C.byref(srows))
        return dict(n_objs=n.value, rows=rows.value, shard_rows=srows.value)

    def _match_host(self, name, q, k, radius):
        nq = q.shape[0]
        row_ptr = np.zeros(nq + 1, np.uint32)
        m = np.zeros(max(nq * k, 1), DMATCH_DTYPE)
        xyz = np.zeros((max(nq * k, 1), 3), np.float32)
        _call(name, self._h, _np_ptr(q), nq, k, radius, _np_ptr(row_ptr), _np_ptr(m), _np_ptr(xyz))
        n = int(row_ptr[nq])
        return row_ptr, m[:n].copy(), xyz[:n].copy()

    def match(self, q_desc, k, radius):
        """Host-buffer form: q_desc u8[nq, 32] or u8[nq, 64] -- the query width must equal the DB's (desc_bytes(); TodError(EINVAL)
        otherwise). On a 64-byte DB distances run 0 ... 512 and a radius >= 512 cuts nothing.
        Returns (row_ptr u32[nq+1], matches DMATCH[n], xyz f32[n,3])."""
        return self._match_host("todhip_match", self._query_rows(q_desc, np.uint8, "todhip_match"), k, radius)

    def match_radius(self, q_desc, radius, max_per_query):
        """The true radius search, host-buffer form (todhip_match_radius): every searched row within `radius` bits, the nearest
        max_per_query of them per query. Returns (row_ptr u32[nq+1], matches DMATCH[n], xyz f32[n,3], in_radius u32[nq])."""
        q = np.ascontiguousarray(q_desc, np.uint8)
        nq = q.shape[0]
        cap = max(nq * max_per_query, 1)
        row_ptr, in_radius = np.zeros(nq + 1, np.uint32), np.zeros(nq, np.uint32)
        m, xyz = np.empty(cap, DMATCH_DTYPE), np.empty((cap, 3), np.float32)
        n = C.c_uint32(cap)
        _call("todhip_match_radius", self._h, _np_ptr(q), nq, radius, max_per_query, _np_ptr(row_ptr), _np_ptr(m), _np_ptr(xyz),
              C.byref(n), _np_ptr(in_radius))
        return row_ptr, m[:n.value].copy(), xyz[:n.value].copy(), in_radius

    def match_radius_device(self, d_q, nq, radius, max_per_query, d_counts, d_matches, d_xyz, d_in_radius=None):
        """Device-pointer form (ints from tensor.data_ptr()), fixed stride max_per_query; d_in_radius may be None."""
        _call("todhip_match_radius_device", self._h, d_q, nq, radius, max_per_query, d_counts, d_matches, d_xyz, d_in_radius)

    def match_radius_shard_device(self, d_q, nq, radius, max_per_query, d_keys):
        """The sharded radius search, step 1: this context's shard -> d_keys u64[nq, max_per_query + 1] (ascending keys
        distance << 32 | row of the full DB, UINT64_MAX padding, the shard's exact count in the last slot; every slot written)."""
        _call("todhip_match_radius_shard_device", self._h, d_q, nq, radius, max_per_query, d_keys)

    def _merge(self, name, stream, *args):
        """A merge of shard keys on the context's stream, or (its _on form) on a HIP stream of the caller's: the merges only read the
        context's immutable tables"""
        if stream is None:
            _call(name, self._h, *args)
        else:
            _call(name + "_on", self._h, stream, *args)

    def merge_radius_shards_device(self, d_keys_all, n_shards, nq, max_per_query, d_counts, d_matches, d_xyz, d_in_radius=None, stream=None):
        """Step 2: d_keys_all u64[n_shards, nq, max_per_query + 1] -> what match_radius_device leaves on the unsharded DB.
        stream: as merge_shards_device."""
        self._merge("todhip_merge_radius_shards_device", stream, d_keys_all, n_shards, nq, max_per_query, d_counts, d_matches, d_xyz, d_in_radius)

    def merge_radius_shards_device_on(self, stream, d_keys_all, n_shards, nq, max_per_query, d_counts, d_matches, d_xyz, d_in_radius=None):
        """The same merge on a stream of the caller's (it only reads the context's immutable tables)."""
        self.merge_radius_shards_device(d_keys_all, n_shards, nq, max_per_query, d_counts, d_matches, d_xyz, d_in_radius, stream=stream)

    def match_l2(self, q_desc, k, radius):
        """Float descriptors, host-buffer form. Returns (row_ptr u32[nq+1], matches DMATCH[n], xyz f32[n,3]). q_desc f32[nq, 64] or
        f32[nq, 128]: the query width must equal the DB's (desc_bytes() / 4; TodError(EINVAL) otherwise)."""
        return self._match_host("todhip_match_l2", self._query_rows(q_desc, np.float32, "todhip_match_l2"), k, radius)

    def match_l2_device(self, d_q, nq, k, radius, d_counts, d_matches, d_xyz):
        _call("todhip_match_l2_device", self._h, d_q, nq, k, radius, d_counts, d_matches, d_xyz)

    def match_l2_radius(self, q_desc, radius, max_per_query):
        """The true L2 radius search over a float DB, host-buffer form (todhip_match_l2_radius): every row whose distance is not
        > radius, the nearest max_per_query of them per query. Returns (row_ptr u32[nq+1], matches DMATCH[n], xyz f32[n,3],
        in_radius u32[nq]). The output buffers start at 16 matches per query and grow to the count the library asks for. The query
        width must equal the DB's, as in match_l2."""
        q = self._query_rows(q_desc, np.float32, "todhip_match_l2_radius")
        nq = q.shape[0]
        row_ptr, in_radius = np.zeros(nq + 1, np.uint32), np.zeros(nq, np.uint32)
        cap = max(nq * min(max_per_query, 16), 1)
        while True:
            m, xyz = np.empty(cap, DMATCH_DTYPE), np.empty((cap, 3), np.float32)
            n = C.c_uint32(cap)
            rc = lib().todhip_match_l2_radius(self._h, _np_ptr(q), nq, radius, max_per_query, _np_ptr(row_ptr), _np_ptr(m), _np_ptr(xyz),
                                              C.byref(n), _np_ptr(in_radius))
            if rc != ECAPACITY or n.value <= cap:
                break
            cap = n.value                                                 # the needed count: the same call fits now
        if rc != OK:
            raise TodError(rc, "todhip_match_l2_radius")
        return row_ptr, m[:n.value].copy(), xyz[:n.value].copy(), in_radius

    def match_l2_radius_device(self, d_q, nq, radius, max_per_query, d_counts, d_matches, d_xyz, d_in_radius=None):
        """Device-pointer form (ints from tensor.data_ptr()), fixed stride max_per_query; d_in_radius may be None."""
        _call("todhip_match_l2_radius_device", self._h, d_q, nq, radius, max_per_query, d_counts, d_matches, d_xyz, d_in_radius)

    def match_l2_shard_device(self, d_q, nq, k, d_keys):
        """The sharded float k-NN search, step 1: this context's shard -> d_keys u64[nq, k] (ascending keys
        binary32 bits of d2 << 32 | row of the full DB, UINT64_MAX padding; the plain top-k, every slot written)."""
        _call("todhip_match_l2_shard_device", self._h, d_q, nq, k, d_keys)

    def merge_l2_shards_device(self, d_keys_all, n_shards, nq, k, radius, d_counts, d_matches, d_xyz, stream=None):
        """Step 2: d_keys_all u64[n_shards, nq, k] -> what match_l2_device leaves on the unsharded DB. stream: as merge_shards_device."""
        self._merge("todhip_merge_l2_shards_device", stream, d_keys_all, n_shards, nq, k, radius, d_counts, d_matches, d_xyz)

    def match_l2_radius_shard_device(self, d_q, nq, radius, max_per_query, d_keys):
        """The sharded float radius search, step 1: this context's shard -> d_keys u64[nq, max_per_query + 1] (ascending keys,
        UINT64_MAX padding, the shard's exact count in the last slot; every slot written)."""
        _call("todhip_match_l2_radius_shard_device", self._h, d_q, nq, radius, max_per_query, d_keys)

    def merge_l2_radius_shards_device(self, d_keys_all, n_shards, nq, max_per_query, d_counts, d_matches, d_xyz, d_in_radius=None,
                                      stream=None):
        """Step 2: d_keys_all u64[n_shards, nq, max_per_query + 1] -> what match_l2_radius_device leaves on the unsharded DB.
        stream: as merge_shards_device."""
        self._merge("todhip_merge_l2_radius_shards_device", stream, d_keys_all, n_shards, nq, max_per_query, d_counts, d_matches, d_xyz,
                    d_in_radius)

    def match_device(self, d_q, nq, k, radius, d_counts, d_matches, d_xyz):
        """Device-pointer form (ints from tensor.data_ptr()). d_q: nq rows of the DB's width, 32 or 64 bytes (desc_bytes()) -- the
        query width must equal the DB's, and a pointer carries no shape: the caller answers for it."""
        _call("todhip_match_device", self._h, d_q, nq, k, radius, d_counts, d_matches, d_xyz)

    def cross_check_device(self, d_q, nq, frame_queries, stride, d_counts, d_matches, d_xyz, frame_nq=None):
        """The cross-check filter in place on a fixed-stride device output (todhip_cross_check_device): a match stays only where its
        query is the nearest valid query of its frame (frame_queries rows each) to the DB row it names, ties to the lower query
        index. frame_nq: per frame, how many of its first rows compete (None: all). Asynchronous on the context's stream."""
        fn = _frame_limits(frame_nq, nq, frame_queries, "todhip_cross_check_device")
        _call("todhip_cross_check_device", self._h, d_q, nq, frame_queries, _np_ptr(fn), stride, d_counts, d_matches, d_xyz)

    def set_cross_check(self, frame_queries):
        """match() and match_device() run the cross-check behind their finalize step, in frames of frame_queries query rows (0 = off,
        the default). The sharded and radius forms ignore it: filter their outputs with cross_check_device."""
        _call("todhip_set_cross_check", self._h, frame_queries)

    def set_l2_ratio_test(self, ratio):
        """Lowe's ratio test of the float forms (todhip_set_l2_ratio_test; 0 = off, the default; 0 < ratio <= 1 = on): match_l2,
        match_l2_device and merge_l2_shards_device drop every match of a query whose two nearest rows over the whole DB do not
        satisfy sqrtf(d2_1) < ratio * sqrtf(d2_2) in binary32. k == 1 searches two rows and returns one; match_l2_shard_device and
        the merge refuse k < 2 while it is on. The radius forms ignore it. set_ratio_test does not apply to the float forms."""
        _call("todhip_set_l2_ratio_test", self._h, ratio)

    def cross_check_l2_device(self, d_q, nq, frame_queries, stride, d_counts, d_matches, d_xyz, frame_nq=None):
        """The cross-check filter over a float DB, in place on a fixed-stride device output of match_l2_device,
        match_l2_radius_device or either float merge (todhip_cross_check_l2_device): cross_check_device's definition with the
        binary32 bits of the exact d2 as the distance. d_q: the nq query rows of 128 f32. frame_nq: per frame, how many of its
        first rows compete (None: all). Asynchronous on the context's stream. On a DB of 64 x f32 rows the query rows are 64 f32.
        d_q may also be the device tensor itself (anything with .shape and .data_ptr()): its width is then checked against the DB's
        (TodError(EINVAL)) before the library reads it -- a bare pointer carries no shape and the caller answers for it."""
        if hasattr(d_q, "data_ptr"):
            B = self.desc_bytes()
            if B in (256, 512) and (len(d_q.shape) != 2 or d_q.shape[1] * 4 != B or d_q.shape[0] < nq):
                raise TodError(EINVAL, "todhip_cross_check_l2_device (queries of shape %s against a DB of %d x f32 descriptors)" % (tuple(d_q.shape), B // 4))
            d_q = d_q.data_ptr()
        fn = _frame_limits(frame_nq, nq, frame_queries, "todhip_cross_check_l2_device")
        _call("todhip_cross_check_l2_device", self._h, d_q, nq, frame_queries, _np_ptr(fn), stride, d_counts, d_matches, d_xyz)

    def set_l2_cross_check(self, frame_queries):
        """match_l2() and match_l2_device() run the float cross-check behind their finalize step -- behind the ratio test and the
        radius cut -- in frames of frame_queries query rows (0 = off, the default). The shard, merge and radius forms ignore it:
        filter their outputs with cross_check_l2_device. set_cross_check does not apply to the float forms."""
        _call("todhip_set_l2_cross_check", self._h, frame_queries)

    def match_shard_device(self, d_q, nq, k, radius, d_keys):
        _call("todhip_match_shard_device", self._h, d_q, nq, k, radius, d_keys)

    def merge_shards_device(self, d_keys_all, n_shards, nq, k, radius, d_counts, d_matches, d_xyz, stream=None):
        """stream: a HIP stream of the caller's instead of the context's (the merge only reads the context's immutable tables)."""
        self._merge("todhip_merge_shards_device", stream, d_keys_all, n_shards, nq, k, radius, d_counts, d_matches, d_xyz)

    def merge_shards_device_on(self, stream, d_keys_all, n_shards, nq, k, radius, d_counts, d_matches, d_xyz):
        """The merge on a stream of the caller's (it only reads the context's immutable tables)."""
        self.merge_shards_device(d_keys_all, n_shards, nq, k, radius, d_counts, d_matches, d_xyz, stream=stream)

    # ---------------------------------------------------------------- stage C
    def _verify(self, name, front, n_kp, spans, min_inliers, n_iter, err, rng, max_poses, n_frames=None, cache=False):
        """Every verify* call: `front` are the function's arguments between the context and spans, n_kp the keypoints of a frame. The
        numpy arrays in `front` go over as their pointers (`ptrs`); the parameter `front` stays bound to the tuple until this
        function returns, and the tuple holds the arrays, so a temporary such as _k9(K) in a caller's tuple lives through the call.
        n_frames None: one frame, rng one Rng, -> list of pose dicts. n_frames given: the batch form, rng a ctypes array
        Rng * n_frames, -> that list per frame. cache: keep the inlier array in the context between calls."""
        ptrs = [_np_ptr(a) if isinstance(a, np.ndarray) else a for a in front]
        sp, prm = np.ascontiguousarray(spans, np.float32), VerifyParams(min_inliers, n_iter, err)
        poses, n_poses, inl, n_inl, pose_ptr = _pose_out(max_poses, n_kp, n_frames, self if cache else None)
        if n_frames is None:
            _call(name, self._h, *ptrs, _np_ptr(sp), len(sp), C.byref(prm), C.byref(rng), poses, C.byref(n_poses), _np_ptr(inl), C.byref(n_inl))
            return _pose_list(poses, 0, n_poses.value, inl)
        _call(name, self._h, *ptrs, _np_ptr(sp), len(sp), C.byref(prm), rng, poses, C.byref(n_poses), pose_ptr, _np_ptr(inl), C.byref(n_inl))
        return [_pose_list(poses, pose_ptr[f], pose_ptr[f + 1], inl) for f in range(n_frames)]

    def verify(self, kp_xy, cloud, row_ptr, matches, matches_xyz, spans, min_inliers, n_iter, err, rng,
               max_poses=64):
        kp = np.ascontiguousarray(kp_xy, np.float32)
        cloud = np.ascontiguousarray(cloud, np.float32)
        H, W = (cloud.shape[0], cloud.shape[1]) if cloud.ndim == 3 else (0, 0)
        front = (kp, len(kp), cloud, H, W, np.ascontiguousarray(row_ptr, np.uint32), np.ascontiguousarray(matches, DMATCH_DTYPE),
                 np.ascontiguousarray(matches_xyz, np.float32))
        return self._verify("todhip_verify", front, len(kp), spans, min_inliers, n_iter, err, rng, max_poses)

    def verify_2d(self, kp_xy, K, row_ptr, matches, matches_xyz, spans, min_inliers, n_iter, err_px, rng, max_poses=64):
        """The 2D-only branch (no cloud): todhip_verify_2d. err_px: reprojection threshold in pixels."""
        kp = np.ascontiguousarray(kp_xy, np.float32)
        front = (kp, len(kp), _k9(K), np.ascontiguousarray(row_ptr, np.uint32), np.ascontiguousarray(matches, DMATCH_DTYPE),
                 np.ascontiguousarray(matches_xyz, np.float32))
        return self._verify("todhip_verify_2d", front, len(kp), spans, min_inliers, n_iter, err_px, rng, max_poses)

    def verify_2d_device(self, d_kp_xy, nq, K, d_counts, d_matches, d_xyz, k, spans, min_inliers, n_iter, err_px, rng, max_poses=64):
        return self._verify("todhip_verify_2d_device", (d_kp_xy, nq, _k9(K), d_counts, d_matches, d_xyz, k), nq, spans, min_inliers, n_iter,
                            err_px, rng, max_poses)

    def verify_2d_batch_device(self, n_frames, d_kp_xy, nq, K, d_counts, d_matches, d_xyz, k, spans, min_inliers, n_iter, err_px, rngs,
                               max_poses=16):
        """rngs: ctypes array (Rng * n_frames). Returns a list (per frame) of lists of pose dicts."""
        return self._verify("todhip_verify_2d_batch_device", (n_frames, d_kp_xy, nq, _k9(K), d_counts, d_matches, d_xyz, k), nq, spans,
                            min_inliers, n_iter, err_px, rngs, max_poses, n_frames)

    def verify_device(self, d_kp_xy, nq, d_cloud, H, W, d_counts, d_matches, d_xyz, k, spans, min_inliers, n_iter,
                      err, rng, max_poses=64):
        """Device-pointer form (ints from tensor.data_ptr()); poses are returned on the host."""
        return self._verify("todhip_verify_device", (d_kp_xy, nq, d_cloud, H, W, d_counts, d_matches, d_xyz, k), nq, spans, min_inliers,
                            n_iter, err, rng, max_poses, cache=True)

    def verify_device_depth(self, d_kp_xy, nq, d_depth, depth_is_u16, H, W, K, d_counts, d_matches, d_xyz, k, spans,
                            min_inliers, n_iter, err, rng, max_poses=64):
        return self._verify("todhip_verify_device_depth", (d_kp_xy, nq, d_depth, 1 if depth_is_u16 else 0, H, W, _k9(K), d_counts, d_matches,
                                                           d_xyz, k), nq, spans, min_inliers, n_iter, err, rng, max_poses)

    def verify_batch_device(self, n_frames, d_kp_xy, nq, d_cloud, H, W, d_counts, d_matches, d_xyz, k, spans, min_inliers,
                            n_iter, err, rngs, max_poses=16, depth=None):
        """rngs: ctypes array (Rng * n_frames). depth = (d_depth, is_u16, K) selects the depth form (d_cloud ignored).
        Returns a list (per frame) of lists of pose dicts."""
        if depth is None:
            name, image = "todhip_verify_batch_device", (d_cloud, H, W)
        else:
            name, image = "todhip_verify_batch_device_depth", (depth[0], 1 if depth[1] else 0, H, W, _k9(depth[2]))
        return self._verify(name, (n_frames, d_kp_xy, nq) + image + (d_counts, d_matches, d_xyz, k), nq, spans, min_inliers, n_iter, err,
                            rngs, max_poses, n_frames, cache=True)

    def verify_device_depth_rescaled(self, d_kp_xy, nq, d_depth, depth_is_u16, dH, dW, nearest, H, W, K, d_counts, d_matches, d_xyz, k,
                                     spans, min_inliers, n_iter, err, rng, max_poses=64):
        """verify_device_depth on a dH x dW depth image: the result of rescale_depth_device followed by verify_device_depth, without
        the H x W intermediate (H, W, K: the image's)."""
        front = (d_kp_xy, nq, d_depth, 1 if depth_is_u16 else 0, dH, dW, 1 if nearest else 0, H, W, _k9(K), d_counts, d_matches, d_xyz, k)
        return self._verify("todhip_verify_device_depth_rescaled", front, nq, spans, min_inliers, n_iter, err, rng, max_poses)

    def verify_batch_device_depth_rescaled(self, n_frames, d_kp_xy, nq, d_depth, depth_is_u16, dH, dW, nearest, H, W, K, d_counts,
                                           d_matches, d_xyz, k, spans, min_inliers, n_iter, err, rngs, max_poses=16):
        """The batch form (d_depth: n_frames x dH x dW, rngs: ctypes array Rng * n_frames); a list per frame of lists of pose dicts."""
        front = (n_frames, d_kp_xy, nq, d_depth, 1 if depth_is_u16 else 0, dH, dW, 1 if nearest else 0, H, W, _k9(K), d_counts, d_matches,
                 d_xyz, k)
        return self._verify("todhip_verify_batch_device_depth_rescaled", front, nq, spans, min_inliers, n_iter, err, rngs, max_poses,
                            n_frames, cache=True)

    def test_depth_lookup(self, d_depth, depth_is_u16, dH, dW, nearest, H, W, kp_xy, fill=0.0):
        """z (f32 [n]) of the verifier's depth lookup at the pixel positions kp_xy [n, 2]. Returns (status, z): OK, or ERANGE when a
        position lies outside the H x W image (its z keeps `fill`)."""
        kp = np.ascontiguousarray(kp_xy, np.float32).reshape(-1, 2)
        z = np.full(len(kp), fill, np.float32)
        rc = lib().todhip_test_depth_lookup(self._h, d_depth, 1 if depth_is_u16 else 0, dH, dW, 1 if nearest else 0, H, W, _np_ptr(kp),
                                            len(kp), _np_ptr(z))
        if rc not in (OK, ERANGE):
            raise TodError(rc, "todhip_test_depth_lookup")
        return rc, z

    def verify_trace(self, cap=4096):
        arr = (RoundTrace * cap)()
        n = C.c_uint32(cap)
        _call("todhip_verify_trace", self._h, arr, C.byref(n))
        return [arr[i] for i in range(n.value)]

    def test_adjacency(self, train, query, kp_per_match, span, err):
        t = np.ascontiguousarray(train, np.float32)
        q = np.ascontiguousarray(query, np.float32)
        kp = np.ascontiguousarray(kp_per_match, np.float32)
        n = len(t)
        W = (n + 63) // 64
        phys = np.zeros((n, W), np.uint64)
        samp = np.zeros((n, W), np.uint64)
        _call("todhip_test_adjacency", self._h, _np_ptr(t), _np_ptr(q), _np_ptr(kp), n, span, err, _np_ptr(phys), _np_ptr(samp))
        return phys, samp

    def test_consensus(self, train, query, kp_per_match, span, err, triples, stop_level=0, dbg_stride=0):
        t = np.ascontiguousarray(train, np.float32)
        q = np.ascontiguousarray(query, np.float32)
        kp = np.ascontiguousarray(kp_per_match, np.float32)
        tr = np.ascontiguousarray(triples, np.uint32).reshape(-1, 3)
        counts = np.zeros(len(tr), np.int32)
        dbg = np.zeros((len(tr), dbg_stride), np.uint32) if dbg_stride else None
        _call("todhip_test_consensus", self._h, _np_ptr(t), _np_ptr(q), _np_ptr(kp), len(t), span, err, _np_ptr(tr), len(tr), stop_level,
              _np_ptr(counts), _np_ptr(dbg), dbg_stride)
        return counts, dbg

    def test_draw_table(self, samp, valid, n, rnd, S, form=0):
        """The draw table of one object (todhip_test_draw_table): samp u64 [n, W], valid u64 [W], rnd u32 [window_len]. Returns
        (status, entries u32 [S, 6]): OK, or EINVAL when `form` (0 routing, 1 lane, 2 wave of one slice, 3 of eight, 4 eight-word lane)
        cannot hold n matches."""
        W = (n + 63) // 64
        samp = np.ascontiguousarray(samp, np.uint64).reshape(n, W)
        valid = np.ascontiguousarray(valid, np.uint64).reshape(W)
        rnd = np.ascontiguousarray(rnd, np.uint32).reshape(-1)
        out = np.zeros((S, 6), np.uint32)
        rc = lib().todhip_test_draw_table(self._h, _np_ptr(samp), _np_ptr(valid), n, _np_ptr(rnd), len(rnd), S, form, _np_ptr(out))
        if rc not in (OK, EINVAL):
            raise TodError(rc, "todhip_test_draw_table")
        return rc, out

    def test_kabsch(self, Hd, Cc):
        """kabsch_solve alone (todhip_test_kabsch): Hd f64 [n, 3, 3] correlation matrices, Cc f32 [n, 6] centroids (train, query).
        Returns R f32 [n, 3, 3], T f32 [n, 3], query -> train, before the inversion."""
        Hd = np.ascontiguousarray(Hd, np.float64).reshape(-1, 9)
        Cc = np.ascontiguousarray(Cc, np.float32).reshape(-1, 6)
        assert len(Hd) == len(Cc)
        R = np.zeros((len(Hd), 9), np.float32)
        T = np.zeros((len(Hd), 3), np.float32)
        _call("todhip_test_kabsch", self._h, len(Hd), _np_ptr(Hd), _np_ptr(Cc), _np_ptr(R), _np_ptr(T))
        return R.reshape(-1, 3, 3), T

    def test_clique(self, m, edges, minimal_size=0xFFFFFFFF, gate=False):
        e = np.ascontiguousarray(np.asarray(edges, np.uint32).reshape(-1, 2))
        out = np.zeros(3, np.uint32)
        _call("todhip_test_clique_gate" if gate else "todhip_test_clique", self._h, m, _np_ptr(e), len(e), minimal_size, _np_ptr(out))
        return int(out[0]), int(out[1]), int(out[2])

    # ---------------------------------------------------------------- stage A
    def orb(self, gray, n_features=1000, n_levels=3, scale_factor=1.2, pattern=None, mask=None, cap=None, stride=None, W=None):
        """todhip_orb_masked. cap: output capacity (default n_features). stride: gray (and mask) are 2-D arrays of that row pitch in
        bytes whose first W columns (default: all) are the image; they are passed as they are, not copied, so a view that ends with
        the last row's W pixels is what the library gets."""
        if stride is None:
            g = np.ascontiguousarray(gray, np.uint8)
            mk = _opt(mask, np.uint8)
            H, W = g.shape
            stride = W
        else:
            g, H, W = _strided_rows(gray, stride, W)
            mk = None if mask is None else _strided_rows(mask, stride, W)[0]
        cap = n_features if cap is None else cap
        kp = np.zeros((max(cap, 1), 2), np.float32)
        aux = np.zeros((max(cap, 1), 4), np.float32)
        desc = np.zeros((max(cap, 1), 32), np.uint8)
        n_out = C.c_uint32(cap)
        pat = _opt(pattern, np.int8)
        _call("todhip_orb_masked", self._h, _np_ptr(g), _np_ptr(mk), H, W, stride, n_features, n_levels, scale_factor, _np_ptr(pat),
              _np_ptr(kp), _np_ptr(aux), _np_ptr(desc), C.byref(n_out))
        n = n_out.value
        return kp[:n].copy(), aux[:n].copy(), desc[:n].copy()

    def orb_device(self, d_gray, H, W, stride, n_features, n_levels, scale_factor, d_kp_xy, d_kp_aux, d_desc, cap, pattern=None):
        n_out = C.c_uint32(cap)
        pat = _opt(pattern, np.int8)
        _call("todhip_orb_device", self._h, d_gray, H, W, stride, n_features, n_levels, scale_factor, _np_ptr(pat), d_kp_xy, d_kp_aux,
              d_desc, C.byref(n_out))
        return n_out.value

    def orb_batch_device(self, d_gray, n_frames, frame_stride, H, W, stride, n_features, n_levels, scale_factor, d_kp_xy, d_kp_aux,
                         d_desc, cap, pattern=None):
        n = (C.c_uint32 * n_frames)()
        pat = _opt(pattern, np.int8)
        _call("todhip_orb_batch_device", self._h, d_gray, n_frames, frame_stride, H, W, stride, n_features, n_levels, scale_factor,
              _np_ptr(pat), d_kp_xy, d_kp_aux, d_desc, cap, n)
        return list(n)

    def orb_batch_device_masked(self, d_gray, d_mask, n_frames, frame_stride, H, W, stride, n_features, n_levels, scale_factor, d_kp_xy,
                                d_kp_aux, d_desc, cap, pattern=None):
        """orb_batch_device with a packed mask per frame (d_mask: n_frames x H x W u8 in HBM; None / 0: no masks)."""
        n = (C.c_uint32 * n_frames)()
        pat = _opt(pattern, np.int8)
        _call("todhip_orb_batch_device_masked", self._h, d_gray, d_mask or None, n_frames, frame_stride, H, W, stride, n_features, n_levels,
              scale_factor, _np_ptr(pat), d_kp_xy, d_kp_aux, d_desc, cap, n)
        return list(n)

    def rescale_depth(self, depth, H, W, nearest=False):
        """rescale_depth (Trainer.cpp:62-81): depth [dH, dW] float32 metres / uint16 mm -> [H, W] float32 metres."""
        u16 = depth.dtype == np.uint16
        d = np.ascontiguousarray(depth, np.uint16 if u16 else np.float32)
        out = np.empty((H, W), np.float32)
        _call("todhip_rescale_depth", self._h, _np_ptr(d), 1 if u16 else 0, d.shape[0], d.shape[1], _np_ptr(out), H, W, 1 if nearest else 0)
        return out

    def rescale_depth_device(self, d_depth_in, is_u16, dH, dW, d_depth_out, H, W, nearest=False):
        _call("todhip_rescale_depth_device", self._h, d_depth_in, 1 if is_u16 else 0, dH, dW, d_depth_out, H, W, 1 if nearest else 0)


class Model:
    """One object's model being trained (todhip_model): add observations, then finish() -> (desc, pts)."""

    def __init__(self, ctx, capacity_rows=100000):
        self._ctx = ctx
        self._h = C.c_void_p()
        self._cap = capacity_rows
        _call("todhip_model_begin", ctx._h, capacity_rows, C.byref(self._h))

    def add_observation(self, gray, mask, depth, K, R, T, n_features=500, n_levels=8, scale_factor=1.2, pattern=None):
        g = np.ascontiguousarray(gray, np.uint8)
        mk = np.ascontiguousarray(mask, np.uint8)
        H, W = g.shape
        if tuple(depth.shape) != (H, W):                       # rescale_depth's resize branch (Trainer.cpp:73-80)
            depth = self._ctx.rescale_depth(depth, H, W)
        u16 = depth.dtype == np.uint16
        d = np.ascontiguousarray(depth, np.uint16 if u16 else np.float32)
        K9 = _k9(K)
        R9 = np.ascontiguousarray(R, np.float32).reshape(9)
        T3 = np.ascontiguousarray(T, np.float32).reshape(3)
        n = C.c_uint32(0)
        pat = _opt(pattern, np.int8)
        _call("todhip_model_add_observation", self._ctx._h, self._h, _np_ptr(g), _np_ptr(mk), _np_ptr(d), 1 if u16 else 0, H, W, _np_ptr(K9),
              _np_ptr(R9), _np_ptr(T3), n_features, n_levels, scale_factor, _np_ptr(pat), C.byref(n))
        return n.value

    def add_observations_device(self, d_gray, d_mask, d_depth, n_views, H, W, K, R, T, *, stride=None, frame_stride=None,
                                depth_is_u16=False, depth_size=None, nearest=False, n_features=500, n_levels=8, scale_factor=1.2,
                                pattern=None):
        """n_views device-resident views in one call (todhip_model_add_observations_device): the model afterwards is the model after
        add_observation per view, in order. d_gray, d_mask, d_depth: device pointers -- view v's image at d_gray + v * frame_stride
        (default H * stride) with row pitch stride (default W), masks n_views x H x W u8 packed, depth n_views x dH x dW packed,
        float32 metres or (depth_is_u16) uint16 millimetres, depth_size = (dH, dW) or None for the image's size. K: one 3 x 3 matrix
        for all views or n_views of them; R: n_views x 3 x 3; T: n_views x 3 (host arrays). -> uint32[n_views]: rows added per view."""
        stride = W if stride is None else stride
        frame_stride = H * stride if frame_stride is None else frame_stride
        dH, dW = (0, 0) if depth_size is None else depth_size
        K9 = np.ascontiguousarray(K, np.float32).reshape(-1)
        if K9.size == 9:
            K9 = np.ascontiguousarray(np.tile(K9, max(n_views, 1)))
        R9 = np.ascontiguousarray(R, np.float32).reshape(-1)
        T3 = np.ascontiguousarray(T, np.float32).reshape(-1)
        if n_views and (K9.size != 9 * n_views or R9.size != 9 * n_views or T3.size != 3 * n_views):
            raise ValueError("K, R, T do not hold n_views cameras")
        n = np.zeros(max(n_views, 1), np.uint32)
        pat = _opt(pattern, np.int8)
        _call("todhip_model_add_observations_device", self._ctx._h, self._h, d_gray or None, frame_stride, stride, d_mask or None,
              d_depth or None, 1 if depth_is_u16 else 0, dH, dW, 1 if nearest else 0, n_views, H, W, _np_ptr(K9), _np_ptr(R9), _np_ptr(T3),
              n_features, n_levels, scale_factor, _np_ptr(pat), _np_ptr(n))
        return n[:n_views].copy()

    def add_rows(self, desc, pts):
        """Already-trained rows (desc u8[n, 32], pts f32[n, 3]) behind the model's rows, cut at its capacity -> rows added."""
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        p = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
        if len(d) != len(p):
            raise ValueError("desc and pts differ in rows")
        n = C.c_uint32(0)
        _call("todhip_model_add_rows", self._ctx._h, self._h, _np_ptr(d) if len(d) else None, _np_ptr(p) if len(d) else None, len(d),
              C.byref(n))
        return n.value

    def compact(self, merge_dist, max_hamming=DEFAULT_COMPACT_HAMMING, want_support=False):
        """Merge near-duplicate rows in place (todhip_model_compact: a row goes when a kept row before it lies within merge_dist of its
        point and within max_hamming bits of its descriptor) -> (rows_before, rows_after[, support u32[rows_after]])."""
        before, after, ns = C.c_uint32(0), C.c_uint32(0), C.c_uint32(self._cap if want_support else 0)
        sup = np.zeros(max(self._cap, 1), np.uint32) if want_support else None
        _call("todhip_model_compact", self._ctx._h, self._h, merge_dist, max_hamming, C.byref(before), C.byref(after), _np_ptr(sup),
              C.byref(ns))
        if want_support:
            return before.value, after.value, sup[:ns.value].copy()
        return before.value, after.value

    def device(self):
        """(device pointer of the descriptors, device pointer of the points, rows) -- valid until close()."""
        d, p, n = C.c_void_p(), C.c_void_p(), C.c_uint32()
        _call("todhip_model_device", self._ctx._h, self._h, C.byref(d), C.byref(p), C.byref(n))
        return d.value, p.value, n.value

    def finish(self):
        desc = np.zeros((self._cap, 32), np.uint8)
        pts = np.zeros((self._cap, 3), np.float32)
        n = C.c_uint32(self._cap)
        _call("todhip_model_finish", self._ctx._h, self._h, _np_ptr(desc), _np_ptr(pts), C.byref(n))
        return desc[:n.value].copy(), pts[:n.value].copy()

    def close(self):
        if self._h:
            lib().todhip_model_free(self._ctx._h, self._h)
            self._h = C.c_void_p()


class PatternLearner:
    """An rBRIEF test pattern learned from training views (todhip_pattern_learn_*): add_view() per view, then finish() -> the pattern
    for Context.orb(pattern=...), Model.add_observation(pattern=...) and Pipeline.set_pattern. candidates: int8 [M, 4] tests
    (x0, y0, x1, y1), or None for the built-in set."""

    def __init__(self, ctx, capacity_keypoints=32768, candidates=None):
        self._ctx = ctx
        self._h = C.c_void_p()
        self.n_keypoints = 0
        cand = None if candidates is None else np.ascontiguousarray(candidates, np.int8).reshape(-1, 4)
        _call("todhip_pattern_learn_begin", ctx._h, _np_ptr(cand), 0 if cand is None else len(cand), capacity_keypoints, C.byref(self._h))

    def add_view(self, gray, mask=None, n_features=500, n_levels=8, scale_factor=1.2):
        """The keypoints todhip_orb_masked finds in the view, as many as still fit; returns their number."""
        g = np.ascontiguousarray(gray, np.uint8)
        mk = _opt(mask, np.uint8)
        H, W = g.shape
        return self._add_view("todhip_pattern_learn_add_view", _np_ptr(g), _np_ptr(mk), H, W, W, n_features, n_levels, scale_factor)

    def add_view_device(self, d_gray, d_mask, H, W, stride, n_features=500, n_levels=8, scale_factor=1.2):
        """Device-pointer form (ints from tensor.data_ptr(); d_mask: row stride W, or None)."""
        return self._add_view("todhip_pattern_learn_add_view_device", d_gray, d_mask, H, W, stride, n_features, n_levels, scale_factor)

    def _add_view(self, name, *view):
        n = C.c_uint32(0)
        _call(name, self._ctx._h, self._h, *view, C.byref(n))
        self.n_keypoints += n.value
        return n.value

    def finish(self, order=PATTERN_ORDER_MATCHER):
        """-> dict(pattern i8[256, 4], chosen u32[256], round_of u8[256], n_keypoints, n_candidates, accepted_in_round [6])"""
        pattern, chosen, round_of = np.zeros((256, 4), np.int8), np.zeros(256, np.uint32), np.zeros(256, np.uint8)
        st = PatternStats()
        _call("todhip_pattern_learn_finish", self._ctx._h, self._h, order, _np_ptr(pattern), _np_ptr(chosen), _np_ptr(round_of), C.byref(st))
        return dict(pattern=pattern, chosen=chosen, round_of=round_of, n_keypoints=int(st.n_keypoints), n_candidates=int(st.n_candidates),
                    accepted_in_round=[int(x) for x in st.accepted_in_round])

    def responses(self, first, count):
        """Rows first .. first + count - 1 of the response matrix: u32 [count, ceil(n_keypoints / 32)] (test hook)."""
        words = np.zeros((count, (self.n_keypoints + 31) // 32), np.uint32)
        _call("todhip_pattern_learn_responses", self._ctx._h, self._h, first, count, _np_ptr(words))
        return words

    def close(self):
        if self._h:
            lib().todhip_pattern_learn_free(self._ctx._h, self._h)
            self._h = C.c_void_p()


class _Borrowed(Context):
    """A context somebody else owns (the pipeline's matcher): the setters work, close() does nothing."""

    def __init__(self, handle):
        self._h = C.c_void_p(handle)

    def close(self):
        self._h = C.c_void_p()


def pipeline_params(**kw):
    """todhip_pipeline_default_params with the given fields replaced (K: 3x3 camera matrix, verify: (min_inliers, n_iter, err))."""
    p = PipelineParams()
    _call("todhip_pipeline_default_params", C.byref(p))
    for key, v in kw.items():
        if key == "K":
            p.K9[:] = [float(x) for x in _k9(v)]
        elif key == "verify":
            p.verify = VerifyParams(*v)
        else:
            setattr(p, key, v)
    return p


class Pipeline:
    """ORB -> matcher -> verifier on batches of frames behind submit / wait (todhip_pipeline). Methods return the library's status
    where the protocol makes a non-OK status an answer (submit, wait, db_load); create raises."""

    def __init__(self, device=0, params=None, **kw):
        self.params = params if params is not None else pipeline_params(**kw)
        self._h = C.c_void_p()
        _call("todhip_pipeline_create", device, C.byref(self.params), C.byref(self._h))
        self._n = {}                                                  # ticket -> n_frames

    def close(self):
        if self._h:
            lib().todhip_pipeline_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def matcher(self):
        return _Borrowed(lib().todhip_pipeline_matcher(self._h))

    def db_load(self, desc, pts, obj_off):
        """As Context.db_load, for u8[N,32] only (the ORB stage emits 32 bytes: EINVAL for any other width); returns the status."""
        desc = np.ascontiguousarray(desc, np.uint8)
        pts = np.ascontiguousarray(pts, np.float32)
        objs, n_obj, B = _objects(desc, pts, obj_off)
        return lib().todhip_pipeline_db_load(self._h, objs, n_obj, B)

    def db_load_models(self, models):
        return lib().todhip_pipeline_db_load_device(self._h, _model_objects(models)[0], len(models), 32)

    def set_pattern(self, pattern):
        """The ORB workers' pattern from the next submit on (i8 [256, 4], None = built-in); returns the status (EBUSY while a ticket
        is outstanding)."""
        pat = _opt(pattern, np.int8)
        assert pat is None or pat.size == 1024
        return lib().todhip_pipeline_set_pattern(self._h, _np_ptr(pat))

    def set_cross_check(self, enable):
        """The cross-check behind each step's matcher call, per frame among its n_kp keypoints (todhip_pipeline_set_cross_check).
        Returns the status (EBUSY while a ticket is outstanding)."""
        return lib().todhip_pipeline_set_cross_check(self._h, 1 if enable else 0)

    def select_objects(self, ids):
        """Context.select_objects on the pipeline's matcher, from the next submit on; returns the status (EBUSY while a ticket is
        outstanding)."""
        p, n, keep = _ids_in(ids)
        return lib().todhip_pipeline_select_objects(self._h, p, n)

    def _submit(self, name, n_frames, *buffers):
        """(status, ticket) of a submit call on the buffers (frames, masks where the form has them, depth); remembers an accepted
        ticket's frame count for wait()"""
        t = C.c_uint64(0)
        rc = getattr(lib(), name)(self._h, *buffers, n_frames, C.byref(t))
        if rc == OK:
            self._n[t.value] = n_frames
        return rc, t.value

    def submit(self, frames, depth, n_frames=None):
        """Host form: frames u8 [n, H, W(, 3 | 4)], depth f32 | u16 [n, H, W] as numpy arrays. Returns (status, ticket)."""
        fr = np.ascontiguousarray(frames, np.uint8)
        dp = np.ascontiguousarray(depth, np.uint16 if self.params.depth_is_u16 else np.float32)
        return self._submit("todhip_pipeline_submit", len(fr) if n_frames is None else n_frames, _np_ptr(fr), _np_ptr(dp))

    def set_depth_size(self, dH, dW, nearest=False):
        """A depth image is dH x dW from the next submit on ((0, 0): the image's size); returns the status (EINVAL: a geometry
        rescale_depth refuses, EBUSY while a ticket is outstanding)."""
        return lib().todhip_pipeline_set_depth_size(self._h, dH, dW, 1 if nearest else 0)

    def submit_masked(self, frames, masks, depth, n_frames=None):
        """submit with masks u8 [n, H, W] (None: submit). Returns (status, ticket)."""
        fr = np.ascontiguousarray(frames, np.uint8)
        mk = _opt(masks, np.uint8)
        dp = np.ascontiguousarray(depth, np.uint16 if self.params.depth_is_u16 else np.float32)
        return self._submit("todhip_pipeline_submit_masked", len(fr) if n_frames is None else n_frames, _np_ptr(fr), _np_ptr(mk), _np_ptr(dp))

    def submit_masked_device(self, d_frames, d_masks, d_depth, n_frames):
        """submit_device with d_masks (n x H x W u8 in HBM, None / 0: no masks), read as long as the frames are."""
        return self._submit("todhip_pipeline_submit_masked_device", n_frames, d_frames, d_masks or None, d_depth)

    def submit_device(self, d_frames, d_depth, n_frames):
        """Device form (ints from tensor.data_ptr()); the buffers are read until wait() has returned the ticket's results."""
        return self._submit("todhip_pipeline_submit_device", n_frames, d_frames, d_depth)

    def wait(self, ticket, timeout_ms=0, max_poses=None, max_inliers=None, want_kp=True):
        """Returns (status, result). result (status OK): list per frame of dict(n_kp, kp_xy f32[n_kp, 2] or None, poses = list of pose
        dicts as Context.verify_batch_device returns them). ECAPACITY: result = (poses needed, inlier keypoints needed)."""
        n = self._n.get(ticket, 1)
        nq = self.params.n_features
        cap_p = self.params.max_poses_per_frame * n if max_poses is None else max_poses
        cap_i = cap_p * nq if max_inliers is None else max_inliers
        n_kp = (C.c_uint32 * n)()
        kp = np.zeros((n, nq, 2), np.float32) if want_kp else None
        if getattr(self, "_inl_cap", 0) < max(cap_i, 1):              # kept between calls (megabytes per step; results are copied out)
            self._inl, self._inl_cap = np.zeros(max(cap_i, 1), np.uint32), max(cap_i, 1)
        poses, inl = (Pose * max(cap_p, 1))(), self._inl
        n_poses, n_inl, pose_ptr = C.c_uint32(cap_p), C.c_uint32(cap_i), (C.c_uint32 * (n + 1))()
        rc = lib().todhip_pipeline_wait(self._h, ticket, timeout_ms, n_kp, _np_ptr(kp), poses, C.byref(n_poses), pose_ptr, _np_ptr(inl),
                                        C.byref(n_inl))
        if rc == ECAPACITY:
            return rc, (n_poses.value, n_inl.value)
        if rc != ETIMEOUT:
            self._n.pop(ticket, None)
        if rc != OK:
            return rc, None
        return rc, [dict(n_kp=int(n_kp[f]), kp_xy=None if kp is None else kp[f, :n_kp[f]].copy(),
                         poses=_pose_list(poses, pose_ptr[f], pose_ptr[f + 1], inl)) for f in range(n)]

    def stats(self):
        s = PipelineStats()
        _call("todhip_pipeline_get_stats", self._h, C.byref(s))
        return {name: getattr(s, name) for name, _ in PipelineStats._fields_}


def bgr_to_gray_device(ctx, d_src, channels, H, W, src_stride, d_gray, gray_stride):
    _call("todhip_bgr_to_gray_device", ctx._h, d_src, channels, H, W, src_stride, d_gray, gray_stride)


def set_cu_partition(latency_cus):
    """Reserve the device's last `latency_cus` compute units for latency streams (todhip_set_cu_partition); 0 = none."""
    _call("todhip_set_cu_partition", latency_cus)


def stream_create(device=0, latency=False):
    """A HIP stream handle (int) of the given kind, honouring the CU partition (todhip_stream_create)."""
    out = C.c_void_p()
    _call("todhip_stream_create", device, 1 if latency else 0, C.byref(out))
    return out.value


def rng_new(seed=1):
    r = Rng()
    lib().todhip_rng_seed(C.byref(r), seed)
    return r
