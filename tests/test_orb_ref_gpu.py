"""Stage A of the library against tests/orb_ref.py, the float64 / int64 statement of the published algorithm, under the rules of
orb_ref.compare -- not against the C restatement the kernels were written from, which shares every free choice with them. Every form
(host, device, batch with a row stride, masked), the pyramid parameters and selection sizes of orb_ref.GPU_CASES, three properties no
implementation chooses (transposition, level composition, a permuted pattern), a pattern on the 31 x 31 square and at radius 30, and
the refusal of a pattern outside its domain x^2 + y^2 <= 900 at every entry point that takes one. tests/test_orb_ref_cpu.py holds
the conditions for every input used here: no ambiguous selection boundary, at most 0.5 % of the bits left out."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import orb_ref as R
from test_orb_edges_gpu import DeviceOut, SENTINEL, orb_batch, orb_device, status_of, to_device
from test_orb_gpu import _equal
from tod_amd import capi

pytestmark = pytest.mark.gpu

FIGURES = {}                                                          # the maxima this module measured, printed by every test that adds


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def checked(got, ref, what):
    s = R.compare(got, ref)
    assert ref.ambiguous == []                                        # (the CPU module asserts it for every case: compare() decided all)
    R.merge_stats(FIGURES, s)
    print("%s: n %d, response %.2f u M, angle %.2e deg, left out %.5f | so far %.2f, %.2e, %.5f"
          % (what, s["n"], s["response_err"], s["angle_err"], s["left_out"], FIGURES["response_err"], FIGURES["angle_err"], FIGURES["left_out"]))
    return s


def host(ctx, name):
    img, nf, nl, sf, kw = R.case_args(name)
    return ctx.orb(img, nf, nl, sf, **kw)


# ------------------------------------------------------------------------------------------ the forms
@pytest.mark.parametrize("name", R.GPU_CASES)
def test_host_form(ctx, name):
    got = host(ctx, name)
    checked(got, R.case_ref(name), name)
    img, nf, nl, sf, kw = R.case_args(name)
    _equal(got, O.orb(img, nf, nl, sf, **kw))                         # and the restatement's bits, the left-out ones included


@pytest.mark.parametrize("name", ["rect_150_3", "rect_300_4", "rect_1_3", "rect100_x2"])
def test_device_form(ctx, name):
    img, nf, nl, sf, _ = R.case_args(name)
    n, out = orb_device(ctx, img, nf, nl, sf, nf)
    assert n == R.case_ref(name).n
    got, untouched = out.frame(0, n)
    checked(got, R.case_ref(name), name + " (device)")
    assert untouched
    assert all(np.array_equal(a, b) for a, b in zip(got, host(ctx, name)))


BATCH = ("rect200", "flat200", "rect200_T")


@pytest.mark.parametrize("pad", [0, 24])
def test_batch_of_three_frames(ctx, pad):
    """the rectangle image padded to 200 x 200, a flat frame and the first one's transpose, packed and at a row stride above W"""
    imgs = [R.image(R.CASES[k][0]) for k in BATCH]
    _, nf, nl, sf, _, _ = R.CASES[BATCH[0]]
    n, out = orb_batch(ctx, imgs, nf, nl, sf, nf, stride=200 + pad, frame_stride=200 * (200 + pad) + (5 if pad else 0))
    assert n == [R.case_ref(k).n for k in BATCH] and n[1] == 0
    for f, k in enumerate(BATCH):
        got, untouched = out.frame(f, n[f])
        checked(got, R.case_ref(k), "%s (batch, pad %d)" % (k, pad))
        assert untouched, k


def test_masked_forms(ctx):
    """host form (with the other cases above) and the batch form with a mask per frame: the masked frame beside an unmasked-by-an-
    open-mask one"""
    img, nf, nl, sf, kw = R.case_args("rect_masked")
    mask = kw["mask"]
    ref = R.case_ref("rect_masked")
    got = ctx.orb(img, nf, nl, sf, mask=mask)
    checked(got, ref, "rect_masked (host)")
    lvl0 = got[1][:, 3] == 0
    assert lvl0.sum() > 20 and (mask[got[0][lvl0, 1].astype(int), got[0][lvl0, 0].astype(int)] != 0).all()
    d_img = to_device(np.stack([img, img]))
    d_mask = to_device(np.stack([mask, np.full_like(mask, 7)]))
    out = DeviceOut(2, nf)
    n = ctx.orb_batch_device_masked(d_img.data_ptr(), d_mask.data_ptr(), 2, img.size, *img.shape, img.shape[1], nf, nl, sf, *out.ptrs(), nf)
    assert n == [ref.n, R.case_ref("rect_150_3").n]
    for f, k in enumerate(("rect_masked", "rect_150_3")):
        b_got, untouched = out.frame(f, n[f])
        checked(b_got, R.case_ref(k), k + " (masked batch)")
        assert untouched
    assert all(np.array_equal(a, b) for a, b in zip(out.frame(0, n[0])[0], got))


# ------------------------------------------------------------------------------------------ properties
def test_transposition(ctx):
    a, b = host(ctx, "rect_all_1"), host(ctx, "rect_T_all_1")
    d = R.transposition_holds(a, b, R.case_ref("rect_all_1"))
    print("transposed angles: %.2e degrees" % d)


@pytest.mark.parametrize("name", ["rect_150_3", "rect_300_4"])
def test_level_composition(ctx, name):
    """level l of an L-level call against the one-level call on the statement's resized image with that level's quota: the same
    kernels on the same pixels, so bit for bit, the angle too -- which holds only if the library's pyramid is the statement's"""
    img, nf, nl, sf, _ = R.case_args(name)
    ref = R.case_ref(name)
    whole = host(ctx, name)
    assert [L.level for L in ref.levels] == list(range(nl))
    for L in ref.levels:
        one = ctx.orb(ref.images[L.level], L.quota, 1, sf)
        sel = whole[1][:, 3] == L.level
        assert sel.sum() == len(one[0]) == L.n_kept
        assert np.array_equal(one[0] * L.scale, whole[0][sel]) and np.array_equal(one[1][:, 1:3], whole[1][sel][:, 1:3])
        assert np.array_equal(one[2], whole[2][sel])
        one_ref, = R.orb(ref.images[L.level], L.quota, 1, sf).levels
        checked(one, R.Ref([one_ref], [ref.images[L.level]], 1), "%s level %d alone" % (name, L.level))


def test_a_permuted_pattern_moves_bits_not_keypoints(ctx):
    img, nf, nl, sf, _ = R.case_args("rect_150_3")
    perm = np.random.Generator(np.random.PCG64(9)).permutation(256)
    a = host(ctx, "rect_150_3")
    b = ctx.orb(img, nf, nl, sf, pattern=R.default_pattern()[perm])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    bits = lambda d: np.unpackbits(d, axis=1, bitorder="little")
    assert np.array_equal(bits(a[2])[:, perm], bits(b[2])) and not np.array_equal(a[2], b[2])
    checked(b, R.orb(img, nf, nl, sf, pattern=R.default_pattern()[perm]), "permuted pattern")
    assert all(np.array_equal(x, y) for x, y in zip(host(ctx, "rect_150_3"), a))          # and the built-in pattern is back


def test_pattern_on_the_square(ctx):
    """points at (+-15, +-15) and at radius 30: against the statement (descriptor rule) and against the C restatement, bit for bit"""
    img, nf, nl, sf, kw = R.case_args("rect_square")
    got = ctx.orb(img, nf, nl, sf, pattern=kw["pattern"])
    s = checked(got, R.case_ref("rect_square"), "square pattern")
    _equal(got, O.orb(img, nf, nl, sf, pattern=kw["pattern"]))
    plain = host(ctx, "rect_150_3")
    differ = np.unpackbits(got[2] ^ plain[2], axis=1, bitorder="little").any(axis=0)
    assert np.array_equal(got[0], plain[0]) and differ[:8].all() and differ[255] and not differ[8:255].any()
    out, d_img = DeviceOut(1, nf), to_device(img)                                           # and through the device form
    n = ctx.orb_device(d_img.data_ptr(), *img.shape, img.shape[1], nf, nl, sf, *out.ptrs(), nf, pattern=kw["pattern"])
    assert n == s["n"] and all(np.array_equal(x, y) for x, y in zip(out.frame(0, n)[0], got))


# ------------------------------------------------------------------------------------------ a pattern outside its domain
def untouched(out):
    return all((t.cpu().numpy() == SENTINEL).all() for t in out.t)


@pytest.mark.parametrize("bad", sorted(R.bad_patterns()))
def test_refused_pattern_orb_forms(bad):
    """host, masked, device, batch and masked batch: TODHIP_EINVAL, nothing written, the cached built-in pattern and the captured
    sequence as they were, and a good pattern right afterwards"""
    ctx = capi.Context(0)
    pat = R.bad_patterns()[bad]
    img, nf, nl, sf, kw = R.case_args("rect_masked")
    mask, H, W = kw["mask"], *img.shape
    before = ctx.orb(img, nf, nl, sf)                                                       # the built-in pattern is uploaded and cached
    assert status_of(lambda: ctx.orb(img, nf, nl, sf, pattern=pat)) == capi.EINVAL
    assert status_of(lambda: ctx.orb(img, nf, nl, sf, pattern=pat, mask=mask)) == capi.EINVAL
    # the host form's outputs, through the C interface itself
    kp, aux, desc = (np.full((nf, w), SENTINEL, np.uint8) for w in (8, 16, 32))
    n_out = C.c_uint32(nf)
    p = lambda a: C.c_void_p(a.ctypes.data)
    g, bp = np.ascontiguousarray(img), np.ascontiguousarray(pat)
    rc = capi.lib().todhip_orb(ctx._h, p(g), H, W, W, nf, nl, sf, p(bp), p(kp), p(aux), p(desc), C.byref(n_out))
    assert rc == capi.EINVAL and n_out.value == 0 and all((a == SENTINEL).all() for a in (kp, aux, desc))
    d_img, d_mask = to_device(np.stack([img, img])), to_device(np.stack([mask, mask]))
    out = DeviceOut(2, nf)
    assert status_of(lambda: ctx.orb_device(d_img.data_ptr(), H, W, W, nf, nl, sf, *out.ptrs(), nf, pattern=pat)) == capi.EINVAL
    assert status_of(lambda: ctx.orb_batch_device(d_img.data_ptr(), 2, H * W, H, W, W, nf, nl, sf, *out.ptrs(), nf, pattern=pat)) == capi.EINVAL
    assert status_of(lambda: ctx.orb_batch_device_masked(d_img.data_ptr(), d_mask.data_ptr(), 2, H * W, H, W, W, nf, nl, sf, *out.ptrs(), nf,
                                                         pattern=pat)) == capi.EINVAL
    # also where no level can hold a keypoint and nothing would be launched anyway
    assert status_of(lambda: ctx.orb(np.full((40, 40), 9, np.uint8), nf, 1, sf, pattern=pat)) == capi.EINVAL
    assert untouched(out)
    after = ctx.orb(img, nf, nl, sf)                                                        # pattern == NULL: the cached one is used
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    R.compare(after, R.case_ref("rect_150_3"))
    sq = R.square_pattern()
    R.compare(ctx.orb(img, nf, nl, sf, pattern=sq), R.case_ref("rect_square"))
    n = ctx.orb_batch_device_masked(d_img.data_ptr(), d_mask.data_ptr(), 2, H * W, H, W, W, nf, nl, sf, *out.ptrs(), nf, pattern=sq)
    assert n == [nf, nf]
    ref_sq_masked = R.orb(img, nf, nl, sf, pattern=sq, mask=mask)
    for f in (0, 1):
        R.compare(out.frame(f, nf)[0], ref_sq_masked)
    ctx.close()


CAM_K = np.array([[220.0, 0, 100.0], [0, 220.0, 80.0], [0, 0, 1]], np.float32)
DEPTH_Z = 0.8


def training_view():
    img = R.image("rect")
    mask = np.zeros(img.shape, np.uint8)
    mask[10:150, 10:190] = 255
    return img, mask, np.full(img.shape, DEPTH_Z, np.float32)


def test_refused_pattern_training(ctx):
    """todhip_model_add_observation and todhip_model_add_observations_device: refused, the model's rows as they were, and the model
    after a good call equal to a model that never saw the bad one"""
    img, mask, depth = training_view()
    Rm, T = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    args = dict(n_features=150, n_levels=3, scale_factor=1.2)
    sq = R.square_pattern()
    clean = capi.Model(ctx, 1000)
    assert clean.add_observation(img, mask, depth, CAM_K, Rm, T, pattern=sq, **args) > 50
    want = clean.finish()
    clean.close()
    d_img, d_mask, d_depth = to_device(img), to_device(mask), __import__("torch").from_numpy(depth).cuda()
    device_call = lambda m, pat: m.add_observations_device(d_img.data_ptr(), d_mask.data_ptr(), d_depth.data_ptr(), 1, *img.shape, CAM_K,
                                                           Rm[None], T[None], pattern=pat, **args)
    for form in ("host", "device"):
        m = capi.Model(ctx, 1000)
        call = (lambda pat: m.add_observation(img, mask, depth, CAM_K, Rm, T, pattern=pat, **args)) if form == "host" else \
               (lambda pat: device_call(m, pat))
        for name, bad in sorted(R.bad_patterns().items()):
            assert status_of(lambda: call(bad)) == capi.EINVAL, (form, name)
            assert m.device()[2] == 0
        assert int(np.sum(call(sq))) == len(want[0])
        got = m.finish()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), form
        m.close()


def test_refused_pattern_pipeline(ctx):
    """todhip_pipeline_set_pattern refuses at the call and the pattern in use stays. It is seen through the poses: the DB holds the
    frame's own descriptors under the reversed built-in pattern (points back-projected from a constant depth), so the frame's object
    is found exactly while the pipeline describes with that pattern."""
    img, _, depth = training_view()
    H, W = img.shape
    rev = np.ascontiguousarray(R.default_pattern()[::-1])
    kp, aux, desc = ctx.orb(img, 150, 1, 1.2, pattern=rev)
    pts = np.stack([(kp[:, 0] - CAM_K[0, 2]) * DEPTH_Z / CAM_K[0, 0], (kp[:, 1] - CAM_K[1, 2]) * DEPTH_Z / CAM_K[1, 1],
                    np.full(len(kp), DEPTH_Z)], axis=1).astype(np.float32)
    pipe = capi.Pipeline(0, frames_per_step=1, H=H, W=W, K=CAM_K, n_features=150, n_levels=1, scale_factor=1.2, k=2, radius=8,
                         verify=(8, 500, 0.01), ring_depth=3)
    try:
        assert pipe.db_load(desc, pts, np.array([0, len(desc)], np.uint32)) == capi.OK

        def poses():
            rc, t = pipe.submit(img[None], depth[None])
            assert rc == capi.OK
            rc, res = pipe.wait(t, 60000)
            assert rc == capi.OK and res[0]["n_kp"] == len(kp) and np.array_equal(res[0]["kp_xy"], kp)
            return res[0]["poses"]

        assert poses() == []                                                                # the built-in pattern: other descriptors
        assert pipe.set_pattern(rev) == capi.OK
        found = poses()
        assert len(found) == 1 and len(found[0]["inliers"]) > 50
        for name, bad in sorted(R.bad_patterns().items()):
            assert pipe.set_pattern(bad) == capi.EINVAL, name
        again = poses()                                                                     # still the reversed pattern
        assert len(again) == 1 and np.array_equal(again[0]["inliers"], found[0]["inliers"]) and np.array_equal(again[0]["R"], found[0]["R"])
        assert pipe.set_pattern(R.square_pattern()) == capi.OK and pipe.set_pattern(None) == capi.OK
        assert poses() == []
    finally:
        pipe.close()
