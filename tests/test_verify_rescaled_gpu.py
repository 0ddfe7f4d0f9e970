"""todhip_verify[_batch]_device_depth_rescaled on rendered frames (480 x 640, a DB of 3 objects): with the depth image at a size of
its own the result must be the one of todhip_rescale_depth_device into an H x W image followed by todhip_verify_device_depth on it --
objects, R, t, inlier lists and the generator's state, exactly -- in every mode of the rescale, for float and uint16 sources, and the
batch form must equal its singles. The reference route has to find the rendered object in every variant: two empty results would
be "equal" too."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NF, LEVELS, SCALE, K, RADIUS = 500, 3, 1.2, 5, 55
VERIFY = (8, 2500, 0.01)
B = 4


def variants(D):
    """name -> (depth image, nearest) made from a frame's H x W float depth D"""
    half = np.ascontiguousarray(D[::2, ::2])
    mm = np.where(np.isnan(half), 0, np.round(1000.0 * half)).astype(np.uint16)
    return {
        "half-bilinear": (half, False),
        "half-nearest": (half, True),
        "double-shrink": (np.ascontiguousarray(np.repeat(np.repeat(D, 2, 0), 2, 1)), False),
        "upper-three-quarters": (np.ascontiguousarray(D[:360:2, ::2]), False),     # 180 x 320: the image's rows 360.. have no depth
        "half-u16": (mm, False),
        "same-size": (D, False),
    }


NAMES = list(variants(np.zeros((480, 640), np.float32)))


class Env:
    def __init__(self):
        import torch
        from tod_amd import capi, scenes
        self.torch, self.capi, self.scenes = torch, capi, scenes
        self.H, self.W = scenes.H, scenes.W
        textures = scenes.make_textures(3)
        self.ctx = capi.Context(0)
        self.db = scenes.train_db(self.ctx, textures, n_features=600)
        self.spans = self.ctx.db_load(*self.db)
        self.batch = scenes.make_detection_batches(textures, 1, B, visible_fraction=1.0)[0]
        # the rendered depth (the plane's constant Z) with what a sensor adds: a smooth half-millimetre ripple, so that interpolated
        # values differ from their taps and from each other, scattered holes and one block without depth
        rng = np.random.Generator(np.random.PCG64(31))
        ys, xs = np.mgrid[0:self.H, 0:self.W]
        D = self.batch["depth"].cpu().numpy() + (0.0005 * np.sin(xs / 37.0) * np.cos(ys / 23.0)).astype(np.float32)[None]
        D[rng.random(D.shape) < 0.01] = np.nan
        for f in range(B):
            D[f, 40 + 30 * f:80 + 30 * f, 500:560] = np.nan
        self.D = D.astype(np.float32)
        # keypoints and matches of the four frames, in the batch layout
        self.kp = torch.zeros((B, NF, 2), device="cuda")
        self.aux = torch.zeros((NF, 4), device="cuda")
        self.desc = torch.zeros((B, NF, 32), dtype=torch.uint8, device="cuda")
        self.counts = torch.zeros((B, NF), dtype=torch.int32, device="cuda")
        self.matches = torch.zeros((B, NF * K, 4), dtype=torch.int32, device="cuda")
        self.xyz = torch.zeros((B, NF * K, 3), device="cuda")
        self.full = torch.zeros((self.H, self.W), device="cuda")
        torch.cuda.synchronize()
        c = self.ctx
        for f in range(B):
            n = c.orb_device(self.batch["images"][f].data_ptr(), self.H, self.W, self.W, NF, LEVELS, SCALE, self.kp[f].data_ptr(),
                             self.aux.data_ptr(), self.desc[f].data_ptr(), NF)
            assert n == NF
            c.match_device(self.desc[f].data_ptr(), NF, K, RADIUS, self.counts[f].data_ptr(), self.matches[f].data_ptr(), self.xyz[f].data_ptr())
        c.synchronize()
        self._dev, self._ref = {}, {}

    def depth(self, name, f):
        """(device tensor, is_u16, dH, dW, nearest) of frame f's variant"""
        if (name, f) not in self._dev:
            img, nearest = variants(self.D[f])[name]
            u16 = img.dtype == np.uint16
            t = self.torch.from_numpy(img.view(np.int16) if u16 else img).cuda()
            self.torch.cuda.synchronize()
            self._dev[(name, f)] = (t, u16, img.shape[0], img.shape[1], nearest)
        return self._dev[(name, f)]

    def tail(self, f):
        return (self.counts[f].data_ptr(), self.matches[f].data_ptr(), self.xyz[f].data_ptr(), K, self.spans) + VERIFY

    def ref(self, name, f):
        """the reference route: rescale into an H x W image, then the existing call on it; (poses, generator), computed once"""
        if (name, f) not in self._ref:
            t, u16, dH, dW, nearest = self.depth(name, f)
            c, rng = self.ctx, self.capi.rng_new(1)
            c.rescale_depth_device(t.data_ptr(), u16, dH, dW, self.full.data_ptr(), self.H, self.W, nearest)
            poses = c.verify_device_depth(self.kp[f].data_ptr(), NF, self.full.data_ptr(), False, self.H, self.W, self.scenes.K,
                                          *self.tail(f), rng)
            c.synchronize()
            self._ref[(name, f)] = (poses, rng)
        return self._ref[(name, f)]


def same_rng(a, b):
    return list(a.s) == list(b.s) and (a.f, a.b, a.draws) == (b.f, b.b, b.draws)


def same_poses(got, ref):
    assert [p["object"] for p in got] == [p["object"] for p in ref]
    for a, b in zip(got, ref):
        assert np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"]) and np.array_equal(a["inliers"], b["inliers"])


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.ctx.close()


@pytest.mark.parametrize("name", NAMES)
def test_single_frame_equals_rescale_then_verify(env, name):
    for f in range(B):
        ref, ref_rng = env.ref(name, f)
        # precondition, on the reference route: the rendered object is found
        assert any(p["object"] == env.batch["objects"][f] for p in ref), "the reference route misses the object in %s frame %d" % (name, f)
        t, u16, dH, dW, nearest = env.depth(name, f)
        rng = env.capi.rng_new(1)
        got = env.ctx.verify_device_depth_rescaled(env.kp[f].data_ptr(), NF, t.data_ptr(), u16, dH, dW, nearest, env.H, env.W,
                                                   env.scenes.K, *env.tail(f), rng)
        same_poses(got, ref)
        assert same_rng(rng, ref_rng) and rng.draws > 0


def test_the_variants_are_different_inputs(env):
    """the holes and the band take keypoints away: the variants do not all give one result, so equality above is per variant"""
    inl = {name: sum(len(p["inliers"]) for p in env.ref(name, 0)[0]) for name in NAMES}
    assert len(set(inl.values())) > 1, inl
    band = env.ref("upper-three-quarters", 0)[0]
    kp = env.kp[0].cpu().numpy()
    assert (kp[:, 1] >= 360).any() and all((kp[p["inliers"], 1] < 360).all() for p in band)


@pytest.mark.parametrize("name", ["half-bilinear", "upper-three-quarters", "half-u16"])
def test_batch_equals_its_singles(env, name):
    torch = env.torch
    per = [env.depth(name, f) for f in range(B)]
    _, u16, dH, dW, nearest = per[0]
    d_all = torch.stack([p[0] for p in per]).contiguous()
    rngs = (env.capi.Rng * B)(*[env.capi.rng_new(1) for _ in range(B)])
    torch.cuda.synchronize()
    got = env.ctx.verify_batch_device_depth_rescaled(B, env.kp.data_ptr(), NF, d_all.data_ptr(), u16, dH, dW, nearest, env.H, env.W,
                                                     env.scenes.K, env.counts.data_ptr(), env.matches.data_ptr(), env.xyz.data_ptr(), K,
                                                     env.spans, *VERIFY, rngs, max_poses=64)
    for f in range(B):
        ref, ref_rng = env.ref(name, f)
        same_poses(got[f], ref)
        assert same_rng(rngs[f], ref_rng)


def test_refused_geometry_and_bad_arguments(env):
    capi = env.capi
    t, u16, dH, dW, nearest = env.depth("half-bilinear", 0)
    for bad in ((480, 320), (0, 320), (240, 0)):                 # 480 x 320 -> 640 wide needs 960 rows
        rng = capi.rng_new(1)
        with pytest.raises(capi.TodError) as e:
            env.ctx.verify_device_depth_rescaled(env.kp[0].data_ptr(), NF, t.data_ptr(), u16, bad[0], bad[1], nearest, env.H, env.W,
                                                 env.scenes.K, *env.tail(0), rng)
        assert e.value.status == capi.EINVAL and rng.draws == 0
