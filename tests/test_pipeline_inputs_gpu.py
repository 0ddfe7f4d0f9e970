"""The pipeline's two further inputs: a mask per frame (todhip_pipeline_submit_masked[_device]) and depth images of the sensor's own
size (todhip_pipeline_set_depth_size). Every frame of every step must come back as the single-frame device chain computes it on that
frame alone -- masked ORB -> todhip_match_device -> todhip_rescale_depth_device -> todhip_verify_device_depth with a generator
seeded 1 -- in host and device form, for float and uint16 depth, whatever the ring slot carried before. Every wait has a finite
timeout, as in test_pipeline_gpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NF, LEVELS, SCALE, K, RADIUS = 500, 3, 1.2, 5, 55
VERIFY = (8, 2500, 0.01)
B, RING = 4, 3
DH, DW = 240, 320
TIMEOUT_MS = 60000


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
        self.batches = scenes.make_detection_batches(textures, 2, B, visible_fraction=1.0)
        rng = np.random.Generator(np.random.PCG64(97))
        ys, xs = np.mgrid[0:self.H, 0:self.W]
        ripple = (0.0005 * np.sin(xs / 41.0) * np.cos(ys / 29.0)).astype(np.float32)
        # masks that differ per frame: a half plane ending at an odd column, the rows below 101, 16 x 16 blocks of {0, 1, 255}, a hole
        m = np.full((B, self.H, self.W), 255, np.uint8)
        m[0, :, 417:] = 0
        m[1, :101] = 0
        m[2] = np.kron(rng.choice(np.array([0, 1, 255, 255], np.uint8), (self.H // 16, self.W // 16)), np.ones((16, 16), np.uint8))
        m[3, 180:300, 250:390] = 0
        self.masks = m
        self.d_masks = torch.from_numpy(m).cuda()
        for i, b in enumerate(self.batches):
            b["key"] = "batch%d" % i
            D = b["depth"].cpu().numpy() + ripple[None]                     # the plane's constant Z with a half-millimetre ripple and holes
            D[rng.random(D.shape) < 0.01] = np.nan
            half = np.ascontiguousarray(D[:, ::2, ::2]).astype(np.float32)
            b["half"] = half
            b["half16"] = np.where(np.isnan(half), 0, np.round(1000.0 * half)).astype(np.uint16)
            b["d_half"] = torch.from_numpy(half).cuda()
            b["d_half16"] = torch.from_numpy(b["half16"].view(np.int16)).cuda()
        self.kp = torch.zeros((NF, 2), device="cuda")
        self.aux = torch.zeros((NF, 4), device="cuda")
        self.desc = torch.zeros((NF, 32), dtype=torch.uint8, device="cuda")
        self.counts = torch.zeros(NF, dtype=torch.int32, device="cuda")
        self.matches = torch.zeros((NF * K, 4), dtype=torch.int32, device="cuda")
        self.xyz = torch.zeros((NF * K, 3), device="cuda")
        self.full = torch.zeros((self.H, self.W), device="cuda")
        self._ref = {}
        torch.cuda.synchronize()

    def pipeline(self, **kw):
        prm = dict(frames_per_step=B, H=self.H, W=self.W, K=self.scenes.K, n_features=NF, n_levels=LEVELS, scale_factor=SCALE, k=K,
                   radius=RADIUS, verify=VERIFY, ring_depth=RING)
        prm.update(kw)
        p = self.capi.Pipeline(0, **prm)
        assert p.db_load(*self.db) == self.capi.OK
        return p

    def ref(self, batch, f, masked, depth):
        """The single-frame device chain on frame f of the batch, computed once. masked: with mask f; depth: "full" (the rendered
        H x W image, no rescale: the chain the pipeline had before), "half" or "half16" (240 x 320, rescaled)."""
        key = (batch["key"], f, masked, depth)
        if key in self._ref:
            return self._ref[key]
        c, capi = self.ctx, self.capi
        n = c.orb_batch_device_masked(batch["images"][f].data_ptr(), self.d_masks[f].data_ptr() if masked else None, 1, 0, self.H, self.W,
                                      self.W, NF, LEVELS, SCALE, self.kp.data_ptr(), self.aux.data_ptr(), self.desc.data_ptr(), NF)[0]
        poses = []
        if n:
            c.match_device(self.desc.data_ptr(), n, K, RADIUS, self.counts.data_ptr(), self.matches.data_ptr(), self.xyz.data_ptr())
            if depth == "full":
                d_depth = batch["depth"][f]
            else:
                src = batch["d_" + depth][f]
                c.rescale_depth_device(src.data_ptr(), depth == "half16", DH, DW, self.full.data_ptr(), self.H, self.W)
                d_depth = self.full
            poses = c.verify_device_depth(self.kp.data_ptr(), n, d_depth.data_ptr(), False, self.H, self.W, self.scenes.K,
                                          self.counts.data_ptr(), self.matches.data_ptr(), self.xyz.data_ptr(), K, self.spans, *VERIFY,
                                          capi.rng_new(1))
        c.synchronize()
        self._ref[key] = dict(n_kp=n, kp_xy=self.kp[:n].cpu().numpy(), poses=poses)
        return self._ref[key]

    def wait(self, p, t):
        rc, res = p.wait(t, TIMEOUT_MS)
        assert rc == self.capi.OK, "todhip_pipeline_wait: status %d" % rc
        return res


def same_frame(got, ref):
    assert got["n_kp"] == ref["n_kp"]
    assert np.array_equal(got["kp_xy"], ref["kp_xy"])
    assert [p["object"] for p in got["poses"]] == [p["object"] for p in ref["poses"]]
    for a, b in zip(got["poses"], ref["poses"]):
        assert np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"])
        assert np.array_equal(a["inliers"], b["inliers"])


def same_step(env, res, batch, masked, depth, n=B):
    assert len(res) == n
    for f in range(n):
        same_frame(res[f], env.ref(batch, f, masked, depth))


@pytest.fixture(scope="module")
def env():
    e = Env()
    # preconditions, on the reference chain: the masks take keypoints away (each frame differently), and the rendered object is still
    # found through the rescaled depth -- otherwise equality below would be equality of empty results
    b = e.batches[0]
    for f in range(B):
        plain, masked = e.ref(b, f, False, "half"), e.ref(b, f, True, "half")
        assert plain["n_kp"] == NF and not np.array_equal(plain["kp_xy"], masked["kp_xy"])
        kp = masked["kp_xy"]
        assert (e.masks[f][kp[:, 1].astype(int), kp[:, 0].astype(int)] != 0).mean() > 0.9     # (upper levels sample the mask at the nearest pixel)
        for r in (plain, masked, e.ref(b, f, True, "half16")):
            assert any(p["object"] == b["objects"][f] for p in r["poses"]), "the reference chain misses the object in frame %d" % f
    yield e
    e.ctx.close()


@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
def test_masks_and_sensor_sized_depth_in_both_forms(env, u16):
    capi, b = env.capi, env.batches[0]
    depth = "half16" if u16 else "half"
    p = env.pipeline(depth_is_u16=1 if u16 else 0)
    assert p.set_depth_size(DH, DW) == capi.OK
    rc, t_dev = p.submit_masked_device(b["images"].data_ptr(), env.d_masks.data_ptr(), b["d_" + depth].data_ptr(), B)
    assert rc == capi.OK
    rc, t_host = p.submit_masked(b["images"].cpu().numpy(), env.masks, b[depth])
    assert rc == capi.OK
    rc, t_part = p.submit_masked(b["images"][:3].cpu().numpy(), env.masks[:3], b[depth][:3])     # staging reused, partial
    assert rc == capi.OK
    same_step(env, env.wait(p, t_dev), b, True, depth)
    same_step(env, env.wait(p, t_host), b, True, depth)
    same_step(env, env.wait(p, t_part), b, True, depth, 3)
    p.close()


def test_ring_alternating_masked_and_unmasked_then_the_image_size_again(env):
    """Ring of 3 over 4 steps, masked and unmasked in turn (an unmasked step in a slot, and on an ORB context, that carried masks),
    host and device form mixed; then the depth size is taken back and a step equals what the pipeline computed before it had any
    of this."""
    capi = env.capi
    p = env.pipeline()
    assert p.set_depth_size(DH, DW) == capi.OK
    b0, b1 = env.batches

    def submit(b, masked, host):
        if host:
            rc, t = p.submit_masked(b["images"].cpu().numpy(), env.masks if masked else None, b["half"])
        else:
            rc, t = p.submit_masked_device(b["images"].data_ptr(), env.d_masks.data_ptr() if masked else None, b["d_half"].data_ptr(), B)
        assert rc == capi.OK
        return t
    plan = [(b0, True, True), (b1, False, True), (b0, True, False), (b1, False, False)]
    t = [submit(*s) for s in plan[:RING]]
    assert p.submit_masked_device(b0["images"].data_ptr(), None, b0["d_half"].data_ptr(), B)[0] == capi.EBUSY      # the ring is full
    assert p.set_depth_size(0, 0) == capi.EBUSY and p.set_depth_size(DH, DW, True) == capi.EBUSY                # tickets outstanding
    res = [env.wait(p, t[0])]
    t.append(submit(*plan[3]))
    res += [env.wait(p, x) for x in t[1:]]
    for r, (b, masked, _) in zip(res, plan):
        same_step(env, r, b, masked, "half")
    # a geometry the rescale refuses changes nothing: 480 x 320 would need 960 rows
    assert p.set_depth_size(480, 320) == capi.EINVAL and p.set_depth_size(0, 320) == capi.EINVAL
    rc, tt = p.submit_device(b1["images"].data_ptr(), b1["d_half"].data_ptr(), B)
    assert rc == capi.OK
    same_step(env, env.wait(p, tt), b1, False, "half")
    # the image's size again: plain submits, the rendered H x W depth, in a slot whose staging was sized for the smaller images
    assert p.set_depth_size(0, 0) == capi.OK
    rc, t_dev = p.submit_device(b0["images"].data_ptr(), b0["depth"].data_ptr(), B)
    assert rc == capi.OK
    rc, t_host = p.submit(b0["images"].cpu().numpy(), b0["depth"].cpu().numpy())
    assert rc == capi.OK
    rc, t_msk = p.submit_masked(b0["images"].cpu().numpy(), env.masks, b0["depth"].cpu().numpy())
    assert rc == capi.OK
    same_step(env, env.wait(p, t_dev), b0, False, "full")
    same_step(env, env.wait(p, t_host), b0, False, "full")
    same_step(env, env.wait(p, t_msk), b0, True, "full")
    p.close()


def test_nearest_mode_and_equal_size(env):
    """set_depth_size(H, W) is the image's size; the nearest mode reaches the verifier"""
    capi, b = env.capi, env.batches[1]
    p = env.pipeline()
    assert p.set_depth_size(env.H, env.W) == capi.OK
    rc, t = p.submit_device(b["images"].data_ptr(), b["depth"].data_ptr(), 2)
    assert rc == capi.OK
    same_step(env, env.wait(p, t), b, False, "full", 2)
    assert p.set_depth_size(DH, DW, True) == capi.OK
    rc, t = p.submit_device(b["images"].data_ptr(), b["d_half"].data_ptr(), 2)
    assert rc == capi.OK
    got = env.wait(p, t)
    p.close()
    c = env.ctx
    for f in range(2):
        env._ref.pop((b["key"], f, False, "half"), None)                     # computed now: it leaves this frame's keypoints and
        r = env.ref(b, f, False, "half")                                     # matches in the reference buffers
        c.rescale_depth_device(b["d_half"][f].data_ptr(), False, DH, DW, env.full.data_ptr(), env.H, env.W, True)
        want = c.verify_device_depth(env.kp.data_ptr(), r["n_kp"], env.full.data_ptr(), False, env.H, env.W, env.scenes.K,
                                     env.counts.data_ptr(), env.matches.data_ptr(), env.xyz.data_ptr(), K, env.spans, *VERIFY,
                                     env.capi.rng_new(1))
        c.synchronize()
        same_frame(got[f], dict(n_kp=r["n_kp"], kp_xy=r["kp_xy"], poses=want))
