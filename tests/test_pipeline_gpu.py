"""todhip_pipeline on the GPU: every frame of every step must come back as the single-frame device chain computes it on that frame
alone -- todhip_orb_device -> todhip_match_device (its n_kp queries) -> todhip_verify_device_depth with a generator seeded 1 --
whatever the ring slot held before, however the steps are scheduled, in host and device form, gray or colour, float or uint16 depth.
Every wait has a finite timeout: a scheduling bug shows as TODHIP_ETIMEOUT and a failed assertion, not as a hang."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NF, LEVELS, SCALE, K, RADIUS = 500, 3, 1.2, 5, 55
VERIFY = (8, 2500, 0.01)
B, RING = 4, 3
TIMEOUT_MS = 60000


class Env:
    """The shared scene: a DB of 3 objects, 3 batches of 4 rendered frames, a reference context with the DB loaded, and the
    reference chain's result per frame, computed once."""

    def __init__(self):
        import torch
        from tod_amd import capi, scenes
        self.torch, self.capi, self.scenes = torch, capi, scenes
        self.H, self.W = scenes.H, scenes.W
        textures = scenes.make_textures(3)
        self.ctx = capi.Context(0)
        self.db = scenes.train_db(self.ctx, textures, n_features=600)
        self.spans = self.ctx.db_load(*self.db)
        self.batches = scenes.make_detection_batches(textures, 3, B, visible_fraction=1.0)
        self.kp = torch.zeros((NF, 2), device="cuda")
        self.aux = torch.zeros((NF, 4), device="cuda")
        self.desc = torch.zeros((NF, 32), dtype=torch.uint8, device="cuda")
        self.counts = torch.zeros(NF, dtype=torch.int32, device="cuda")
        self.matches = torch.zeros((NF * K, 4), dtype=torch.int32, device="cuda")
        self.xyz = torch.zeros((NF * K, 3), device="cuda")
        self._ref = {}
        # the special frames of the short-step test, with the batch layout (images [4, H, W], depth [4, H, W])
        imgs = self.batches[1]["images"].clone()
        imgs[1] = 128
        imgs[2, :, self.W // 3:] = 128
        # the left third alone still holds more FAST corners than the 500 asked for (about 500 / 440 / 390 on the three levels), so
        # its texture is kept at a fifth of its contrast: the detector's threshold of 20 grey levels then passes only the corners
        # that had more than 100, a few hundred in all
        left = imgs[2, :, :self.W // 3].to(torch.float32)
        imgs[2, :, :self.W // 3] = torch.clamp(torch.round(128.0 + 0.2 * (left - 128.0)), 0, 255).to(torch.uint8)
        self.short = dict(images=imgs.contiguous(), depth=self.batches[1]["depth"], key="short")
        for i, b in enumerate(self.batches):
            b["key"] = "batch%d" % i
        torch.cuda.synchronize()

    def pipeline(self, **kw):
        prm = dict(frames_per_step=B, H=self.H, W=self.W, K=self.scenes.K, n_features=NF, n_levels=LEVELS, scale_factor=SCALE, k=K,
                   radius=RADIUS, verify=VERIFY, ring_depth=RING)
        prm.update(kw)
        load = prm.pop("load_db", True)
        p = self.capi.Pipeline(0, **prm)
        if load:
            assert p.db_load(*self.db) == self.capi.OK
        return p

    def chain(self, gray, depth, u16=False):
        """The single-frame device chain on one frame (tensors on the GPU)."""
        capi, c = self.capi, self.ctx
        self.torch.cuda.synchronize()
        n = c.orb_device(gray.data_ptr(), self.H, self.W, self.W, NF, LEVELS, SCALE, self.kp.data_ptr(), self.aux.data_ptr(),
                         self.desc.data_ptr(), NF)
        poses = []
        if n:
            c.match_device(self.desc.data_ptr(), n, K, RADIUS, self.counts.data_ptr(), self.matches.data_ptr(), self.xyz.data_ptr())
            poses = c.verify_device_depth(self.kp.data_ptr(), n, depth.data_ptr(), u16, self.H, self.W, self.scenes.K, self.counts.data_ptr(),
                                          self.matches.data_ptr(), self.xyz.data_ptr(), K, self.spans, *VERIFY, capi.rng_new(1))
        c.synchronize()
        return dict(n_kp=n, kp_xy=self.kp[:n].cpu().numpy(), poses=poses)

    def ref(self, batch, f):
        key = (batch["key"], f)
        if key not in self._ref:
            self._ref[key] = self.chain(batch["images"][f], batch["depth"][f])
        return self._ref[key]

    def submit(self, p, batch, n=B):
        rc, t = p.submit_device(batch["images"].data_ptr(), batch["depth"].data_ptr(), n)
        assert rc == self.capi.OK
        return t

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


def same_step(env, res, batch, n=B):
    assert len(res) == n
    for f in range(n):
        same_frame(res[f], env.ref(batch, f))


@pytest.fixture(scope="module")
def env():
    e = Env()
    # precondition of every comparison below: the reference chain alone finds the visible object of every textured frame at the
    # pose it was rendered from (bench.py's bounds) -- otherwise "equal to the reference" would be equality of two empty results
    for b in e.batches:
        for f in range(B):
            r = e.ref(b, f)
            hit = [p for p in r["poses"] if p["object"] == b["objects"][f]]
            assert hit, "the reference chain misses object %d in %s frame %d" % (b["objects"][f], b["key"], f)
            Rt, tt = b["poses"][f]
            assert np.abs(hit[0]["R"] - Rt).max() < 0.03 and np.abs(hit[0]["t"] - tt).max() < 0.006
    yield e
    e.ctx.close()


@pytest.fixture(scope="module")
def pipe(env):
    p = env.pipeline()
    yield p
    p.close()


def test_equals_the_single_frame_chain_over_reused_slots(env, pipe):
    """5 steps through 3 ring slots, ring_depth tickets in flight."""
    t = [env.submit(pipe, env.batches[i % 3]) for i in range(3)]
    res = {0: env.wait(pipe, t[0])}
    t.append(env.submit(pipe, env.batches[0]))
    res[1] = env.wait(pipe, t[1])
    t.append(env.submit(pipe, env.batches[1]))
    for i in (2, 3, 4):
        res[i] = env.wait(pipe, t[i])
    assert t == sorted(t) and len(set(t)) == 5
    for i in range(5):
        same_step(env, res[i], env.batches[i % 3])
    st = pipe.stats()
    assert st["steps"] >= 5 and st["frames"] >= 20 and st["keypoints"] >= 20 * NF and st["poses"] >= 20 and st["orb_s"] > 0 and st["verify_s"] > 0


def test_short_and_empty_frames_in_a_used_slot(env, pipe):
    """A step whose frames find fewer keypoints than the capacity, in a slot whose spare rows hold an earlier step's descriptors,
    keypoints and matches: without the zeroed counts those rows produce matches and poses."""
    r_const, r_third = env.ref(env.short, 1), env.ref(env.short, 2)
    assert r_const["n_kp"] == 0 and r_const["poses"] == []
    assert 0 < r_third["n_kp"] < NF
    same_step(env, env.wait(pipe, env.submit(pipe, env.batches[0])), env.batches[0])     # nothing outstanding: the first slot
    res = env.wait(pipe, env.submit(pipe, env.short))                                    # the first slot again
    assert res[1]["n_kp"] == 0 and res[1]["poses"] == []
    same_step(env, res, env.short)
    same_step(env, env.wait(pipe, env.submit(pipe, env.batches[2])), env.batches[2])


def test_partial_steps(env, pipe):
    capi = env.capi
    for n in (1, 3):
        same_step(env, env.wait(pipe, env.submit(pipe, env.batches[2], n)), env.batches[2], n)
    b = env.batches[0]
    for n in (0, B + 1):
        assert pipe.submit_device(b["images"].data_ptr(), b["depth"].data_ptr(), n)[0] == capi.EINVAL
    same_step(env, env.wait(pipe, env.submit(pipe, b)), b)                               # and nothing was taken by the refused ones


def test_host_form_equals_device_form(env, pipe):
    b = env.batches[1]
    rc, t = pipe.submit(b["images"].cpu().numpy(), b["depth"].cpu().numpy())
    assert rc == env.capi.OK
    same_step(env, env.wait(pipe, t), b)
    rc, t = pipe.submit(b["images"][:2].cpu().numpy(), b["depth"][:2].cpu().numpy())    # staging reused, partial
    assert rc == env.capi.OK
    same_step(env, env.wait(pipe, t), b, 2)


@pytest.mark.parametrize("workers", [(1, 1), (1, 2), (2, 2)])
def test_schedule_independence(env, workers):
    p = env.pipeline(orb_workers=workers[0], verify_workers=workers[1])
    order = [env.batches[0], env.short, env.batches[2], env.batches[1]]
    t = [env.submit(p, b) for b in order[:RING]]
    res = [env.wait(p, t[0])]
    t.append(env.submit(p, order[3]))
    res += [env.wait(p, x) for x in t[1:]]
    p.close()
    for r, b in zip(res, order):
        same_step(env, r, b)


def gray_numpy(img):
    """Y = (1868 B + 9617 G + 4899 R + 8192) >> 14 on [..., channels] u8."""
    v = img.astype(np.uint32)
    return ((1868 * v[..., 0] + 9617 * v[..., 1] + 4899 * v[..., 2] + 8192) >> 14).astype(np.uint8)


@pytest.mark.parametrize("H,W,ch,stride", [(1, 1, 3, 3), (5, 67, 3, 208), (7, 64, 4, 256), (3, 130, 4, 520)])
def test_bgr_to_gray_device(env, H, W, ch, stride):
    torch, capi = env.torch, env.capi
    rng = np.random.Generator(np.random.PCG64(H * 1000 + W))
    src = rng.integers(0, 256, (H, stride), dtype=np.uint8)
    d_src = torch.from_numpy(src).cuda()
    d_gray = torch.full((H, W), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    capi.bgr_to_gray_device(env.ctx, d_src.data_ptr(), ch, H, W, stride, d_gray.data_ptr(), W)
    env.ctx.synchronize()
    want = gray_numpy(src[:, :W * ch].reshape(H, W, ch))
    assert np.array_equal(d_gray.cpu().numpy(), want)
    for bad in (dict(ch=2), dict(stride=W * ch - 1), dict(gs=W - 1)):
        rc = capi.lib().todhip_bgr_to_gray_device(env.ctx._h, d_src.data_ptr(), bad.get("ch", ch), H, W, bad.get("stride", stride),
                                                  d_gray.data_ptr(), bad.get("gs", W))
        assert rc == capi.EINVAL


@pytest.mark.parametrize("fmt,ch", [("bgr", 3), ("bgra", 4)])
def test_colour_frames_equal_gray_frames(env, pipe, fmt, ch):
    """A BGR8 / BGRA8 step equals a GRAY8 step fed the numpy-converted frames (and that one the reference chain)."""
    torch, capi = env.torch, env.capi
    rng = np.random.Generator(np.random.PCG64(77 + ch))
    g = env.batches[0]["images"].cpu().numpy()
    col = np.clip(g[..., None].astype(np.int32) + rng.integers(-25, 26, g.shape + (ch,)), 0, 255).astype(np.uint8)
    gray = dict(images=torch.from_numpy(gray_numpy(col)).cuda(), depth=env.batches[0]["depth"], key="gray-of-" + fmt)
    d_col = torch.from_numpy(col).cuda()
    torch.cuda.synchronize()
    want = env.wait(pipe, env.submit(pipe, gray))
    same_step(env, want, gray)
    assert all(len(r["poses"]) >= 1 for r in want)
    p = env.pipeline(frame_format=capi.FRAME_BGR8 if ch == 3 else capi.FRAME_BGRA8)
    rc, t = p.submit_device(d_col.data_ptr(), gray["depth"].data_ptr(), B)
    assert rc == capi.OK
    got = env.wait(p, t)
    rc, t = p.submit(col[:3], gray["depth"][:3].cpu().numpy())                          # host form, partial
    assert rc == capi.OK
    got_host = env.wait(p, t)
    p.close()
    for f in range(B):
        same_frame(got[f], want[f])
    for f in range(3):
        same_frame(got_host[f], want[f])


def test_protocol(env, pipe):
    capi = env.capi
    # tickets waited for in reverse order return their own steps
    order = [env.batches[0], env.short, env.batches[2]]
    t = [env.submit(pipe, b) for b in order]
    b = env.batches[1]
    # the ring is full: the next submit is refused, and accepted after one wait
    assert pipe.submit_device(b["images"].data_ptr(), b["depth"].data_ptr(), B)[0] == capi.EBUSY
    # db_load with tickets outstanding
    assert pipe.db_load(*env.db) == capi.EBUSY
    same_step(env, env.wait(pipe, t[2]), order[2])
    t3 = env.submit(pipe, b)
    same_step(env, env.wait(pipe, t3), b)
    # too little room for the poses: the needed counts, and the ticket is still there
    rc, need = pipe.wait(t[0], TIMEOUT_MS, max_poses=1)
    n_ref = sum(len(env.ref(order[0], f)["poses"]) for f in range(B))
    assert n_ref >= B and rc == capi.ECAPACITY and need[0] == n_ref
    assert need[1] == sum(len(p["inliers"]) for f in range(B) for p in env.ref(order[0], f)["poses"])
    rc, res = pipe.wait(t[0], TIMEOUT_MS, max_poses=need[0], max_inliers=need[1])
    assert rc == capi.OK
    same_step(env, res, order[0])
    same_step(env, env.wait(pipe, t[1]), order[1])
    # each ticket once; unknown tickets
    assert pipe.wait(t[1], TIMEOUT_MS)[0] == capi.EINVAL
    assert pipe.wait(10 ** 9, TIMEOUT_MS)[0] == capi.EINVAL
    assert pipe.db_load(*env.db) == capi.OK                                             # nothing outstanding now
    same_step(env, env.wait(pipe, env.submit(pipe, b)), b)


def test_no_db_and_destroy_with_tickets_outstanding(env):
    capi = env.capi
    p = env.pipeline(load_db=False)
    t = env.submit(p, env.batches[0])
    assert p.wait(t, TIMEOUT_MS)[0] == capi.ENODB
    assert p.db_load(*env.db) == capi.OK                                                # the failed ticket was ended by its wait
    t = [env.submit(p, env.batches[i]) for i in range(3)]
    same_step(env, env.wait(p, t[1]), env.batches[1])
    p.close()                                                                           # two tickets nobody waits for: returns
    assert not p._h


def test_uint16_depth(env):
    torch = env.torch
    h16 = np.full((B, env.H, env.W), 800, np.uint16)
    d16 = torch.from_numpy(h16.view(np.int16)).cuda()                                   # (the same bits)
    b = env.batches[2]
    torch.cuda.synchronize()
    want = [env.chain(b["images"][f], d16[f], u16=True) for f in range(B)]
    assert all(any(p["object"] == b["objects"][f] for p in want[f]["poses"]) for f in range(B))
    p = env.pipeline(depth_is_u16=1)
    rc, t = p.submit_device(b["images"].data_ptr(), d16.data_ptr(), B)
    assert rc == env.capi.OK
    got = env.wait(p, t)
    rc, t = p.submit(b["images"].cpu().numpy(), h16)
    assert rc == env.capi.OK
    got_host = env.wait(p, t)
    p.close()
    for f in range(B):
        same_frame(got[f], want[f])
        same_frame(got_host[f], want[f])
