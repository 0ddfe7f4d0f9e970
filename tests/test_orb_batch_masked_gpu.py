"""todhip_orb_batch_device_masked: a batch of frames with a mask each. Frame f must come back as the CPU restatement computes it on
frame f with mask f (oracle_lib.orb(mask=...), the comparisons of test_orb_gpu.py's masked frame), whatever the other frames' masks
are, for one frame and for several, and a masked call must not colour an unmasked one of the same shape that follows it."""
import numpy as np
import pytest

import oracle_lib as O
from tod_amd import capi, synth

pytestmark = pytest.mark.gpu

H, W, NF, LEVELS, SCALE, F = 200, 264, 300, 3, 1.2, 4


class Env:
    def __init__(self):
        import torch
        self.torch = torch
        self.ctx = capi.Context(0)
        self.imgs = np.stack([np.ascontiguousarray(synth.make_image(70 + f)[40:40 + H, 100:100 + W]) for f in range(F)])
        rng = np.random.Generator(np.random.PCG64(4242))
        m = np.zeros((F, H, W), np.uint8)
        m[0] = 255
        m[1, :, :133] = 255                                     # a half plane that ends at an odd column
        blocks = rng.choice(np.array([0, 1, 255], np.uint8), (H // 8, W // 8))
        m[2] = np.kron(blocks, np.ones((8, 8), np.uint8))       # 8 x 8 blocks; 1 counts as set (mask != 0)
        self.masks = m                                          # m[3]: all zero
        self.d_imgs = torch.from_numpy(self.imgs).cuda()
        self.kp = torch.zeros((F, NF, 2), device="cuda")
        self.aux = torch.zeros((F, NF, 4), device="cuda")
        self.desc = torch.zeros((F, NF, 32), dtype=torch.uint8, device="cuda")
        self._ref = {}
        torch.cuda.synchronize()

    def ref(self, f, mi):
        """the restatement on frame f with mask mi (None: no mask), computed once"""
        if (f, mi) not in self._ref:
            self._ref[(f, mi)] = O.orb(self.imgs[f], NF, LEVELS, SCALE, mask=None if mi is None else self.masks[mi])[:3]
        return self._ref[(f, mi)]

    def run(self, mask_of, frames=range(F)):
        """the batch of `frames` with mask mask_of[i] on its i-th frame (mask_of None: the unmasked call through the masked entry)"""
        torch = self.torch
        frames = list(frames)
        d_mask = None if mask_of is None else torch.from_numpy(np.ascontiguousarray(self.masks[list(mask_of)])).cuda()
        self.kp.fill_(-1); self.aux.fill_(-1); self.desc.fill_(0xEE)
        torch.cuda.synchronize()
        n = self.ctx.orb_batch_device_masked(self.d_imgs[frames[0]].data_ptr(), None if d_mask is None else d_mask.data_ptr(), len(frames),
                                             H * W, H, W, W, NF, LEVELS, SCALE, self.kp.data_ptr(), self.aux.data_ptr(),
                                             self.desc.data_ptr(), NF)
        self.ctx.synchronize()
        return n, self.kp.cpu().numpy(), self.aux.cpu().numpy(), self.desc.cpu().numpy()


def check(env, out, i, f, mi):
    n, kp, aux, desc = out
    o_kp, o_aux, o_d = env.ref(f, mi)
    assert n[i] == len(o_kp), (i, f, mi)
    kp, aux, desc = kp[i, :n[i]], aux[i, :n[i]], desc[i, :n[i]]
    assert np.array_equal(kp, o_kp) and np.array_equal(desc, o_d)
    assert np.array_equal(aux[:, [0, 2, 3]], o_aux[:, [0, 2, 3]])          # size, Harris response, octave: bit-exact
    if n[i]:
        da = np.abs(aux[:, 1] - o_aux[:, 1])
        assert np.minimum(da, 360.0 - da).max() < 1e-2                      # the angle goes through atan2f (device libm)
    if mi is not None:
        l0 = aux[:, 3] == 0                                                 # level-0 keypoints sit on the pixel the mask was sampled at
        assert (env.masks[mi][kp[l0, 1].astype(int), kp[l0, 0].astype(int)] != 0).all()


@pytest.fixture(scope="module")
def env():
    e = Env()
    # what makes the comparisons below mean something: the masks change the result, each in its own way
    full = [len(e.ref(f, None)[0]) for f in range(F)]
    assert all(n == NF for n in full)
    assert np.array_equal(e.ref(0, 0)[0], e.ref(0, None)[0])               # all 255: the unmasked frame
    assert 50 < len(e.ref(1, 1)[0]) and not np.array_equal(e.ref(1, 1)[0], e.ref(1, None)[0]) and e.ref(1, 1)[0][:, 0].max() < 133
    assert 50 < len(e.ref(2, 2)[0]) and not np.array_equal(e.ref(2, 2)[0], e.ref(2, None)[0])
    assert len(e.ref(3, 3)[0]) == 0
    yield e
    e.ctx.close()


def test_each_frame_under_its_own_mask(env):
    out = env.run([0, 1, 2, 3])
    for f in range(F):
        check(env, out, f, f, f)
    assert out[0][3] == 0


def test_masks_rotated_by_one_frame(env):
    """frame f with mask (f + 1) % 4: a mask offset by the wrong stride, or by the frame index of another buffer, shows here"""
    rot = [(f + 1) % F for f in range(F)]
    out = env.run(rot)
    for f in range(F):
        check(env, out, f, f, rot[f])


def test_one_frame(env):
    for f, mi in ((1, 2), (2, 1)):
        out = env.run([mi], frames=[f])
        check(env, out, 0, f, mi)


def test_unmasked_call_after_a_masked_one_of_the_same_shape(env):
    """the captured launch sequence is keyed by the mask's workspace copy: the unmasked call must not replay the masked one"""
    masked = env.run([3, 2, 1, 0])
    for f in range(F):
        check(env, masked, f, f, 3 - f)
    plain = env.run(None)
    for f in range(F):
        check(env, plain, f, f, None)
    torch = env.torch
    env.kp.fill_(-1)
    torch.cuda.synchronize()
    old = env.ctx.orb_batch_device(env.d_imgs.data_ptr(), F, H * W, H, W, W, NF, LEVELS, SCALE, env.kp.data_ptr(), env.aux.data_ptr(),
                                   env.desc.data_ptr(), NF)
    env.ctx.synchronize()
    assert old == plain[0] and np.array_equal(env.kp.cpu().numpy(), plain[1])
    again = env.run([3, 2, 1, 0])                                           # and masked again behind the unmasked one
    for f in range(F):
        check(env, again, f, f, 3 - f)
