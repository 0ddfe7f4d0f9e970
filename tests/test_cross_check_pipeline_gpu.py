"""todhip_pipeline_set_cross_check on the GPU, on the rendered-view scene of tests/test_pipeline_gpu.py: with the option on, every
frame of a step must come back as the single-frame chain todhip_orb_device -> todhip_match_device -> todhip_cross_check_device(frame_nq
= {n_kp}) -> todhip_verify_device_depth computes it on that frame alone -- n_kp, keypoints, poses in order, R and t bit for bit, the
inlier lists -- also for a blank and a masked-down frame submitted into a slot whose spare rows hold a full step's descriptors (a
filter that ignored frame_nq would let those compete). Off again, the steps are those of a pipeline that never set it."""
import numpy as np
import pytest

import test_pipeline_gpu as TP

pytestmark = pytest.mark.gpu

NF, K, B = TP.NF, TP.K, TP.B


class CrossEnv(TP.Env):
    def __init__(self):
        super().__init__()
        self._cc = {}
        self.removed = {}

    def chain_cc(self, batch, f):
        """The single-frame chain with the cross-check between matcher and verifier; self.removed: matches the filter took."""
        key = (batch["key"], f)
        if key in self._cc:
            return self._cc[key]
        capi, c = self.capi, self.ctx
        gray, depth = batch["images"][f], batch["depth"][f]
        self.torch.cuda.synchronize()
        n = c.orb_device(gray.data_ptr(), self.H, self.W, self.W, NF, TP.LEVELS, TP.SCALE, self.kp.data_ptr(), self.aux.data_ptr(),
                         self.desc.data_ptr(), NF)
        poses, removed = [], 0
        if n:
            out = (self.counts.data_ptr(), self.matches.data_ptr(), self.xyz.data_ptr())
            c.match_device(self.desc.data_ptr(), n, K, TP.RADIUS, *out)
            c.synchronize()
            before = int(self.counts[:n].sum())
            c.cross_check_device(self.desc.data_ptr(), n, n, K, *out, frame_nq=[n])
            c.synchronize()
            removed = before - int(self.counts[:n].sum())
            poses = c.verify_device_depth(self.kp.data_ptr(), n, depth.data_ptr(), False, self.H, self.W, self.scenes.K, *out, K, self.spans,
                                          *TP.VERIFY, capi.rng_new(1))
        c.synchronize()
        self.removed[key] = removed
        self._cc[key] = dict(n_kp=n, kp_xy=self.kp[:n].cpu().numpy(), poses=poses)
        return self._cc[key]


@pytest.fixture(scope="module")
def env():
    e = CrossEnv()
    yield e
    e.ctx.close()


def same_step_cc(env, res, batch, n=B):
    assert len(res) == n
    for f in range(n):
        TP.same_frame(res[f], env.chain_cc(batch, f))


def test_pipeline_equals_the_chain_with_the_filter(env):
    capi = env.capi
    p = env.pipeline()
    try:
        assert p.set_cross_check(True) == capi.OK
        full = env.batches[0]
        same_step_cc(env, env.wait(p, env.submit(p, full)), full)             # nothing outstanding: the first slot
        # the filter did something, and poses are still found (equality below is not equality of empty results)
        assert all(env.removed[(full["key"], f)] > 0 for f in range(B))
        assert sum(len(env.chain_cc(full, f)["poses"]) for f in range(B)) > 0
        short = env.short                                                     # the first slot again: frame 1 blank, frame 2 masked down
        res = env.wait(p, env.submit(p, short))
        assert res[1]["n_kp"] == 0 and res[1]["poses"] == [] and 0 < res[2]["n_kp"] < NF
        same_step_cc(env, res, short)
        # several steps in flight over reused slots, a partial step
        t = [env.submit(p, env.batches[i]) for i in (1, 2, 0)]
        for ticket, i in zip(t, (1, 2, 0)):
            same_step_cc(env, env.wait(p, ticket), env.batches[i])
        same_step_cc(env, env.wait(p, env.submit(p, env.batches[2], 3)), env.batches[2], 3)
        # EBUSY with a ticket outstanding, and the setting stays
        ticket = env.submit(p, env.batches[1])
        assert p.set_cross_check(False) == capi.EBUSY
        same_step_cc(env, env.wait(p, ticket), env.batches[1])
        # off: the steps of a pipeline that never set it (the plain chain of tests/test_pipeline_gpu.py)
        assert p.set_cross_check(False) == capi.OK
        TP.same_step(env, env.wait(p, env.submit(p, full)), full)
        TP.same_step(env, env.wait(p, env.submit(p, short)), short)
    finally:
        p.close()
