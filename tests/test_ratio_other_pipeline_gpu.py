"""todhip_set_ratio_test_other through todhip_pipeline_matcher, on the rendered-view scene of tests/test_pipeline_gpu.py: a small
pipeline (2 frames per step) with the setter applied to its matcher context, and no pipeline change. Every frame of a step must come
back as the single-frame chain todhip_orb_device -> todhip_match_device -> todhip_ratio_other_device -> todhip_verify_device_depth
computes it on that frame alone -- n_kp, keypoints, poses in order, R and t bit for bit, the inlier lists -- also for a blank frame in
a slot whose spare rows hold an earlier step's descriptors. Off again, the steps are those of a pipeline that never set it."""
import pytest

import test_pipeline_gpu as TP

pytestmark = pytest.mark.gpu

NF, K, B2, RATIO = TP.NF, TP.K, 2, 0.8


class OtherEnv(TP.Env):
    def __init__(self):
        super().__init__()
        self._ro = {}
        self.dropped = {}

    def chain_ro(self, batch, f):
        """The single-frame chain with the filter between matcher and verifier; self.dropped: queries the filter emptied."""
        key = (batch["key"], f)
        if key in self._ro:
            return self._ro[key]
        capi, c = self.capi, self.ctx
        gray, depth = batch["images"][f], batch["depth"][f]
        self.torch.cuda.synchronize()
        n = c.orb_device(gray.data_ptr(), self.H, self.W, self.W, NF, TP.LEVELS, TP.SCALE, self.kp.data_ptr(), self.aux.data_ptr(),
                         self.desc.data_ptr(), NF)
        poses, dropped = [], 0
        if n:
            out = (self.counts.data_ptr(), self.matches.data_ptr(), self.xyz.data_ptr())
            c.match_device(self.desc.data_ptr(), n, K, TP.RADIUS, *out)
            c.synchronize()
            before = int((self.counts[:n] > 0).sum())
            c.ratio_other_device(self.desc.data_ptr(), n, RATIO, K, out[0], out[1])
            c.synchronize()
            dropped = before - int((self.counts[:n] > 0).sum())
            poses = c.verify_device_depth(self.kp.data_ptr(), n, depth.data_ptr(), False, self.H, self.W, self.scenes.K, *out, K, self.spans,
                                          *TP.VERIFY, capi.rng_new(1))
        c.synchronize()
        self.dropped[key] = dropped
        self._ro[key] = dict(n_kp=n, kp_xy=self.kp[:n].cpu().numpy(), poses=poses)
        return self._ro[key]


@pytest.fixture(scope="module")
def env():
    e = OtherEnv()
    yield e
    e.ctx.close()


def same_step_ro(env, res, batch, n=B2):
    assert len(res) == n
    for f in range(n):
        TP.same_frame(res[f], env.chain_ro(batch, f))


def test_pipeline_equals_the_chain_with_the_filter(env):
    capi = env.capi
    p = env.pipeline(frames_per_step=B2)
    try:
        p.matcher().set_ratio_test_other(RATIO)
        full = env.batches[0]
        same_step_ro(env, env.wait(p, env.submit(p, full, B2)), full)        # nothing outstanding: the first slot
        # the filter did something, and poses are still found (equality below is not equality of empty results)
        assert all(env.dropped[(full["key"], f)] > 0 for f in range(B2))
        assert sum(len(env.chain_ro(full, f)["poses"]) for f in range(B2)) > 0
        short = env.short                                                    # the first slot again: frame 1 blank
        res = env.wait(p, env.submit(p, short, B2))
        assert res[1]["n_kp"] == 0 and res[1]["poses"] == []
        same_step_ro(env, res, short)
        # several steps in flight over reused slots, a partial step
        t = [env.submit(p, env.batches[i], B2) for i in (1, 2, 0)]
        for ticket, i in zip(t, (1, 2, 0)):
            same_step_ro(env, env.wait(p, ticket), env.batches[i])
        same_step_ro(env, env.wait(p, env.submit(p, env.batches[2], 1)), env.batches[2], 1)
        # the setter refuses a float ratio outside [0, 1] and keeps what it had
        assert capi.lib().todhip_set_ratio_test_other(p.matcher()._h, 1.5) == capi.EINVAL
        same_step_ro(env, env.wait(p, env.submit(p, env.batches[1], B2)), env.batches[1])
        # off: the steps of a pipeline that never set it (the plain chain of tests/test_pipeline_gpu.py)
        p.matcher().set_ratio_test_other(0.0)
        TP.same_step(env, env.wait(p, env.submit(p, full, B2)), full, B2)
        TP.same_step(env, env.wait(p, env.submit(p, short, B2)), short, B2)
    finally:
        p.close()
