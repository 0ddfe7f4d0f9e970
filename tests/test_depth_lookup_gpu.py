"""todhip_test_depth_lookup: the depth lookup of the verifier's cluster kernel on a depth image of the sensor's own size, at every
pixel of small H x W grids (tests/depth_cases.py). z must be the pixel todhip_rescale_depth_device writes, bit for bit, and the CPU
restatement's (oracle_lib.train_rescale_depth); a position outside the image is refused as the cluster kernel refuses it."""
import numpy as np
import pytest

import depth_cases as DC
from tod_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def grid(H, W):
    """every pixel of the H x W image as a keypoint position, with a fraction that the truncation must drop"""
    ys, xs = np.mgrid[0:H, 0:W]
    off = ((xs * 7 + ys * 3) % 10).astype(np.float32) / 10.0
    return np.stack([xs + off, ys + 0.9 * off], -1).reshape(-1, 2).astype(np.float32)


@pytest.mark.parametrize("case", DC.CASES, ids=DC.case_id)
def test_lookup_equals_the_rescaled_image(ctx, case):
    import torch
    (dH, dW, H, W), u16, nearest = case
    assert H * W <= 224
    src, want = DC.reference(case)
    d_src = torch.from_numpy((src.view(np.int16) if u16 else src).copy()).cuda()
    d_full = torch.full((H, W), -1.0, device="cuda")
    torch.cuda.synchronize()
    ctx.rescale_depth_device(d_src.data_ptr(), u16, dH, dW, d_full.data_ptr(), H, W, nearest)
    ctx.synchronize()
    full = d_full.cpu().numpy()
    rc, z = ctx.test_depth_lookup(d_src.data_ptr(), u16, dH, dW, nearest, H, W, grid(H, W), fill=-2.0)
    assert rc == capi.OK
    z = z.reshape(H, W)
    assert DC.same_bits(full, want)                              # (the unchanged kernel, through the shared header)
    assert DC.same_bits(z, full) and DC.same_bits(z, want)


def test_positions_outside_the_image_are_refused(ctx):
    """The cluster kernel reports a keypoint whose truncated position is outside the image as an error of the frame (TODHIP_ERANGE
    from the verify calls); the hook reports the same, leaves that entry alone and fills the others."""
    import torch
    case = ((4, 8, 12, 16), False, False)
    src, want = DC.reference(case)
    d_src = torch.from_numpy(src.copy()).cuda()
    torch.cuda.synchronize()
    kp = np.array([[3.0, 2.0], [16.0, 2.0], [3.0, 12.0], [-1.0, 2.0], [3.0, -1.5], [15.9, 11.9], [-0.5, -0.5]], np.float32)
    rc, z = ctx.test_depth_lookup(d_src.data_ptr(), False, 4, 8, False, 12, 16, kp, fill=-2.0)
    assert rc == capi.ERANGE
    assert list(z[1:5]) == [-2.0] * 4
    # (int)-0.5 == 0: truncation toward zero, as the cluster kernel's
    assert DC.same_bits(z[[0, 5, 6]], np.array([want[2, 3], want[11, 15], want[0, 0]], np.float32))
    rc, z = ctx.test_depth_lookup(d_src.data_ptr(), False, 4, 8, False, 12, 16, kp[[0, 5]], fill=-2.0)
    assert rc == capi.OK and DC.same_bits(z, np.array([want[2, 3], want[11, 15]], np.float32))
    rdH, rdW, rH, rW = DC.REFUSED
    with pytest.raises(capi.TodError) as e:
        ctx.test_depth_lookup(d_src.data_ptr(), False, rdH, rdW, False, rH, rW, kp[:1])
    assert e.value.status == capi.EINVAL
