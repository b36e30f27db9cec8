"""The torch statement of the uint8 batch (capture.batch_from_uniforms_u8, CPU branch) against synthetic.batch_from_uniforms' CPU branch fed
the decoded fp32 bank and the same uniforms: every output bitwise equal."""
import pytest
import torch

from nerf2mesh_amd import synthetic
from nerf2mesh_amd.capture import Capture, batch_from_uniforms_u8


@pytest.mark.parametrize("linear", [False, True])
@pytest.mark.parametrize("cnf", [False, True])
def test_u8_batch_statement_equals_the_fp32_one(linear, cnf):
    Hh = Ww = 16
    focal = synthetic.LEGO_FOCAL * Hh / synthetic.LEGO_HW
    poses = synthetic.make_cameras(3, seed=0)
    g = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (3, Hh, Ww, 4), generator=g, dtype=torch.uint8)
    near_far = synthetic.cam_near_far(poses, "lego", Hh, Ww, focal) if cnf else None
    cap = Capture.from_arrays(poses, images, (focal, focal, Ww / 2, Hh / 2), linear=linear, cam_near_far=near_far)
    u = torch.rand(777, 6, generator=g)
    u[0, :2] = 0.0
    u[1, :2] = torch.nextafter(torch.tensor(1.0), torch.tensor(0.0))
    aabb = torch.tensor([-1.0, -1, -1, 1, 1, 1])
    counter = torch.ones(1, dtype=torch.int32)
    got = batch_from_uniforms_u8(cap.poses, cap.bank, cap.lut, u, aabb, 0.05, Hh, Ww, cap.intrinsics, counter=counter, cam_near_far=near_far)
    want = synthetic.batch_from_uniforms(poses, cap.decode(), u, aabb, 0.05, Hh, Ww, focal, cam_near_far=near_far)
    for a, b, name in zip(got, want, ("rays_o", "rays_d", "rgba", "nears", "fars", "noises", "bg")):
        assert a.shape == b.shape and torch.equal(a, b), name
    assert int(counter) == 0
    x = images.float() / 255
    if linear:
        x[..., :3] = torch.where(x[..., :3] < 0.04045, x[..., :3] / 12.92, ((x[..., :3] + 0.055) / 1.055) ** 2.4)
    assert torch.equal(cap.decode(), x.view(3, -1, 4))
