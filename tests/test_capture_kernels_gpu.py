"""The kernels of csrc/capture.hip against their torch statements in nerf2mesh_amd/capture.py (taken on the CPU): bit for bit."""
import numpy as np
import pytest
import torch

from nerf2mesh_amd import synthetic
from nerf2mesh_amd.capture import Capture, batch_from_uniforms_u8, box_downscale, pack_rgba8

pytestmark = pytest.mark.gpu

V, H, W, N = 3, 5, 7, 1000
INTR = (9.5, 7.25, 3.3, 2.85)          # fx != fy, principal point off-centre by a non-integer amount
NAMES = ("rays_o", "rays_d", "rgba", "nears", "fars", "noises", "bg")


def _captures(channels, linear, cnf):
    g = torch.Generator().manual_seed(channels + 2 * linear)
    images = torch.randint(0, 256, (V, H, W, channels), generator=g, dtype=torch.uint8)
    images[0, 0, 0] = 255
    images[0, 0, 1] = 0
    poses = synthetic.make_cameras(V, seed=1)
    near_far = synthetic.cam_near_far(poses, "lego", H, W, INTR[0]) if cnf else None
    mk = lambda dev: Capture.from_arrays(poses, images, INTR, linear=linear, cam_near_far=near_far, device=dev)
    cpu, gpu = mk("cpu"), mk("cuda")
    # the decode table is an INPUT of the kernels, built by torch on the set's own device (where `x / 255` and `pow` may round differently
    # from the host's): the statement gathers from the same table the kernel gathers from
    assert (cpu.lut - gpu.lut.cpu()).abs().max() < 1e-6
    cpu.lut = gpu.lut.cpu()
    return cpu, gpu


def _uniforms():
    u = torch.rand(N, 6, generator=torch.Generator().manual_seed(9))
    below_one = torch.nextafter(torch.tensor(1.0), torch.tensor(0.0))
    u[0, :2] = 0.0
    u[1, :2] = below_one
    u[2, 0], u[2, 1] = 0.0, below_one
    u[3, 0], u[3, 1] = below_one, 0.0
    return u


@pytest.mark.parametrize("linear", [False, True])
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("ancillary", ["cnf_nobg_counter", "nocnf_bg"])
def test_batch_rays_u8_equals_the_torch_statement(linear, channels, ancillary):
    cnf = ancillary == "cnf_nobg_counter"
    cpu, gpu = _captures(channels, linear, cnf)
    u = _uniforms()
    aabb = torch.tensor([-1.0, -1, -1, 1, 1, 1])
    want = batch_from_uniforms_u8(cpu.poses, cpu.bank, cpu.lut, u, aabb, 0.05, H, W, cpu.intrinsics, cam_near_far=cpu.cam_near_far)
    f = lambda *s: torch.full(s, -7.0, dtype=torch.float32, device="cuda")
    out = [f(N, 3), f(N, 3), f(N, 4), f(N), f(N), f(N), f(N, 3)]
    counter = None
    if cnf:
        out[6] = None                                            # bg NULL
        counter = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    got = batch_from_uniforms_u8(gpu.poses, gpu.bank, gpu.lut, u.cuda(), aabb.cuda(), 0.05, H, W, gpu.intrinsics, out=tuple(out), counter=counter,
                                 cam_near_far=gpu.cam_near_far)
    torch.cuda.synchronize()
    for a, b, name in zip(got, want, NAMES):
        if a is None:
            assert name == "bg" and cnf
            continue
        assert torch.equal(a.cpu(), b), name
    if cnf:
        assert int(counter) == 0
    else:
        assert torch.equal(got[6].cpu(), u[:, 3:6])
    if channels == 3:
        assert (got[2][:, 3] == 1).all()


@pytest.fixture(scope="module")
def fp32_case():
    """The fp32-image batch (synthetic.batch_from_uniforms, the benchmark's path): 300 rays over V = 3 views of 5 x 7 px -- two blocks, the
    second partial.  The first rows of u are set by hand: 0; 1 - 2^-24, the largest uniform (at these sizes its products round to just
    below V and H W: the last view and pixel without the clamps); 1, which only the two index clamps keep inside the bank; and the
    neighbours of k / V on both sides, where the view index steps.  The torch statement is taken once per clamp setting."""
    n = 300
    g = torch.Generator().manual_seed(11)
    u = torch.rand(n, 6, generator=g)
    one = torch.tensor(1.0)
    u[0, :2] = 0.0
    u[1, :2] = 1.0 - 2.0 ** -24
    u[2, :2] = 1.0
    row = 3
    for k in (1, 2):
        edge = torch.tensor(k / V, dtype=torch.float32)
        for x in (torch.nextafter(edge, 0 * one), edge, torch.nextafter(edge, one)):
            u[row, 0], u[row + 1, 1] = x, x
            row += 2
    poses = synthetic.make_cameras(V, seed=1)
    images = torch.rand(V, H * W, 4, generator=g)
    near_far = synthetic.cam_near_far(poses, "lego", H, W, INTR[0])
    aabb = torch.tensor([-1.0, -1, -1, 1, 1, 1])
    want = {cnf: synthetic.batch_from_uniforms(poses, images, u, aabb, 0.05, H, W, INTR[0], cam_near_far=near_far if cnf else None)
            for cnf in (False, True)}
    cam, pix = (u[:, 0] * V).long(), (u[:, 1] * (H * W)).long()
    assert (int(cam[1]), int(pix[1])) == (V - 1, H * W - 1) and (int(cam[2]), int(pix[2])) == (V, H * W)      # row 2 needs both clamps
    assert cam[3:15:2].tolist() == [0, 1, 1, 1, 2, 2] and sorted(set(cam.clamp(max=V - 1).tolist())) == [0, 1, 2]
    assert not torch.equal(want[False][3], want[True][3]) and not torch.equal(want[False][4], want[True][4])      # the per-view clamp acts
    return dict(n=n, u=u, poses=poses, images=images, near_far=near_far, aabb=aabb, want=want)


@pytest.mark.parametrize("with_bg", [False, True])
@pytest.mark.parametrize("cnf", [False, True])
def test_batch_rays_fp32_equals_the_torch_statement(fp32_case, cnf, with_bg):
    c, n = fp32_case, fp32_case["n"]
    f = lambda *s: torch.full(s, -7.0, dtype=torch.float32, device="cuda")
    out = [f(n + 3, 3), f(n + 3, 3), f(n + 3, 4), f(n + 3), f(n + 3), f(n + 3), f(n + 3, 3) if with_bg else None]          # 3 guard rows each
    counter = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    got = synthetic.batch_from_uniforms(c["poses"].cuda(), c["images"].cuda(), c["u"].cuda(), c["aabb"].cuda(), 0.05, H, W, INTR[0], out=tuple(out),
                                        counter=counter, cam_near_far=c["near_far"].cuda() if cnf else None)
    torch.cuda.synchronize()
    for a, b, name in zip(got, c["want"][cnf], NAMES):
        if a is None:
            assert name == "bg" and not with_bg
            continue
        assert torch.equal(a[:n].cpu(), b), name
        assert (a[n:] == -7.0).all(), (name, "wrote past its N rows")
    assert int(counter) == 0


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("linear", [False, True])
def test_capture_view_equals_the_torch_statement(stride, linear):
    cpu, gpu = _captures(4, linear, False)
    for v in range(V):
        want = cpu.view(v, stride=stride, dirs_ssaa=2)
        got = gpu.view(v, stride=stride, dirs_ssaa=2)
        torch.cuda.synchronize()
        h, w = H // stride, W // stride
        if stride == 2:
            assert (h, w) == (2, 3)
        assert got[0].shape == (h * w, 3) and got[2].shape == (h * w, 4) and got[3].shape == (h * 2 * w * 2, 3)
        for a, b, name in zip(got, want, ("rays_o", "rays_d", "rgba", "dirs")):
            assert torch.equal(a.cpu(), b), (v, name)
    assert gpu.view(0, stride=stride)[3] is None
    # the layout of the directions is the one Stage1Trainer._dirs holds: nearest upscale of the rays, normalised
    d = want[1].view(1, h, w, 3).permute(0, 3, 1, 2)
    up = torch.nn.functional.interpolate(d, (2 * h, 2 * w), mode="nearest").permute(0, 2, 3, 1).reshape(-1, 3)
    np.testing.assert_allclose(want[3].numpy(), (up / up.norm(dim=-1, keepdim=True)).numpy(), rtol=1e-6)


@pytest.mark.parametrize("k", [2, 3])
def test_box_downscale_equals_numpy(k):
    rng = np.random.default_rng(k)
    images = rng.integers(0, 256, (2, 7, 10, 4), dtype=np.uint8)
    images[0, :k, :k] = 255
    images[1, :k, k:2 * k, :2] = 255
    bank, _ = pack_rgba8(torch.from_numpy(images))
    h, w = 7 // k, 10 // k
    got = box_downscale(bank.cuda(), 7, 10, k).cpu().view(torch.uint8).view(2, h, w, 4).numpy()
    blocks = images[:, :h * k, :w * k].astype(np.int64).reshape(2, h, k, w, k, 4)
    want = ((blocks.sum((2, 4)) + (k * k) // 2) // (k * k)).astype(np.uint8)
    assert np.array_equal(got, want)
    assert (got[0, 0, 0] == 255).all()
