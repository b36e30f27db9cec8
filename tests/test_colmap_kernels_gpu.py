"""n2m_batch_rays in keypoint mode (csrc/capture.hip) against its torch statement (capture.batch_sparse_u8 on CPU tensors): bit for bit.

V = 3 views of 6 x 5 px with K = [1, 7, 70] keypoints (a view with a single ray, two partial workgroups), and one view with 300 keypoints
(a full workgroup of 256 and a partial one).  The statement has no normalisation in it (rays_d is the unnormalised direction, as in
the uniform mode), so the fp64 square root of the trap note on unit directions has nothing to apply to here; division and the
slab test are correctly rounded on both sides."""
import pytest
import torch

from nerf2mesh_amd import synthetic
from nerf2mesh_amd.capture import Capture, SparseDepth, batch_sparse_u8

pytestmark = pytest.mark.gpu

H, W = 5, 6
INTR = (9.5, 7.25, 3.3, 2.85)
NAMES = ("rays_o", "rays_d", "rgba", "nears", "fars", "noises", "bg", "gt_depth", "depth_weight")


def _case(counts, channels, linear, cnf):
    V = len(counts)
    g = torch.Generator().manual_seed(channels + 2 * linear + 4 * V)
    images = torch.randint(0, 256, (V, H, W, channels), generator=g, dtype=torch.uint8)
    poses = synthetic.make_cameras(V, seed=1)
    near_far = synthetic.cam_near_far(poses, "lego", H, W, INTR[0]) if cnf else None
    K = sum(counts)
    coords = torch.stack([torch.randint(0, H, (K,), generator=g), torch.randint(0, W, (K,), generator=g)], -1)
    coords[0] = torch.tensor([0, 0])
    coords[-1] = torch.tensor([H - 1, W - 1])
    depth = torch.rand(K, generator=g) * 3
    depth[::3] = 0.0
    weight = torch.rand(K, generator=g) * 2
    offsets = torch.tensor([0] + counts).cumsum(0)
    mk = lambda dev: Capture.from_arrays(poses, images, INTR, linear=linear, cam_near_far=near_far, device=dev)
    cpu, gpu = mk("cpu"), mk("cuda")
    cpu.lut = gpu.lut.cpu()               # the decode table is an input of the kernel (tests/test_capture_kernels_gpu.py)
    cpu.sparse_depth = SparseDepth(offsets, coords, depth, weight, "cpu")
    gpu.sparse_depth = SparseDepth(offsets, coords, depth, weight, "cuda")
    return cpu, gpu


def _compare(cpu, gpu, v, nobg):
    K = cpu.sparse_depth.counts[v]
    u = torch.rand(K, 6, generator=torch.Generator().manual_seed(100 + v))
    aabb = torch.tensor([-1.0, -1, -1, 1, 1, 1])
    want = batch_sparse_u8(cpu.poses, cpu.bank, cpu.lut, u, v, cpu.sparse_depth, aabb, 0.05, H, W, cpu.intrinsics, cam_near_far=cpu.cam_near_far)
    f = lambda *s: torch.full(s, -7.0, dtype=torch.float32, device="cuda")
    out = [f(K + 3, 3), f(K + 3, 3), f(K + 3, 4), f(K + 3), f(K + 3), f(K + 3), f(K + 3, 3), f(K + 3), f(K + 3)]      # 3 guard rows each
    counter = None
    if nobg:
        out[6] = None                     # bg NULL, and the counter clear
        counter = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    got = batch_sparse_u8(gpu.poses, gpu.bank, gpu.lut, u.cuda(), v, gpu.sparse_depth, aabb.cuda(), 0.05, H, W, gpu.intrinsics, out=tuple(out),
                          counter=counter, cam_near_far=gpu.cam_near_far)
    torch.cuda.synchronize()
    for a, b, name in zip(got, want, NAMES):
        if a is None:
            assert name == "bg" and nobg
            continue
        assert torch.equal(a[:K].cpu(), b), (v, name)
        assert (a[K:] == -7.0).all(), (v, name, "wrote past its K rows")
    if nobg:
        assert int(counter) == 0
    first = cpu.sparse_depth.host_offsets[v]
    assert torch.equal(got[7][:K].cpu(), cpu.sparse_depth.depth[first:first + K])
    assert torch.equal(got[8][:K].cpu(), cpu.sparse_depth.weight[first:first + K])


@pytest.mark.parametrize("linear", [False, True])
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("ancillary", ["cnf_nobg_counter", "nocnf_bg", "cnf_bg", "nocnf_nobg_counter"])
def test_batch_rays_sparse_u8_equals_the_torch_statement(linear, channels, ancillary):
    """cam_near_far with and without, each with a background and no counter (what the engine runs with a random background) and with neither."""
    cnf, nobg = ancillary.startswith("cnf"), "nobg" in ancillary
    cpu, gpu = _case([1, 7, 70], channels, linear, cnf)
    assert (cpu.cam_near_far is not None) == cnf
    for v in range(3):
        _compare(cpu, gpu, v, nobg)


def test_batch_rays_sparse_u8_more_than_one_workgroup():
    cpu, gpu = _case([300], 4, False, True)
    _compare(cpu, gpu, 0, True)


def test_batch_rays_sparse_u8_refuses_a_wrong_view_or_count():
    cpu, gpu = _case([1, 7, 70], 4, False, False)
    aabb = torch.tensor([-1.0, -1, -1, 1, 1, 1]).cuda()
    with pytest.raises(ValueError, match="7 keypoints"):
        batch_sparse_u8(gpu.poses, gpu.bank, gpu.lut, torch.rand(8, 6).cuda(), 1, gpu.sparse_depth, aabb, 0.05, H, W, gpu.intrinsics)
    with pytest.raises(IndexError):
        batch_sparse_u8(gpu.poses, gpu.bank, gpu.lut, torch.rand(8, 6).cuda(), 3, gpu.sparse_depth, aabb, 0.05, H, W, gpu.intrinsics)
