"""n2m_batch_rays with an intrinsics table (csrc/capture.hip) and the per-view paths of n2m_capture_view / the keypoint batch against their torch statements
in nerf2mesh_amd/capture.py (taken on the CPU), and -- with a table of EQUAL rows -- against the shared-intrinsics kernels: bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from nerf2mesh_amd import synthetic
from nerf2mesh_amd.capture import Capture, SparseDepth, batch_from_uniforms_u8, batch_sparse_u8

pytestmark = pytest.mark.gpu

V, H, W, N = 3, 5, 7, 1000
ROWS = np.array([[9.5, 7.25, 3.3, 2.85], [8.7, 8.1, 3.9, 2.2], [10.2, 6.9, 3.05, 2.65]])       # all different, some no fp32 numbers
NAMES = ("rays_o", "rays_d", "rgba", "nears", "fars", "noises", "bg", "gt_depth")


def _captures(channels, linear, cnf, rows=ROWS, per_view=None):
    g = torch.Generator().manual_seed(channels + 2 * linear)
    images = torch.randint(0, 256, (V, H, W, channels), generator=g, dtype=torch.uint8)
    images[0, 0, 0] = 255
    images[0, 0, 1] = 0
    depth = torch.rand(V, H * W, generator=g) * 3 + 0.5
    poses = synthetic.make_cameras(V, seed=1)
    near_far = synthetic.cam_near_far(poses, "lego", H, W, float(ROWS[0, 0])) if cnf else None
    mk = lambda dev: Capture.from_arrays(poses, images, rows, linear=linear, cam_near_far=near_far, device=dev, per_view=per_view)
    cpu, gpu = mk("cpu"), mk("cuda")
    # the decode table is an INPUT of the kernels, built by torch on the set's own device: the statement gathers from the kernel's table
    assert (cpu.lut - gpu.lut.cpu()).abs().max() < 1e-6
    cpu.lut = gpu.lut.cpu()
    cpu.dense_depth, gpu.dense_depth = depth, depth.cuda()
    return cpu, gpu


def _uniforms():
    u = torch.rand(N, 6, generator=torch.Generator().manual_seed(9))
    below_one = torch.nextafter(torch.tensor(1.0), torch.tensor(0.0))
    u[0, :2] = 0.0
    u[1, :2] = below_one
    u[2, 0], u[2, 1] = 0.0, below_one
    u[3, 0], u[3, 1] = below_one, 0.0
    return u


def _outputs(n_out, cnf):
    f = lambda *s: torch.full(s, -7.0, dtype=torch.float32, device="cuda")
    out = [f(N, 3), f(N, 3), f(N, 4), f(N), f(N), f(N), f(N, 3), f(N)][:n_out]
    counter = None
    if cnf:
        out[6] = None                                            # bg NULL
        counter = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    return out, counter


def _compare(got, want, cnf):
    assert len(got) == len(want)
    for a, b, name in zip(got, want, NAMES):
        if a is None:
            assert name == "bg" and cnf
            continue
        assert torch.equal(a.cpu(), b.cpu() if b is not None else b), name


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("linear", [False, True])
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("ancillary", ["cnf_nobg_counter", "nocnf_bg"])
def test_batch_rays_u8_pv_equals_the_torch_statement(linear, channels, ancillary, dense):
    """All seven outputs (eight with a depth bank) for N = 1000 rays over three views whose rows all differ: more than one block, N no
    multiple of the block, the first and last view and pixel among the uniforms."""
    cnf = ancillary == "cnf_nobg_counter"
    cpu, gpu = _captures(channels, linear, cnf)
    assert gpu.per_view_intrinsics and gpu.intrinsics.is_cuda and gpu.intrinsics.data_ptr() % 16 == 0
    u = _uniforms()
    aabb = torch.tensor([-1.0, -1, -1, 1, 1, 1])
    dd = (lambda c: c.dense_depth) if dense else (lambda c: None)
    want = batch_from_uniforms_u8(cpu.poses, cpu.bank, cpu.lut, u, aabb, 0.05, H, W, cpu.intrinsics, cam_near_far=cpu.cam_near_far, dense_depth=dd(cpu))
    out, counter = _outputs(8 if dense else 7, cnf)
    got = batch_from_uniforms_u8(gpu.poses, gpu.bank, gpu.lut, u.cuda(), aabb.cuda(), 0.05, H, W, gpu.intrinsics, out=tuple(out), counter=counter,
                                 cam_near_far=gpu.cam_near_far, dense_depth=dd(gpu))
    torch.cuda.synchronize()
    _compare(got, want, cnf)
    if cnf:
        assert int(counter) == 0
    else:
        assert torch.equal(got[6].cpu(), u[:, 3:6])
    if channels == 3:
        assert (got[2][:, 3] == 1).all()
    # the rows are per view: the shared kernel at row 0 agrees on view 0's rays only
    shared = batch_from_uniforms_u8(gpu.poses, gpu.bank, gpu.lut, u.cuda(), aabb.cuda(), 0.05, H, W, gpu.intrinsics_of(0), cam_near_far=gpu.cam_near_far)
    cam = (u[:, 0] * V).long().clamp(max=V - 1)
    assert torch.equal(shared[1].cpu()[cam == 0], got[1].cpu()[cam == 0]) and not torch.equal(shared[1].cpu()[cam == 1], got[1].cpu()[cam == 1])
    # without `out` the call allocates its own
    fresh = batch_from_uniforms_u8(gpu.poses, gpu.bank, gpu.lut, u.cuda(), aabb.cuda(), 0.05, H, W, gpu.intrinsics, cam_near_far=gpu.cam_near_far,
                                   dense_depth=dd(gpu))
    assert len(fresh) == len(want) and all(torch.equal(a.cpu(), b) for a, b in zip(fresh, want))


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("ancillary", ["cnf_nobg_counter", "nocnf_bg"])
def test_equal_rows_give_the_bits_of_the_shared_kernels(ancillary, dense):
    """per_view=True with equal rows: n2m_batch_rays with the table against the same entry point with the four scalars, with and without
    the depth bank, on the same set."""
    cnf = ancillary == "cnf_nobg_counter"
    same = np.tile(ROWS[1], (V, 1))
    _, table = _captures(4, False, cnf, rows=same, per_view=True)
    _, shared = _captures(4, False, cnf, rows=same)
    assert table.per_view_intrinsics and not shared.per_view_intrinsics and torch.equal(table.bank, shared.bank)
    u, aabb = _uniforms().cuda(), torch.tensor([-1.0, -1, -1, 1, 1, 1]).cuda()
    runs = []
    for cap in (table, shared):
        out, counter = _outputs(8 if dense else 7, cnf)
        runs.append(batch_from_uniforms_u8(cap.poses, cap.bank, cap.lut, u, aabb, 0.05, H, W, cap.intrinsics, out=tuple(out), counter=counter,
                                           cam_near_far=cap.cam_near_far, dense_depth=cap.dense_depth if dense else None))
        torch.cuda.synchronize()
        assert counter is None or int(counter) == 0
    _compare(runs[0], runs[1], cnf)


def test_one_of_the_two_depth_pointers_missing_is_enull():
    from nerf2mesh_amd import _lib as L
    _, gpu = _captures(4, False, False)
    u, aabb = _uniforms().cuda(), torch.tensor([-1.0, -1, -1, 1, 1, 1]).cuda()
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device="cuda")
    o, d, rgba, a, b, c, gtd = f(N, 3), f(N, 3), f(N, 4), f(N), f(N), f(N), f(N)
    p = L.ptr

    def desc(depth_bank, gt, intrinsics=p(gpu.intrinsics)):
        return ctypes.byref(L.BatchRays(
            poses=p(gpu.poses), uniforms=p(u), V=V, N=N, H=H, W=W, intrinsics=intrinsics, bank=p(gpu.bank), lut=p(gpu.lut), depth_bank=depth_bank,
            aabb=p(aabb), min_near=0.05, rays_o=p(o), rays_d=p(d), rgba=p(rgba), nears=p(a), fars=p(b), noises=p(c), gt_depth=gt))
    for bank, gt, missing in ((p(gpu.dense_depth), None, "gt_depth"), (None, p(gtd), "depth_bank")):
        assert L.lib().n2m_batch_rays(desc(bank, gt), L.stream()) == -2               # N2M_ENULL
        with pytest.raises(RuntimeError, match=rf"n2m_batch_rays failed \(-2\).*{missing} is NULL"):
            L.call("n2m_batch_rays", desc(bank, gt), L.stream())
    L.call("n2m_batch_rays", desc(None, None), L.stream())                             # both NULL: the plain batch
    L.call("n2m_batch_rays", desc(p(gpu.dense_depth), p(gtd)), L.stream())
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        L.call("n2m_batch_rays", desc(None, None, p(gpu.intrinsics) + 4), L.stream())
    with pytest.raises(RuntimeError, match="intrinsics is NULL"):                      # ... and no scalars in their place
        L.call("n2m_batch_rays", desc(None, None, None), L.stream())


@pytest.mark.parametrize("ssaa", [0, 2])
@pytest.mark.parametrize("stride", [1, 2])
def test_capture_view_takes_the_row_of_its_view(stride, ssaa):
    cpu, gpu = _captures(4, False, False)
    seen = []
    for v in range(V):
        want = cpu.view(v, stride=stride, dirs_ssaa=ssaa)
        got = gpu.view(v, stride=stride, dirs_ssaa=ssaa)
        torch.cuda.synchronize()
        for a, b, name in zip(got, want, ("rays_o", "rays_d", "rgba", "dirs")):
            if ssaa == 0 and name == "dirs":
                assert a is None and b is None
                continue
            assert torch.equal(a.cpu(), b), (v, name)
        seen.append(got[1].cpu())
    # the same pose at another view's row gives other rays: the row is what is passed
    other = Capture.from_arrays(gpu.poses.cpu(), gpu.bank_bytes().cpu(), ROWS[[1, 2, 0]], device="cuda").view(0, stride=stride)[1].cpu()
    assert not torch.equal(other, seen[0])


def test_sparse_batch_of_two_views_with_different_rows():
    cpu, gpu = _captures(4, False, True)
    g = torch.Generator().manual_seed(2)
    counts = [300, 9, 261]                                       # more than one block for views 0 and 2
    K = sum(counts)
    coords = torch.stack([torch.randint(0, H, (K,), generator=g), torch.randint(0, W, (K,), generator=g)], -1)
    depth, weight = torch.rand(K, generator=g) + 1, torch.rand(K, generator=g)
    off = np.concatenate([[0], np.cumsum(counts)])
    sd_cpu, sd_gpu = SparseDepth(off, coords, depth, weight), SparseDepth(off, coords, depth, weight, device="cuda")
    aabb = torch.tensor([-1.0, -1, -1, 1, 1, 1])
    rays = {}
    for v in (0, 2):
        u = torch.rand(counts[v], 6, generator=g)
        want = batch_sparse_u8(cpu.poses, cpu.bank, cpu.lut, u, v, sd_cpu, aabb, 0.05, H, W, cpu.intrinsics, cam_near_far=cpu.cam_near_far)
        for table in (gpu.intrinsics, gpu.intrinsics_host, gpu.intrinsics_of(v)):
            got = batch_sparse_u8(gpu.poses, gpu.bank, gpu.lut, u.cuda(), v, sd_gpu, aabb.cuda(), 0.05, H, W, table, cam_near_far=gpu.cam_near_far)
            torch.cuda.synchronize()
            assert len(got) == len(want) == 9
            for a, b in zip(got, want):
                assert torch.equal(a.cpu(), b)
        wrong = batch_sparse_u8(cpu.poses, cpu.bank, cpu.lut, u, v, sd_cpu, aabb, 0.05, H, W, cpu.intrinsics_of(1))
        assert not torch.equal(wrong[1], want[1])
