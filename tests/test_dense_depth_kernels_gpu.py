"""n2m_depth_bank_fill and n2m_batch_rays with a depth bank (csrc/capture.hip) against their torch statements (capture.dense_depth_fill and
capture.batch_from_uniforms_u8(dense_depth=...) on CPU tensors) and against the same entry point without the depth bank: bit for bit."""
import ctypes

import pytest
import torch

from nerf2mesh_amd import synthetic
from nerf2mesh_amd import capture as C

pytestmark = pytest.mark.gpu

H, W, V = 10, 12, 5
INTR = (14.0, 13.0, 6.5, 4.25)
NAMES = ("rays_o", "rays_d", "rgba", "nears", "fars", "noises", "bg", "gt_depth")


@pytest.mark.parametrize("affine", [(1.0, 0.0), (0.37, -1.625)])
@pytest.mark.parametrize("h,w,Ho,Wo", [(5, 7, H, W), (20, 24, H, W), (10, 12, H, W), (1, 1, 3, 2)])
def test_depth_bank_fill_equals_the_torch_statement(h, w, Ho, Wo, affine):
    src = torch.rand(h, w, generator=torch.Generator().manual_seed(h * w)) * 6 - 1
    want = C.dense_depth_fill(src, Ho, Wo, *affine)
    out = torch.full((Ho * Wo + 5,), -7.0, device="cuda")                 # 5 guard values behind the row
    got = C.dense_depth_fill(src.cuda(), Ho, Wo, *affine, out=out[:Ho * Wo])
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(out[:Ho * Wo].cpu(), want)
    assert (out[Ho * Wo:] == -7.0).all(), "wrote past its H*W values"
    if (h, w) == (Ho, Wo) and affine == (1.0, 0.0):
        assert torch.equal(out[:Ho * Wo].cpu().view(h, w), src)


def _case(channels, linear, cnf):
    g = torch.Generator().manual_seed(channels + 2 * linear)
    images = torch.randint(0, 256, (V, H, W, channels), generator=g, dtype=torch.uint8)
    poses = synthetic.make_cameras(V, seed=1)
    near_far = synthetic.cam_near_far(poses, "lego", H, W, INTR[0]) if cnf else None
    depth = torch.rand(V, H * W, generator=g) * 4
    mk = lambda dev: C.Capture.from_arrays(poses, images, INTR, linear=linear, cam_near_far=near_far, device=dev)
    cpu, gpu = mk("cpu"), mk("cuda")
    cpu.lut = gpu.lut.cpu()               # the decode table is an input of the kernel (tests/test_capture_kernels_gpu.py)
    cpu.dense_depth, gpu.dense_depth = depth, depth.cuda()
    return cpu, gpu


@pytest.mark.parametrize("N", [70, 257])
@pytest.mark.parametrize("linear", [False, True])
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("ancillary", ["cnf_nobg_counter", "nocnf_bg"])
def test_batch_rays_u8_depth_equals_the_plain_kernel_and_the_statement(N, linear, channels, ancillary):
    cnf, nobg = ancillary.startswith("cnf"), "nobg" in ancillary
    cpu, gpu = _case(channels, linear, cnf)
    u = torch.rand(N, 6, generator=torch.Generator().manual_seed(N))
    u[0, :2] = 0.0
    u[1, :2] = 1.0                                                        # clamped to the last view and the last pixel
    aabb = torch.tensor([-1.0, -1, -1, 1, 1, 1])
    want = C.batch_from_uniforms_u8(cpu.poses, cpu.bank, cpu.lut, u, aabb, 0.05, H, W, INTR, cam_near_far=cpu.cam_near_far, dense_depth=cpu.dense_depth)
    f = lambda *s: torch.full(s, -7.0, dtype=torch.float32, device="cuda")
    mk = lambda k: [f(N + 3, 3), f(N + 3, 3), f(N + 3, 4), f(N + 3), f(N + 3), f(N + 3), f(N + 3, 3), f(N + 3)][:k]      # 3 guard rows each
    out, ref = mk(8), mk(7)
    c1 = c2 = None
    if nobg:
        out[6] = ref[6] = None
        c1, c2 = (torch.full((1,), 5, dtype=torch.int32, device="cuda") for _ in range(2))
    args = (gpu.poses, gpu.bank, gpu.lut, u.cuda(), aabb.cuda(), 0.05, H, W, INTR)
    got = C.batch_from_uniforms_u8(*args, out=tuple(out), counter=c1, cam_near_far=gpu.cam_near_far, dense_depth=gpu.dense_depth)
    plain = C.batch_from_uniforms_u8(*args, out=tuple(ref), counter=c2, cam_near_far=gpu.cam_near_far)
    torch.cuda.synchronize()
    for k, name in enumerate(NAMES):
        if got[k] is None:
            assert name == "bg" and nobg
            continue
        assert torch.equal(got[k][:N].cpu(), want[k]), name
        assert (got[k][N:] == -7.0).all(), (name, "wrote past its N rows")
        if k < 7:
            assert torch.equal(got[k], plain[k]), name                    # the bits of the call without a depth bank, guard rows included
    if nobg:
        assert int(c1) == 0 and int(c2) == 0
    cam = (u[:, 0] * V).long().clamp(max=V - 1)
    pix = (u[:, 1] * (H * W)).long().clamp(max=H * W - 1)
    assert torch.equal(got[7][:N].cpu(), cpu.dense_depth[cam, pix])


def test_batch_rays_u8_depth_refuses_a_null_bank():
    from nerf2mesh_amd import _lib as L
    cpu, gpu = _case(4, False, False)
    N = 8
    u = torch.rand(N, 6).cuda()
    aabb = torch.tensor([-1.0, -1, -1, 1, 1, 1]).cuda()
    f = lambda *s: torch.full(s, -7.0, dtype=torch.float32, device="cuda")
    o, d, rgba, nears, fars, noises, bg, gtd = f(N, 3), f(N, 3), f(N, 4), f(N), f(N), f(N), f(N, 3), f(N)
    p = L.ptr

    def desc(bank, depth_bank, gt):
        return L.BatchRays(poses=p(gpu.poses), uniforms=p(u), V=V, N=N, H=H, W=W, fx=INTR[0], fy=INTR[1], cx=INTR[2], cy=INTR[3], bank=bank,
                           lut=p(gpu.lut), depth_bank=depth_bank, aabb=p(aabb), min_near=0.05, rays_o=p(o), rays_d=p(d), rgba=p(rgba),
                           nears=p(nears), fars=p(fars), noises=p(noises), bg=p(bg), gt_depth=gt)

    def rc(depth_bank, gt, bank=p(gpu.bank)):
        return L.lib().n2m_batch_rays(ctypes.byref(desc(bank, depth_bank, gt)), L.stream())
    assert rc(None, p(gtd)) == rc(p(gpu.dense_depth), p(gtd), bank=None) == -2
    assert rc(p(gpu.dense_depth), None) == -2                             # N2M_ENULL
    torch.cuda.synchronize()
    assert (gtd == -7.0).all() and (o == -7.0).all()                       # nothing was launched
    with pytest.raises(RuntimeError, match="depth_bank is NULL"):
        L.call("n2m_batch_rays", ctypes.byref(desc(p(gpu.bank), None, p(gtd))), L.stream())
    assert rc(p(gpu.dense_depth), p(gtd)) == 0
