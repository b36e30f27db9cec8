"""GPU: n2m_batch_rays_patch (csrc/capture.hip) against its torch statement taken on the CPU (capture.batch_from_uniforms_u8 /
synthetic.batch_from_uniforms with patch_size=P, held to the draw rule in tests/test_patch_batch_cpu.py): bit for bit on all seven or
eight outputs, over the shapes of tests/patch_batch_case.py and both ground-truth sources, scalar and per-view intrinsics, with and
without a depth bank, with and without the per-view clamp.  Every output carries three guard rows past its N."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import patch_batch_case as K   # noqa: E402

from nerf2mesh_amd import synthetic   # noqa: E402
from nerf2mesh_amd.capture import batch_from_uniforms_u8, batch_views   # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 3


def _outputs(N, n_out, with_bg):
    f = lambda *s: torch.full(s, -7.0, dtype=torch.float32, device="cuda")
    M = N + GUARD
    out = [f(M, 3), f(M, 3), f(M, 4), f(M), f(M), f(M), f(M, 3), f(M)][:n_out]
    if not with_bg:
        out[6] = None
    return out, torch.full((1,), 5, dtype=torch.int32, device="cuda")


def _compare(got, want, N, with_bg):
    assert len(got) == len(want)
    for a, b, name in zip(got, want, K.NAMES):
        if a is None:
            assert name == "bg" and not with_bg
            continue
        assert torch.equal(a[:N].cpu(), b), name
        assert bool((a[N:] == -7.0).all()), (name, "wrote past its N rows")


def _pair(H, W, table, cnf):
    gpu = K.capture(H, W, "cuda", table=table, cnf=cnf)
    return K.capture(H, W, "cpu", table=table, cnf=cnf, lut=gpu.lut.cpu()), gpu      # the statement gathers from the kernel's decode table


@pytest.mark.parametrize("cnf", [False, True], ids=["nocnf_bg", "cnf_nobg"])
@pytest.mark.parametrize("dense", [False, True], ids=["nodepth", "depth"])
@pytest.mark.parametrize("table", [False, True], ids=["scalars", "table"])
@pytest.mark.parametrize("shape", list(K.SHAPES))
def test_bank_source_equals_the_torch_statement(shape, table, dense, cnf):
    H, W, P, B = K.SHAPES[shape]
    N = B * P * P
    cpu, gpu = _pair(H, W, table, cnf)
    u = K.uniforms(P, B)
    dd = (lambda c: c.dense_depth) if dense else (lambda c: None)
    want = batch_from_uniforms_u8(cpu.poses, cpu.bank, cpu.lut, u, K.AABB, K.MIN_NEAR, H, W, cpu.intrinsics, cam_near_far=cpu.cam_near_far,
                                  dense_depth=dd(cpu), patch_size=P)
    out, counter = _outputs(N, 8 if dense else 7, with_bg=not cnf)
    got = batch_from_uniforms_u8(gpu.poses, gpu.bank, gpu.lut, u.cuda(), K.AABB.cuda(), K.MIN_NEAR, H, W, gpu.intrinsics, out=tuple(out),
                                 counter=counter, cam_near_far=gpu.cam_near_far, dense_depth=dd(gpu), patch_size=P)
    torch.cuda.synchronize()
    _compare(got, want, N, with_bg=not cnf)
    assert int(counter) == 0
    _, cam, _, _ = K.draws_by_loop(u, H, W, P)
    assert torch.equal(batch_views(u.cuda(), K.V, patch_size=P).cpu(), cam.to(torch.int32))
    # without `out` the call allocates its own
    fresh = batch_from_uniforms_u8(gpu.poses, gpu.bank, gpu.lut, u.cuda(), K.AABB.cuda(), K.MIN_NEAR, H, W, gpu.intrinsics,
                                   cam_near_far=gpu.cam_near_far, dense_depth=dd(gpu), patch_size=P)
    assert len(fresh) == len(want) and all(torch.equal(a.cpu(), b) for a, b in zip(fresh, want))


@pytest.mark.parametrize("with_bg", [False, True])
@pytest.mark.parametrize("cnf", [False, True])
@pytest.mark.parametrize("shape", list(K.SHAPES))
def test_fp32_source_equals_the_torch_statement(shape, cnf, with_bg):
    H, W, P, B = K.SHAPES[shape]
    N = B * P * P
    _, _, poses, near_far = K.arrays(H, W)
    images = torch.rand(K.V, H * W, 4, generator=torch.Generator().manual_seed(3))
    u = K.uniforms(P, B)
    focal = float(K.ROWS[0, 0])
    want = synthetic.batch_from_uniforms(poses, images, u, K.AABB, K.MIN_NEAR, H, W, focal, cam_near_far=near_far if cnf else None, patch_size=P)
    out, counter = _outputs(N, 7, with_bg)
    got = synthetic.batch_from_uniforms(poses.cuda(), images.cuda(), u.cuda(), K.AABB.cuda(), K.MIN_NEAR, H, W, focal, out=tuple(out), counter=counter,
                                        cam_near_far=near_far.cuda() if cnf else None, patch_size=P)
    torch.cuda.synchronize()
    _compare(got, want, N, with_bg)
    assert int(counter) == 0


def test_pixel_mode_before_and_after_a_patch_call_keeps_its_bits():
    """n2m_batch_rays before and after n2m_batch_rays_patch on the same descriptor contents: both equal the pixel-mode torch statement."""
    H, W, P, B = K.SHAPES["24x40_P16"]
    N = B * P * P
    cpu, gpu = _pair(H, W, True, True)
    u = K.uniforms(P, B)
    want = batch_from_uniforms_u8(cpu.poses, cpu.bank, cpu.lut, u, K.AABB, K.MIN_NEAR, H, W, cpu.intrinsics, cam_near_far=cpu.cam_near_far,
                                  dense_depth=cpu.dense_depth)
    call = lambda P: batch_from_uniforms_u8(gpu.poses, gpu.bank, gpu.lut, u.cuda(), K.AABB.cuda(), K.MIN_NEAR, H, W, gpu.intrinsics,
                                            cam_near_far=gpu.cam_near_far, dense_depth=gpu.dense_depth, patch_size=P)
    before, patches, after = call(1), call(P), call(1)
    torch.cuda.synchronize()
    for a, b, c, name in zip(before, after, want, K.NAMES):
        assert torch.equal(a.cpu(), c) and torch.equal(b.cpu(), c), name
    assert not torch.equal(patches[2], before[2])
    cam = (u[:, 0] * K.V).long().clamp(max=K.V - 1)
    assert torch.equal(batch_views(u.cuda(), K.V).cpu(), cam.to(torch.int32))
