"""CPU: the torch statement of the patch batch (--patch_size; synthetic.patch_pixels, capture.batch_from_uniforms_u8(patch_size=P),
synthetic.batch_from_uniforms(patch_size=P), capture.batch_views(patch_size=P)) -- the statement the kernel n2m_batch_rays_patch is held
to bit for bit in tests/test_patch_batch_gpu.py -- against the draw rule restated as a literal loop and against the pixel-mode helpers
at the same (view, pixel); and the entry point's argument checks, which run on the host before any launch."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import patch_batch_case as K   # noqa: E402

from nerf2mesh_amd import synthetic   # noqa: E402
from nerf2mesh_amd.capture import batch_from_uniforms_u8, batch_views, decode_words, rays_from_pixels   # noqa: E402


@pytest.mark.parametrize("shape", list(K.SHAPES))
def test_patches_are_blocks_of_one_view_inside_the_image(shape):
    H, W, P, B = K.SHAPES[shape]
    u = K.uniforms(P, B)
    per_patch, cam, row, col = K.draws_by_loop(u, H, W, P)
    got = synthetic.patch_pixels(u, K.V, H, W, P)
    for a, b, name in zip(got, (cam, row, col), ("view", "row", "col")):
        assert a.shape == (B * P * P,) and torch.equal(a, b), name
    # the edge draws: 0 -> view 0, row 0, column 0; the largest fp32 below 1 -> the last view and the last start row / column that is
    # ever drawn, H - P - 1 and W - P - 1 (randint's upper end is excluded)
    assert per_patch[0] == (0, 0, 0) and per_patch[1] == (K.V - 1, H - P - 1, W - P - 1) and per_patch[2] == (0, H - P - 1, W - P - 1)
    if B >= 4:
        assert per_patch[3] == (K.V - 1, 0, 0)
    if H - P == 1:
        assert all(i0 == 0 for _, i0, _ in per_patch)
    cam, row, col = (t.view(B, P, P) for t in got)
    for p in range(B):
        v, i0, j0 = per_patch[p]
        assert 0 <= i0 <= H - P - 1 and 0 <= j0 <= W - P - 1
        assert (cam[p] == v).all()
        assert torch.equal(row[p], (i0 + torch.arange(P))[:, None].expand(P, P))          # row-major: ray k is (k // P, k % P)
        assert torch.equal(col[p], (j0 + torch.arange(P))[None, :].expand(P, P))
    assert int(row.max()) < H and int(col.max()) < W and int(row.min()) >= 0 and int(col.min()) >= 0


@pytest.mark.parametrize("table", [False, True], ids=["scalars", "table"])
@pytest.mark.parametrize("shape", list(K.SHAPES))
def test_u8_statement_equals_the_pixel_mode_helpers_at_the_same_pixels(shape, table):
    H, W, P, B = K.SHAPES[shape]
    cap = K.capture(H, W, "cpu", table=table)
    u = K.uniforms(P, B)
    _, cam, row, col = K.draws_by_loop(u, H, W, P)
    pix = row * W + col
    counter = torch.full((1,), 5, dtype=torch.int32)
    got = batch_from_uniforms_u8(cap.poses, cap.bank, cap.lut, u, K.AABB, K.MIN_NEAR, H, W, cap.intrinsics, counter=counter,
                                 cam_near_far=cap.cam_near_far, dense_depth=cap.dense_depth, patch_size=P)
    assert len(got) == 8 and int(counter) == 0
    o, d = rays_from_pixels(cap.poses, cam, col, row, cap.intrinsics[cam].unbind(-1) if table else cap.intrinsics)
    nears, fars = synthetic.near_far_clamped(o, d, K.AABB, K.MIN_NEAR, cap.cam_near_far, cam)
    want = (o, d, decode_words(cap.bank[cam, pix], cap.lut), nears, fars, u[:, 2], u[:, 3:6], cap.dense_depth[cam, pix])
    for a, b, name in zip(got, want, K.NAMES):
        assert torch.equal(a, b), name
    # the images carry their own pixel index: the colours say the same (view, pixel)
    ids = (got[2][:, 0] * 255).round().long() + 256 * (got[2][:, 1] * 255).round().long()
    assert torch.equal(ids, cam * (H * W) + pix)
    # without the clamp and the depth bank: seven outputs, the slab test alone
    plain = batch_from_uniforms_u8(cap.poses, cap.bank, cap.lut, u, K.AABB, K.MIN_NEAR, H, W, cap.intrinsics, patch_size=P)
    n0, f0 = synthetic.near_far_clamped(o, d, K.AABB, K.MIN_NEAR)
    assert len(plain) == 7 and torch.equal(plain[3], n0) and torch.equal(plain[4], f0) and torch.equal(plain[1], d)
    assert torch.equal(batch_views(u, K.V, patch_size=P), cam.to(torch.int32))
    out = torch.full((B * P * P + 2,), -1, dtype=torch.int32)
    assert torch.equal(batch_views(u, K.V, out=out, patch_size=P), cam.to(torch.int32)) and out[-2:].tolist() == [-1, -1]


@pytest.mark.parametrize("shape", list(K.SHAPES))
def test_fp32_statement_equals_the_pixel_mode_helpers_at_the_same_pixels(shape):
    H, W, P, B = K.SHAPES[shape]
    _, _, poses, near_far = K.arrays(H, W)
    images = torch.rand(K.V, H * W, 4, generator=torch.Generator().manual_seed(3))
    u = K.uniforms(P, B)
    _, cam, row, col = K.draws_by_loop(u, H, W, P)
    pix = row * W + col
    focal = float(K.ROWS[0, 0])
    got = synthetic.batch_from_uniforms(poses, images, u, K.AABB, K.MIN_NEAR, H, W, focal, cam_near_far=near_far, patch_size=P)
    o, d = synthetic.rays_from_pixels(poses, cam, pix, H, W, focal)
    nears, fars = synthetic.near_far_clamped(o, d, K.AABB, K.MIN_NEAR, near_far, cam)
    for a, b, name in zip(got, (o, d, images[cam, pix], nears, fars, u[:, 2], u[:, 3:6]), K.NAMES):
        assert torch.equal(a, b), name


def test_pixel_mode_is_untouched_by_the_parameter():
    """patch_size=1 (the default) is the pixel-mode statement: the same tensors with and without the argument."""
    H, W, P, B = K.SHAPES["13x17_P2"]
    cap = K.capture(H, W, "cpu")
    u = K.uniforms(P, B)
    a = batch_from_uniforms_u8(cap.poses, cap.bank, cap.lut, u, K.AABB, K.MIN_NEAR, H, W, cap.intrinsics)
    b = batch_from_uniforms_u8(cap.poses, cap.bank, cap.lut, u, K.AABB, K.MIN_NEAR, H, W, cap.intrinsics, patch_size=1)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    cam = (u[:, 0] * K.V).long().clamp(max=K.V - 1)
    assert torch.equal(batch_views(u, K.V), cam.to(torch.int32)) and torch.equal(batch_views(u, K.V, patch_size=1), cam.to(torch.int32))
    assert not torch.equal(batch_views(u, K.V, patch_size=P), cam.to(torch.int32))         # a patch has ONE view


def test_python_layer_refuses_bad_patch_sizes():
    H, W = 13, 17
    cap = K.capture(H, W, "cpu")
    call = lambda n, P: batch_from_uniforms_u8(cap.poses, cap.bank, cap.lut, torch.rand(n, 6), K.AABB, K.MIN_NEAR, H, W, cap.intrinsics, patch_size=P)
    for n, P in ((13 * 13, 13), (17 * 17, 17), (0, 0), (14 * 14, 14)):
        with pytest.raises(ValueError, match="patch_size must be"):
            call(n, P)
    with pytest.raises(ValueError, match="multiple of patch_size"):
        call(17, 4)
    with pytest.raises(ValueError, match="multiple of patch_size"):
        batch_views(torch.rand(17, 6), 3, patch_size=4)
    _, _, poses, _ = K.arrays(H, W)
    with pytest.raises(ValueError, match="patch_size must be"):
        synthetic.batch_from_uniforms(poses, torch.rand(K.V, H * W, 4), torch.rand(13 * 13, 6), K.AABB, K.MIN_NEAR, H, W, 9.5, patch_size=13)


def test_entry_point_refuses_before_any_launch():
    """n2m_batch_rays_patch checks P and N on the host (N2M_EINVAL), keypoint batches are N2M_EUNSUPPORTED, and the descriptor's own checks
    are those of n2m_batch_rays; 16 stands in for a device pointer, nothing is dereferenced."""
    from nerf2mesh_amd import _lib as L, build
    build.build(verbose=False)
    base = dict(poses=16, uniforms=16, V=2, N=32, H=9, W=7, fx=1.0, fy=1.0, aabb=16, rays_o=16, rays_d=16, rgba=16, nears=16, fars=16, noises=16,
                bank=16, lut=16)
    batch = lambda **kw: ctypes.byref(L.BatchRays(**{**base, **kw}))
    for P in (0, 1):
        with pytest.raises(RuntimeError, match=r"n2m_batch_rays_patch failed \(-1\).*2 <= P"):
            L.call("n2m_batch_rays_patch", batch(N=P * P), P, None)
    with pytest.raises(RuntimeError, match=r"failed \(-1\).*2 <= P"):
        L.call("n2m_batch_rays_patch", batch(N=49), 7, None)                               # P >= W
    with pytest.raises(RuntimeError, match=r"failed \(-1\).*2 <= P"):
        L.call("n2m_batch_rays_patch", batch(N=81, W=12), 9, None)                         # P >= H
    with pytest.raises(RuntimeError, match=r"failed \(-1\).*not a multiple of P\^2"):
        L.call("n2m_batch_rays_patch", batch(N=33), 4, None)
    with pytest.raises(RuntimeError, match=r"failed \(-3\).*keypoint batches"):
        L.call("n2m_batch_rays_patch", batch(coords=16, kp_depth=16, kp_weight=16, gt_depth=16, depth_weight=16), 4, None)
    with pytest.raises(RuntimeError, match=r"failed \(-2\).*both NULL"):
        L.call("n2m_batch_rays_patch", batch(bank=None, lut=None), 4, None)
    with pytest.raises(RuntimeError, match=r"failed \(-2\).*gt_depth is NULL"):
        L.call("n2m_batch_rays_patch", batch(depth_bank=16), 4, None)
    assert L.lib().n2m_batch_rays_patch(batch(N=0), 4, None) == 0                         # an empty batch: accepted, nothing launched


def test_trainer_draws_whole_patches_and_caps_the_adaptive_ray_count():
    """Stage0Trainer.batch() on the CPU statement: B = max(1, num_rays // P^2) patches, one view per patch for the appearance codes; the
    adaptive ray count of a patch batch never exceeds the sample target, a pixel batch's is left alone."""
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    from nerf2mesh_amd.trainer import Stage0Trainer
    H, W, P, _ = K.SHAPES["24x40_P16"]
    cap = K.capture(H, W, "cpu", table=False, cnf=False)
    cap.dense_depth = None
    for rays, B in ((1000, 3), (100, 1)):
        opt = make_options(bound=1, dt_gamma=0, num_rays=rays, patch_size=P, ind_dim=4, ind_num=8)
        tr = Stage0Trainer(NeRFNetwork(opt), opt, None, torch.device("cpu"), capture=cap)
        o, d, rgba, noises, bg = tr.batch()
        assert o.shape == (B * P * P, 3) and rgba.shape == (B * P * P, 4) and tr._patch == P and tr.num_rays == rays
        idx = tr._index.view(B, P * P)
        assert bool((idx == idx[:, :1]).all())
        assert tr._cap_rays(10 ** 9) == opt.num_points and tr._cap_rays(5) == 5
    opt = make_options(bound=1, dt_gamma=0, num_rays=1000)
    tr = Stage0Trainer(NeRFNetwork(opt), opt, None, torch.device("cpu"), capture=cap)
    assert tr.batch()[0].shape == (1000, 3) and tr._patch == 0 and tr._cap_rays(10 ** 9) == 10 ** 9
    with pytest.raises(ValueError, match="patch_size must be"):
        Stage0Trainer(NeRFNetwork(opt), make_options(bound=1, dt_gamma=0, patch_size=H), None, torch.device("cpu"), capture=cap)
    with pytest.raises(ValueError, match="lambda_patch_ssim > 0 needs patch_size 11 .. 64"):
        Stage0Trainer(NeRFNetwork(opt), make_options(bound=1, dt_gamma=0, patch_size=8, lambda_patch_ssim=0.2), None, torch.device("cpu"), capture=cap)


def test_option_defaults():
    from nerf2mesh_amd.options import make_options
    opt = make_options()
    assert opt.lambda_patch_ssim == 0 and opt.patch_size == 1
    assert make_options(lambda_patch_ssim=0.2, patch_size=16).lambda_patch_ssim == 0.2
