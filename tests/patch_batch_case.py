"""Shared cases of the patch-batch tests (tests/test_patch_batch_cpu.py, tests/test_patch_batch_gpu.py): image sets, uniforms with the edge
values in each of the three patch draws, and the draw rule restated as a literal loop in numpy fp32 scalars.

Shapes (V = 3 views each):
    13 x 17, P = 2,  B = 5     the smallest patch; N = 20
    13 x 17, P = 12, B = 3     H - P = 1: every patch starts in row 0; N = 432, two blocks of 256, the second partial
    24 x 40, P = 16, B = 3     the SSIM term's patch size; N = 768, a patch spans blocks
"""
import numpy as np
import torch

from nerf2mesh_amd import synthetic
from nerf2mesh_amd.capture import Capture

V = 3
SHAPES = {"13x17_P2": (13, 17, 2, 5), "13x17_P12": (13, 17, 12, 3), "24x40_P16": (24, 40, 16, 3)}       # H, W, P, B
ROWS = np.array([[9.5, 7.25, 3.3, 2.85], [8.7, 8.1, 3.9, 2.2], [10.2, 6.9, 3.05, 2.65]])                 # per-view (fx, fy, cx, cy), all different
NAMES = ("rays_o", "rays_d", "rgba", "nears", "fars", "noises", "bg", "gt_depth")
AABB = torch.tensor([-1.0, -1, -1, 1, 1, 1])
MIN_NEAR = 0.05


def uniforms(P, B, seed=9):
    """[B P^2, 6] uniforms; the three draws of patch 0 are exactly 0, of patch 1 the largest fp32 below 1, of patch 2 the two mixed: the
    view draw 0 with both position draws at the top, and (B >= 4) patch 3 the other way round."""
    u = torch.rand(B * P * P, 6, generator=torch.Generator().manual_seed(seed))
    top = float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))
    edge = [(0.0, 0.0, 0.0), (top, top, top), (0.0, top, top), (top, 0.0, 0.0)]
    for p, (a, b, c) in enumerate(edge[:B]):
        f = p * P * P
        u[f, 0], u[f, 1], u[f + 1, 1] = a, b, c
    return u


def draws_by_loop(u, H, W, P):
    """(view, i0, j0) per patch and (cam, row, col) per ray, from the rule as the issue states it, one numpy fp32 product at a time."""
    u = u.numpy()
    N = u.shape[0]
    per_patch, cam, row, col = [], [], [], []
    for p in range(N // (P * P)):
        f = p * P * P
        v = min(V - 1, int(np.float32(u[f, 0]) * np.float32(V)))
        i0 = min(H - P - 1, int(np.float32(u[f, 1]) * np.float32(H - P)))
        j0 = min(W - P - 1, int(np.float32(u[f + 1, 1]) * np.float32(W - P)))
        per_patch.append((v, i0, j0))
        for k in range(P * P):
            cam.append(v)
            row.append(i0 + k // P)
            col.append(j0 + k % P)
    return per_patch, torch.tensor(cam), torch.tensor(row), torch.tensor(col)


def arrays(H, W, channels=4, seed=0):
    """uint8 images whose pixels are all different (the pixel's own index in two of the bytes), a depth bank, poses, per-view clamp."""
    g = torch.Generator().manual_seed(seed + channels)
    images = torch.randint(0, 256, (V, H, W, channels), generator=g, dtype=torch.uint8)
    ids = torch.arange(V * H * W).view(V, H, W)
    images[..., 0], images[..., 1] = (ids % 256).to(torch.uint8), (ids // 256).to(torch.uint8)
    depth = torch.rand(V, H * W, generator=g) * 3 + 0.5
    poses = synthetic.make_cameras(V, seed=1)
    near_far = synthetic.cam_near_far(poses, "lego", H, W, float(ROWS[0, 0]))
    return images, depth, poses, near_far


def capture(H, W, device, table=True, cnf=True, channels=4, linear=False, lut=None):
    """A Capture over arrays(H, W) on `device`: per-view intrinsics (the table form) or view 0's four scalars; with or without the clamp.
    lut: the decode table to use instead of the device's own (the statement gathers from the table the kernel gathers from)."""
    images, depth, poses, near_far = arrays(H, W, channels)
    cap = Capture.from_arrays(poses, images, ROWS if table else tuple(float(x) for x in ROWS[0]), linear=linear,
                              cam_near_far=near_far if cnf else None, device=device)
    cap.dense_depth = depth.to(device)
    if lut is not None:
        cap.lut = lut.to(device)
    return cap
