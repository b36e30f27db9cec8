"""Shared by the tests of dense-depth supervision (tests/test_dense_depth_*.py): reconstructions with depths/NAME.npy written through
Capture.save_colmap(..., depths=...), and the restatements the loader's calibration is compared against."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TINY = os.path.join(HERE, "golden", "colmap_tiny")


def lstsq_scale_bias(x, y, w):
    """Weighted least squares y ~ scale * x + bias as numpy states it: rows scaled by sqrt(w), numpy.linalg.lstsq, float64."""
    x, y, w = (np.asarray(a, dtype=np.float64) for a in (x, y, w))
    r = np.sqrt(w)
    sol = np.linalg.lstsq(np.stack([x, np.ones_like(x)], -1) * r[:, None], y * r, rcond=None)[0]
    return float(sol[0]), float(sol[1])


def fallback_two(x, y, w):
    """nerf/colmap_provider.py:310-314 on float64 samples (ties in w: the later sample first, as a reversed stable sort leaves them)."""
    order = np.argsort(w, kind="stable")[::-1]
    x0, y0, x1, y1 = x[order[0]], y[order[0]], x[order[1]], y[order[1]]
    scale = (y0 - y1) / (x0 - x1)
    return float(scale), float(y0 - x0 * scale)


def fallback_one(x, y, w):
    """nerf/colmap_provider.py:318-320."""
    k = np.argsort(w, kind="stable")[::-1][0]
    return float(y[k] / x[k]), 0.0


def nearest_keypoint_map(coords, depth, H, W, h, w):
    """[h,w] float32: every pixel takes the depth of the keypoint nearest to its centre (keypoints (row, col) of the H x W image, compared
    in normalised image coordinates) -- a depth map that agrees with the view's sparse depths, at any size."""
    rc = (np.asarray(coords, dtype=np.float64) + 0.5) / np.array([H, W], dtype=np.float64)
    jj, ii = np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(w) + 0.5) / w, indexing="ij")
    d2 = (jj[..., None] - rc[:, 0]) ** 2 + (ii[..., None] - rc[:, 1]) ** 2
    return np.asarray(depth, dtype=np.float32)[d2.argmin(-1)]


def tiny(**kw):
    """The committed tiny reconstruction (9 views of 12 x 10, fx != fy, off-centre principal point, differing keypoint counts), all views,
    with its model kept so that it can be written back."""
    from nerf2mesh_amd.capture import Capture
    return Capture.load_colmap(TINY, split="trainval", scale=1.0, keep_model=True, sparse_depth=True, **kw)


def write(cap, root, depths):
    """cap (from tiny()) written to `root` with the given depth maps."""
    cap.save_colmap(root, scale=1.0, depths=depths, **cap.colmap)
    return root


def box_depth_maps(poses, H, W, intrinsics, scene="lego"):
    """Per view [H,W] float32: depth along the camera axis of the first box surface the pixel's ray meets in the synthetic box scene (where it
    meets none: the depth of the world's origin, as a monocular estimate has a value everywhere): ray-box slab test against every box, the nearest entry t, times the length of the ray's component along the axis (the
    rays of capture.rays_from_pixels have -1 along the camera's z, so the depth along the axis IS t)."""
    import torch
    from nerf2mesh_amd import synthetic
    from nerf2mesh_amd.capture import rays_from_pixels
    poses = torch.as_tensor(poses).float().cpu()
    bx = synthetic.boxes("cpu", scene)
    lo, hi = bx[:, 0:3], bx[:, 3:6]
    pix = torch.arange(H * W)
    out = []
    for v in range(poses.shape[0]):
        o, d = rays_from_pixels(poses, torch.full_like(pix, v), pix % W, torch.div(pix, W, rounding_mode="floor"), intrinsics)
        inv = 1.0 / d
        a, b = (lo[None] - o[:, None]) * inv[:, None], (hi[None] - o[:, None]) * inv[:, None]
        tn, tf = torch.minimum(a, b).amax(-1), torch.maximum(a, b).amin(-1)
        hit = (tn <= tf) & (tf > 0)
        t = torch.where(hit, tn.clamp(min=0), torch.full_like(tn, float("inf"))).amin(-1)
        centre = float(poses[v, :3, 3] @ poses[v, :3, 2])          # depth of the world's origin: what a ray that meets no box is given
        out.append(torch.where(torch.isfinite(t), t, torch.full_like(t, centre)).view(H, W).numpy().astype(np.float32))
    return out
