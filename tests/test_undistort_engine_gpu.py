"""A set photographed through a lens, end to end: the box scene of Capture.synthetic at 32 x 32, four views, rendered THROUGH the lens
(k1 = 0.1: the ray of every distorted pixel comes from the float64 host inverse), written with save_colmap(distortion=...) and loaded with
undistort=True on the device.  The loaded bank is the scene seen by the zoomed pinhole camera, stage 0 trains on it, and both stages hand
out the new intrinsics' rays."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import undistort_ref as R   # noqa: E402
from nerf2mesh_amd import capture as C   # noqa: E402
from nerf2mesh_amd import synthetic   # noqa: E402

pytestmark = pytest.mark.gpu

H = W = 32
V = 4
INTR = (40.0, 40.0, 16.0, 16.0)
COEFF = (0.1,)


def _render(poses, xn, yn):
    """uint8 [V,H,W,4]: the box scene along the rays of the normalised image coordinates (xn, yn) [H,W] (y down), quantised as Capture.synthetic does."""
    bx = synthetic.boxes("cpu", "lego")
    i, j = torch.from_numpy(xn * INTR[0] + INTR[2] - 0.5).reshape(-1), torch.from_numpy(yn * INTR[1] + INTR[3] - 0.5).reshape(-1)
    out = []
    for v in range(V):
        o, d = C.rays_from_pixels(poses, torch.full((H * W,), v), i, j, INTR)         # fractional "pixels": the same ray arithmetic
        out.append((synthetic.render_gt(o, d, bx) * 255 + 0.5).to(torch.uint8).view(H, W, 4))
    return torch.stack(out)


@pytest.fixture(scope="module")
def lens_set(tmp_path_factory):
    poses = synthetic.make_cameras(V, seed=0)
    _, family, row = C.lens_row("SIMPLE_RADIAL", R.colmap_params("SIMPLE_RADIAL", INTR, COEFF))
    jj, ii = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    x, y = C.lens_undistort(family, row, (ii - INTR[2]) / INTR[0], (jj - INTR[3]) / INTR[1])
    photos = _render(poses, x, y)
    src = C.Capture.from_arrays(poses, photos, INTR)
    root = str(tmp_path_factory.mktemp("lens32"))
    pts = np.random.default_rng(0).uniform(-0.4, 0.4, (120, 3))
    src.save_colmap(root, pts, distortion=(COEFF, "SIMPLE_RADIAL"))
    s = C.undistort_zoom(H, W, INTR, family, row)
    # the same views through the zoomed pinhole camera, rendered directly
    clean = _render(poses, (ii - INTR[2]) / (s * INTR[0]), (jj - INTR[3]) / (s * INTR[1]))
    cap = C.Capture.load_colmap(root, split="trainval", scale=1.0, undistort=True, device="cuda")
    return dict(cap=cap, photos=photos, clean=clean, s=s, root=root)


def test_loaded_bank_is_the_scene_through_the_zoomed_pinhole(lens_set):
    cap, s = lens_set["cap"], lens_set["s"]
    out = (s * INTR[0], s * INTR[1], INTR[2], INTR[3])
    assert cap.undistort_zoom == s and cap.intrinsics == out and s > 1
    got = cap.bank_bytes().cpu().numpy().astype(np.float64)
    model64, _ = R.undistort_images(lens_set["photos"].numpy(), "SIMPLE_RADIAL", COEFF, INTR, out)
    clean = lens_set["clean"].numpy().astype(np.float64)
    yard, err = np.abs(model64 - clean), np.abs(got - clean)
    print(f"bank against the direct render: max {err.max():.0f} LSB, mean {err.mean():.3f}; float64 resampler: max {yard.max():.0f}, mean {yard.mean():.3f}")
    assert (err <= yard + 1).all()                                        # per value: the resampler's own error (box edges included) + the statement's 1 LSB
    assert np.abs(got - model64).max() <= 1


def test_stage0_trains_on_the_undistorted_set(lens_set):
    from nerf2mesh_amd.engine import Stage0Engine
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    cap = lens_set["cap"]
    torch.manual_seed(0)
    opt = make_options(O=True, bound=1, dt_gamma=0, iters=30000, fused_mlp=True)
    opt.num_rays, opt.num_points = 1024, 1 << 14
    eng = Stage0Engine(NeRFNetwork(opt), opt, None, torch.device("cuda", 0), seed=0, capture=cap)
    eng.mark_untrained()
    scale0 = float(eng.optimizer.scale)
    losses = [float(eng.train_step()) for _ in range(8)]
    torch.cuda.synchronize()
    print("losses:", losses)
    assert np.isfinite(losses).all()
    assert float(eng.optimizer.found_inf) == 0 and float(eng.optimizer.scale) >= scale0          # no step overflowed: the scale never backed off


def test_both_stages_hand_out_the_new_intrinsics_rays(lens_set):
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    from nerf2mesh_amd.trainer import Stage1Trainer
    cap = lens_set["cap"]
    corner = torch.tensor([H * W - 1])
    wo, wd = C.rays_from_pixels(cap.poses.cpu(), torch.tensor([2]), corner % W, corner // W, cap.intrinsics)
    old = C.rays_from_pixels(cap.poses.cpu(), torch.tensor([2]), corner % W, corner // W, INTR)[1]
    o, d, _, _ = cap.view(2)
    assert torch.equal(d[-1:].cpu(), wd) and torch.equal(o[-1:].cpu(), wo) and not torch.equal(wd, old)
    torch.manual_seed(0)
    v, f = synthetic.scene_mesh(2000)
    opt = make_options(O=True, bound=1, dt_gamma=0, stage=1, fused_mlp=True)
    tr = Stage1Trainer(NeRFNetwork(opt), opt, None, v, f, torch.device("cuda", 0), capture=cap)
    o1, d1, _ = tr._view(2)
    assert torch.equal(d1[-1:].cpu(), wd) and torch.equal(o1[-1:].cpu(), wo)
    assert torch.equal(tr.mvps, cap.mvps)
    proj = C.proj_matrix(H, W, *cap.intrinsics)
    assert torch.equal(cap.mvps[2].cpu(), proj @ torch.inverse(cap.poses[2].cpu()))               # the rasteriser's camera is the new one too
