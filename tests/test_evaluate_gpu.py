"""GPU: metrics.evaluate_views and the renderer factories on a synthetic capture of 3 views at 24 x 24.

The SSIM tolerance is the one of tests/test_ssim_gpu.py: 4 x the largest error of the fp32 model against the float64 model over that
file's case set (tests/ssim_ref.py: yardstick()["mean"], 1.02e-04 measured -> 4.1e-04)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ssim_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu

HW, V = 24, 3


@pytest.fixture(scope="module")
def cap():
    from nerf2mesh_amd import synthetic
    from nerf2mesh_amd.capture import Capture
    f = synthetic.LEGO_FOCAL * HW / synthetic.LEGO_HW
    return Capture.synthetic(synthetic.make_cameras(V, seed=1), H=HW, W=HW, intrinsics=(f, f, HW / 2, HW / 2), alpha=True, device="cuda")


@pytest.fixture(scope="module")
def tol():
    return 4.0 * R.yardstick()["mean"]


def _gt(cap, v, bg=1.0):
    rgba = cap.decode(v)
    return rgba[:, :3] * rgba[:, 3:] + bg * (1 - rgba[:, 3:])


def test_ground_truth_renderer_scores_one_and_inf(cap, tol):
    from nerf2mesh_amd import metrics
    assert cap.has_alpha and len(cap) == V
    ev = metrics.evaluate_views(lambda v: {"image": _gt(cap, v)}, cap)
    assert list(ev) == ["psnr", "ssim", "mean_psnr", "mean_ssim", "views"]
    assert ev["views"] == [0, 1, 2] and len(ev["psnr"]) == len(ev["ssim"]) == V
    assert all(p == math.inf for p in ev["psnr"]) and ev["mean_psnr"] == math.inf
    assert all(abs(s - 1.0) <= tol for s in ev["ssim"]) and abs(ev["mean_ssim"] - 1.0) <= tol
    # another background: the ground truth follows it (the scene does not fill the frame, so the two differ)
    black = metrics.evaluate_views(lambda v: {"image": _gt(cap, v, 0.0)}, cap, bg=0.0)
    assert all(p == math.inf for p in black["psnr"])
    mixed = metrics.evaluate_views(lambda v: {"image": _gt(cap, v, 0.0)}, cap)
    assert all(math.isfinite(p) for p in mixed["psnr"])


def test_known_perturbation_gives_numpy_psnr_and_model_ssim(cap, tol):
    import torch
    from nerf2mesh_amd import metrics
    views = [2, 0]
    gen = torch.Generator().manual_seed(11)
    pert = {v: ((torch.rand(HW * HW, 3, generator=gen) - 0.5) * 0.2) for v in views}
    imgs = {v: (_gt(cap, v).cpu() + pert[v]).clamp(0, 1) for v in views}
    ev = metrics.evaluate_views(lambda v: {"image": imgs[v].cuda()}, cap, views=views)
    assert ev["views"] == views                                       # the order asked for
    for k, v in enumerate(views):
        gt = _gt(cap, v).cpu()
        mse = np.mean((imgs[v].numpy().astype(np.float64) - gt.numpy().astype(np.float64)) ** 2)
        want_psnr = -10.0 * np.log10(mse)
        want_ssim = float(R.ssim_model(imgs[v].view(HW, HW, 3), gt.view(HW, HW, 3))[0])
        print(f"view {v}: psnr {ev['psnr'][k]:.6f} (numpy {want_psnr:.6f})  ssim {ev['ssim'][k]:.6f} (float64 model {want_ssim:.6f})")
        assert abs(ev["psnr"][k] - want_psnr) <= 1e-9 * want_psnr      # both are float64 means of the same fp32 pixels
        assert abs(ev["ssim"][k] - want_ssim) <= tol
        assert 0.0 < want_ssim < 0.999 and 10 < want_psnr < 40           # the perturbation is one: neither score is at a trivial value
    assert ev["mean_psnr"] == pytest.approx(np.mean(ev["psnr"]), rel=1e-12) and ev["mean_ssim"] == pytest.approx(np.mean(ev["ssim"]), rel=1e-12)


def test_field_renderer_on_an_untrained_model(cap):
    import torch
    from nerf2mesh_amd import metrics
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    torch.manual_seed(0)
    opt = make_options(O=True, bound=1, dt_gamma=0, fused_mlp=True)
    model = NeRFNetwork(opt).cuda()
    render = metrics.field_renderer(model, cap)
    img = render(1)["image"]
    assert tuple(img.shape) == (HW * HW, 3) and not img.requires_grad
    ev = metrics.evaluate_views(render, cap)
    assert ev["views"] == [0, 1, 2] and len(ev["psnr"]) == len(ev["ssim"]) == V
    assert all(math.isfinite(p) for p in ev["psnr"]) and all(math.isfinite(s) and -1.0 <= s <= 1.0 for s in ev["ssim"])
    assert math.isfinite(ev["mean_psnr"]) and math.isfinite(ev["mean_ssim"])


def test_psnr_is_the_assets():
    from nerf2mesh_amd import asset, metrics
    assert metrics.psnr is asset.psnr
