"""GPU: the opt-in SSIM term of stage 1 (options.lambda_ssim, trainer.Stage1Trainer) on the marching-cubes sphere of tools/eval_export.py
(R = 24) seen by a synthetic capture at 32 x 32, ssaa 1.

One step with lambda_ssim = 0.2 against one step of an identically seeded trainer with lambda_ssim = 0 that is forced onto the torch-graph
head (the branch lambda_ssim selects): the loss gains 0.2 (1 - SSIM) of that trainer's frame, SSIM by the float64 model of tests/ssim_ref.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ssim_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu

LAM, HW, RES = 0.2, 32, 24


def _sphere():
    import torch
    from nerf2mesh_amd.marching_cubes import marching_cubes
    x = torch.linspace(-1, 1, RES, device="cuda")
    X, Y, Z = torch.meshgrid(x, x, x, indexing="ij")
    return marching_cubes((0.6 - torch.sqrt(X * X + Y * Y + Z * Z)).contiguous(), 0.0, div=RES - 1.0, mul=2.0, add=-1.0)


def _capture():
    from nerf2mesh_amd import synthetic
    from nerf2mesh_amd.capture import Capture
    f = synthetic.LEGO_FOCAL * HW / synthetic.LEGO_HW                      # the whole scene in the frame: the sphere has a silhouette
    return Capture.synthetic(synthetic.make_cameras(4, seed=0), H=HW, W=HW, intrinsics=(f, f, HW / 2, HW / 2), alpha=True, device="cuda")


def _trainer(lam, cap, force_graph=False, **over):
    import torch
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    from nerf2mesh_amd.trainer import Stage1Trainer
    torch.manual_seed(0)
    opt = make_options(O=True, bound=1, dt_gamma=0, stage=1, fused_mlp=True, ssaa=1, **({"lambda_ssim": lam} if lam is not None else {}), **over)
    v, f = _sphere()
    tr = Stage1Trainer(NeRFNetwork(opt), opt, None, v, f, torch.device("cuda"), capture=cap)
    if force_graph:
        tr.fused_head = False
    return tr


def _step(tr):
    """One step; what the optimizer was handed (gradients carry the loss scale) and the frame the torch-graph head rendered, with its target."""
    seen, model = {}, tr.model
    step, render = tr.optimizer.step, model.render_stage1

    def spy_step(flagged=()):
        seen["offsets"] = model.vertices_offsets.grad.detach().float().clone()
        table = tr._amp["color"].get("grad_half")
        seen["table"] = (table if table is not None else model.encoder_color.embeddings.grad).detach().float().clone()
        return step(flagged=flagged)

    def spy_render(rays_o, rays_d, mvp, h0, w0, **kw):
        out = render(rays_o, rays_d, mvp, h0, w0, **kw)
        seen["image"], seen["bg"] = out["image"].detach().float().clone(), kw["bg_color"].clone()
        return out
    tr.optimizer.step, model.render_stage1 = spy_step, spy_render
    seen["scale"] = float(tr.optimizer.scale)
    seen["loss"] = float(tr.train_step().detach())
    tr.optimizer.step, model.render_stage1 = step, render
    return seen


@pytest.fixture(scope="module")
def runs():
    cap = _capture()
    on = _trainer(LAM, cap)
    assert on.fused_head is False and on.lambda_ssim == LAM
    out = {"cap": cap, "on": _step(on), "off": _step(_trainer(0, cap, force_graph=True)), "off2": _step(_trainer(0, cap, force_graph=True))}
    return out


def _ulp(x):
    return float(np.spacing(np.float32(abs(x))))


def test_loss_gains_lambda_times_one_minus_ssim(runs):
    """loss(lambda_ssim = 0.2) = loss(lambda_ssim = 0, torch-graph head) + 0.2 (1 - SSIM), SSIM by the float64 model from the frame the
    lambda_ssim = 0 trainer rendered and its target.  Allowed: the kernel's SSIM tolerance (4 x the fp32 yardstick's largest error,
    tests/test_ssim_gpu.py) times 0.2, the fp32 roundings of the two losses and of the sum (one ulp of the loss each), and 10 x what two
    runs of the lambda_ssim = 0 step differ by (the margin tests/test_stage1.py gives that distance)."""
    on, off, off2, cap = runs["on"], runs["off"], runs["off2"], runs["cap"]
    assert on["scale"] == off["scale"]
    rgba = cap.view(0)[2]
    gt = rgba[:, :3] * rgba[:, 3:] + off["bg"] * (1 - rgba[:, 3:])
    s = float(R.ssim_model(off["image"].cpu().view(HW, HW, 3), gt.cpu().view(HW, HW, 3))[0])
    want = LAM * (1.0 - s)
    tol = LAM * 4.0 * R.yardstick()["mean"] + 3 * _ulp(on["loss"]) + 10 * abs(off["loss"] - off2["loss"])
    print(f"loss with the term {on['loss']:.8g}, without {off['loss']:.8g} (a second run {off2['loss']:.8g}); SSIM of the frame {s:.6f}, "
          f"term {want:.6g}, difference {on['loss'] - off['loss']:.6g}, allowed {tol:.3g}")
    assert want > 100 * tol                                               # the term is far above what the comparison resolves
    assert abs((on["loss"] - off["loss"]) - want) <= tol


def test_gradients_are_finite_and_carry_the_term(runs):
    import torch
    on, off, off2 = runs["on"], runs["off"], runs["off2"]
    for k in ("offsets", "table"):
        assert bool(torch.isfinite(on[k]).all()) and float(on[k].abs().max()) > 0, k
        noise = float((off[k] - off2[k]).abs().max())                     # float atomics in the raster / antialias / table backward
        diff = float((on[k] - off[k]).abs().max())
        print(f"{k}: max |gradient| {float(on[k].abs().max()):.4g}, with-vs-without the term {diff:.4g}, two runs without {noise:.4g}")
        assert diff > 10 * noise and diff > 0, k


def test_executor_refuses_the_term_and_keeps_the_default(runs):
    from nerf2mesh_amd.engine_stage1 import Stage1Engine
    cap = runs["cap"]
    tr = _trainer(LAM, cap)
    assert not Stage1Engine.supported(tr)
    with pytest.raises(ValueError, match="Stage1Engine covers"):
        Stage1Engine(tr)
    default = _trainer(None, cap)                                         # no lambda_ssim given: the default, 0
    assert default.opt.lambda_ssim == 0 and default.fused_head is True and Stage1Engine.supported(default)


def test_option_and_construction_checks():
    import torch
    from nerf2mesh_amd.options import make_options
    assert make_options().lambda_ssim == 0
    assert make_options(lambda_ssim=0.2).lambda_ssim == 0.2
    from nerf2mesh_amd import synthetic
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.trainer import Stage1Trainer
    opt = make_options(O=True, bound=1, dt_gamma=0, stage=1, fused_mlp=True, ssaa=1, lambda_ssim=0.2)
    v, f = _sphere()
    with pytest.raises(ValueError, match="at least 11 x 11"):
        Stage1Trainer(NeRFNetwork(opt), opt, synthetic.make_cameras(2, seed=0), v, f, torch.device("cuda"), H=10, W=32)
