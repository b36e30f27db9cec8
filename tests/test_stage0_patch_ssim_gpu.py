"""GPU: patch batches (options.patch_size) and the opt-in patch SSIM term (options.lambda_patch_ssim) of trainer.Stage0Trainer on a
synthetic capture of 4 views at 48 x 48: patch_size 16, num_rays 1024 (B = 4 patches), the fused field.

One step with lambda_patch_ssim = 0.2 against one step of an identically seeded trainer with lambda_patch_ssim = 0 on the unfused loss
branch (the branch the term selects): the loss gains 0.2 (1 - SSIM), SSIM by the float64 model of tests/ssim_ref.py, per patch, on the
zero-weight trainer's last_patches."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ssim_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu

LAM, HW, P, RAYS = 0.2, 48, 16, 1024


def _capture():
    from nerf2mesh_amd import synthetic
    from nerf2mesh_amd.capture import Capture
    f = synthetic.LEGO_FOCAL * HW / synthetic.LEGO_HW                      # the whole scene in the frame
    return Capture.synthetic(synthetic.make_cameras(4, seed=0), H=HW, W=HW, intrinsics=(f, f, HW / 2, HW / 2), alpha=True, device="cuda")


def _trainer(cap, unfused=False, **over):
    import torch
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    from nerf2mesh_amd.trainer import Stage0Trainer
    torch.manual_seed(0)
    opt = make_options(O=True, bound=1, dt_gamma=0, iters=30000, fused_mlp=True, num_rays=RAYS, **over)
    tr = Stage0Trainer(NeRFNetwork(opt), opt, None, torch.device("cuda", 0), seed=0, capture=cap)
    if unfused:
        tr.fused_loss = False
    tr.mark_untrained()
    return tr


def _step(tr):
    """One step: the loss, and the table gradients the optimizer was handed (they carry the loss scale)."""
    seen, model = {}, tr.model
    step = tr.optimizer.step

    def spy_step(flagged=()):
        half = tr._amp["color"].get("grad_half")
        seen["color"] = (half if half is not None else model.encoder_color.embeddings.grad).detach().float().clone()
        seen["density"] = model.encoder.embeddings.grad.detach().float().clone()
        return step(flagged=flagged)
    tr.optimizer.step = spy_step
    seen["scale"] = float(tr.optimizer.scale)
    seen["loss"] = float(tr.train_step().detach())
    tr.optimizer.step = step
    seen["patches"] = tr.last_patches
    return seen


@pytest.fixture(scope="module")
def runs():
    cap = _capture()
    on = _trainer(cap, patch_size=P, lambda_patch_ssim=LAM)
    assert on.fused_loss is False and on.lambda_patch_ssim == LAM and on.patch_size == P
    return {"cap": cap, "on": _step(on), "off": _step(_trainer(cap, unfused=True, patch_size=P)),
            "off2": _step(_trainer(cap, unfused=True, patch_size=P))}


def test_batch_is_four_patches_and_last_patches_has_the_stated_shape(runs):
    import torch
    for k in ("on", "off"):
        image, gt = runs[k]["patches"]
        assert image.shape == gt.shape == (RAYS // (P * P), P, P, 3) and image.shape[0] == 4
        assert not image.requires_grad and not gt.requires_grad and image.is_cuda
        assert bool(torch.isfinite(image).all()) and float(gt.min()) >= 0 and float(gt.max()) <= 1
    assert torch.equal(runs["on"]["patches"][1], runs["off"]["patches"][1])            # the same seed draws the same patches


def test_loss_gains_lambda_times_one_minus_ssim(runs):
    """loss(lambda_patch_ssim = 0.2) = loss(0, unfused branch) + 0.2 (1 - SSIM): SSIM the float64 model's mean over the four patches of the
    zero-weight trainer.  Allowed: 0.2 x the kernel's SSIM tolerance (4 x the fp32 yardstick's largest error, tests/test_ssim_patches_gpu.py)
    plus the distance two zero-weight runs of this step show."""
    import torch
    on, off, off2 = runs["on"], runs["off"], runs["off2"]
    assert on["scale"] == off["scale"]
    image, gt = (t.cpu() for t in off["patches"])
    s = float(torch.stack([R.ssim_model(image[b], gt[b])[0] for b in range(image.shape[0])]).mean())
    want = LAM * (1.0 - s)
    tol = LAM * 4.0 * R.yardstick()["mean"] + abs(off["loss"] - off2["loss"])
    print(f"loss with the term {on['loss']:.8g}, without {off['loss']:.8g} (a second run {off2['loss']:.8g}); SSIM of the patches {s:.6f}, "
          f"term {want:.6g}, difference {on['loss'] - off['loss']:.6g}, allowed {tol:.3g}")
    assert want > 100 * tol                                               # the term is far above what the comparison resolves
    assert abs((on["loss"] - off["loss"]) - want) <= tol


def test_the_term_reaches_the_tables(runs):
    import torch
    on, off, off2 = runs["on"], runs["off"], runs["off2"]
    for k in ("color", "density"):
        assert bool(torch.isfinite(on[k]).all()) and float(on[k].abs().max()) > 0, k
        noise = float((off[k] - off2[k]).abs().max())                     # float atomics in the table backward
        diff = float((on[k] - off[k]).abs().max())
        print(f"{k}: max |gradient| {float(on[k].abs().max()):.4g}, with-vs-without the term {diff:.4g}, two runs without {noise:.4g}")
        assert diff > 10 * noise and diff > 0, k


def test_individual_codes_take_one_view_per_patch(runs):
    import torch
    tr = _trainer(runs["cap"], patch_size=P, lambda_patch_ssim=LAM, ind_dim=8, ind_num=16)
    tr.batch()
    idx = tr._index
    assert idx.dtype == torch.int32 and idx.shape == (RAYS,)
    per_patch = idx.view(-1, P * P)
    assert bool((per_patch == per_patch[:, :1]).all()) and 0 <= int(idx.min()) and int(idx.max()) < len(runs["cap"])
    tr._next = None
    loss = float(tr.train_step().detach())
    assert loss == loss and tr.last_patches[0].shape == (4, P, P, 3)


def test_construction_checks(runs):
    cap = runs["cap"]
    for size in (1, 8):
        with pytest.raises(ValueError, match="lambda_patch_ssim > 0 needs patch_size 11 .. 64"):
            _trainer(cap, patch_size=size, lambda_patch_ssim=LAM)
    for size in (HW, HW + 1):
        with pytest.raises(ValueError, match="patch_size must be"):
            _trainer(cap, patch_size=size)


def test_defaults_and_the_executor(runs):
    from nerf2mesh_amd.engine import Stage0Engine
    cap = runs["cap"]
    tr = _trainer(cap)
    assert tr.opt.patch_size == 1 and tr.opt.lambda_patch_ssim == 0 and tr.patch_size == 1 and tr.fused_loss is True
    assert Stage0Engine.supported(tr.model, tr.opt, capture=cap)
    tr.train_step()
    assert tr.last_patches is None and tr._patch == 0                     # pixel batches keep nothing
    zero = _trainer(cap, patch_size=P)                                    # patch batches alone stay on the fused loss
    assert zero.fused_loss is True and not Stage0Engine.supported(zero.model, zero.opt, capture=cap)
    zero.train_step()
    assert zero.last_patches[0].shape == (4, P, P, 3)
    on = _trainer(cap, patch_size=P, lambda_patch_ssim=LAM)
    assert not Stage0Engine.supported(on.model, on.opt, capture=cap)
    on.opt.patch_size = 1                                                 # the weight alone already rules the executor out
    assert not Stage0Engine.supported(on.model, on.opt, capture=cap)
