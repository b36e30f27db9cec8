"""Both stages on a capture.Capture.  (1) Only the source changed: the executor and the trainer fed the quantised lego set through the uint8
bank end in the bits they reach when the same decoded pixels sit in their fp32 bank.  (2) A non-square set with fx != fy and an off-centre
principal point trains; a 3-channel set runs without the mask term.  (3) Stage 1 takes its size, its projections and its view cache from
the capture."""
import numpy as np
import pytest
import torch

from nerf2mesh_amd import synthetic
from nerf2mesh_amd.capture import Capture

pytestmark = pytest.mark.gpu

INTR = (70.0, 60.0, 30.5, 25.25)          # 64 x 48, fx != fy, principal point off-centre


def _opt(**over):
    from nerf2mesh_amd.options import make_options
    kw = dict(O=True, bound=1, dt_gamma=0, iters=30000, fused_mlp=True)
    kw.update(over)
    return make_options(**kw)


def _model(opt):
    from nerf2mesh_amd.network import NeRFNetwork
    torch.manual_seed(0)
    return NeRFNetwork(opt)


@pytest.fixture(scope="module")
def lego_capture():
    return Capture.synthetic(synthetic.make_cameras(4, seed=0), device="cuda")


@pytest.fixture(scope="module")
def small_captures():
    poses = synthetic.make_cameras(6, seed=0)
    return {a: Capture.synthetic(poses, H=48, W=64, intrinsics=INTR, alpha=a, device="cuda") for a in (True, False)}


def _ab(cls, cap, steps=8):
    dev = torch.device("cuda", 0)
    runs = []
    for through_capture in (True, False):
        opt = _opt()
        if through_capture:
            tr = cls(_model(opt), opt, None, dev, seed=0, capture=cap)
        else:
            tr = cls(_model(opt), opt, cap.poses, dev, seed=0)
            tr.images = cap.decode()                              # the same pixels as fp32 [V, H*W, 4]: 41 MB
        tr.mark_untrained()
        losses = [tr.train_step().detach().clone() for _ in range(steps)]
        torch.cuda.synchronize()
        runs.append((torch.stack([l.reshape(()) for l in losses]).cpu(), [p.detach().clone() for p in tr.model.parameters()], tr))
    (la, pa, a), (lb, pb, b) = runs
    print("losses through the capture:", la.tolist())
    print("losses through the fp32 bank:", lb.tolist())
    assert a.images is None, "the capture path renders no fp32 bank"
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32)), (la.tolist(), lb.tolist())
    for (n, _), p, q in zip(a.model.named_parameters(), pa, pb):
        assert torch.equal(p, q), n
    assert a.samples_seen == b.samples_seen and a.rays_seen == b.rays_seen


def test_executor_only_the_source_changed(lego_capture):
    from nerf2mesh_amd.engine import Stage0Engine
    assert lego_capture.intrinsics == (synthetic.LEGO_FOCAL, synthetic.LEGO_FOCAL, 400.0, 400.0) and lego_capture.nbytes == 4 * 800 * 800 * 4
    _ab(Stage0Engine, lego_capture)


def test_trainer_only_the_source_changed(lego_capture):
    from nerf2mesh_amd.trainer import Stage0Trainer
    _ab(Stage0Trainer, lego_capture)


def _train(cap, steps=40, **over):
    from nerf2mesh_amd.engine import Stage0Engine
    opt = _opt(**over)
    assert opt.mark_untrained
    eng = Stage0Engine(_model(opt), opt, None, torch.device("cuda", 0), seed=0, capture=cap)
    eng.mark_untrained()
    losses = [float(eng.train_step()) for _ in range(steps)]
    torch.cuda.synchronize()
    return eng, losses


def test_non_square_capture_trains(small_captures):
    cap = small_captures[True]
    assert (cap.H, cap.W, len(cap)) == (48, 64, 6) and cap.has_alpha
    eng, losses = _train(cap)
    print("losses:", losses)
    assert np.isfinite(losses).all()
    assert np.mean(losses[-5:]) < np.mean(losses[:5])
    psnr = eng.eval_psnr(cam=1, downscale=1)
    print("PSNR of view 1:", psnr)
    assert np.isfinite(psnr)
    assert np.isfinite(eng.eval_psnr(cam=0, downscale=2, capture=small_captures[False]))      # another set handed in


def test_rgb_capture_runs_without_the_mask_term(small_captures):
    cap = small_captures[False]
    assert not cap.has_alpha
    a, la = _train(cap)
    assert a.opt.lambda_mask > 0
    b, lb = _train(cap, lambda_mask=0)
    print("losses:", la)
    assert np.isfinite(la).all()
    assert np.mean(la[-5:]) < np.mean(la[:5])
    assert np.isfinite(a.eval_psnr(cam=1, downscale=1))
    assert np.array_equal(np.float32(la).view(np.int32), np.float32(lb).view(np.int32))
    for (n, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(p, q), n
    # ... and it is a term: with an alpha channel the weight changes the loss
    _, lc = _train(small_captures[True], steps=2)
    _, ld = _train(small_captures[True], steps=2, lambda_mask=0)
    assert lc[0] != ld[0]


def test_stage1_takes_its_views_from_the_capture(small_captures):
    from nerf2mesh_amd.engine_stage1 import Stage1Engine
    from nerf2mesh_amd.trainer import Stage1Trainer
    cap = small_captures[True]
    dev = torch.device("cuda", 0)
    v, f = synthetic.scene_mesh(6000)
    opt = _opt(stage=1, ssaa=2)
    tr = Stage1Trainer(_model(opt), opt, None, v, f, dev, capture=cap)
    assert (tr.H, tr.W) == (48, 64) and torch.equal(tr.mvps, cap.mvps) and torch.equal(tr.poses, cap.poses)
    o, d, rgba = tr._view(2)
    wo, wd, wrgba, wdirs = cap.view(2, dirs_ssaa=2)
    assert torch.equal(o, wo) and torch.equal(d, wd) and torch.equal(rgba, wrgba) and torch.equal(tr._dirs[2], wdirs)
    assert wdirs.shape == (96 * 128, 3)
    losses = [float(tr.train_step().detach()) for _ in range(3)]
    assert np.isfinite(losses).all(), losses
    assert tr.model.last_covered > 0, "the mesh is in front of the capture's cameras"
    if Stage1Engine.supported(tr):
        eng = Stage1Engine(tr)
        assert (eng.h0, eng.w0) == (48, 64)
        loss = float(eng.train_step())
        assert np.isfinite(loss), loss
