"""Per-image appearance codes (--ind_dim) through both stage-0 drivers, on tests/golden/colmap_tiny with its views rendered again at
24 x 20 px (the set of tests/test_colmap_engine_gpu.py): the step executor takes the configuration, follows the autograd trainer as closely
as tests/test_engine.py asks, touches only the rows of views that exist, leaves an ind_dim = 0 run on the calls it made before; and
tools/train_capture.py runs both stages with codes and reports the training-loss tail."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TINY = os.path.join(HERE, "golden", "colmap_tiny")
IND_NUM = 12


@pytest.fixture(scope="module")
def cap():
    from nerf2mesh_amd.capture import Capture
    tiny = Capture.load_colmap(TINY, split="trainval", scale=1.0, keep_model=True)
    fx, fy, cx, cy = tiny.intrinsics
    big = Capture.synthetic(tiny.poses, H=20, W=24, intrinsics=(2 * fx, 2 * fy, 2 * cx, 2 * cy), alpha=True, device="cuda")
    big.pts_aabb = tiny.pts_aabb
    return big


def _drivers():
    from nerf2mesh_amd.engine import Stage0Engine
    from nerf2mesh_amd.trainer import Stage0Trainer
    return Stage0Engine, Stage0Trainer


def _make(cls, cap, ind_dim, **over):
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    torch.manual_seed(0)
    opt = make_options(O=True, bound=1, dt_gamma=0, iters=30000, fused_mlp=True, diffuse_step=3, ind_dim=ind_dim, ind_num=IND_NUM, **over)
    opt.num_rays, opt.num_points = 1024, 1 << 14
    model = NeRFNetwork(opt).to("cuda")
    if cap.pts_aabb is not None:
        model.update_aabb(torch.as_tensor(cap.pts_aabb).cuda())
    tr = cls(model, opt, None, torch.device("cuda", 0), seed=0, capture=cap)
    tr.mark_untrained()
    return tr


def _run(cls, cap, steps, ind_dim=8, **over):
    tr = _make(cls, cap, ind_dim, **over)
    losses, params = [], []
    for _ in range(steps):
        losses.append(float(tr.train_step()))
        params.append({n: p.detach().clone() for n, p in tr.model.named_parameters()})
    torch.cuda.synchronize()
    return tr, losses, params


def _rel(p, q):
    return ((p.float() - q.float()).norm() / p.float().norm().clamp_min(1e-30)).item()


def test_executor_takes_codes_and_follows_the_trainer(cap):
    Engine, Trainer = _drivers()
    steps = 5                      # diffuse steps 1-2, full shading from step 3
    a, la, pa = _run(Trainer, cap, steps)
    assert a.amp_adam, "codes no longer push the trainer off the fused optimizer"
    assert Engine.supported(a.model, a.opt, capture=cap)                 # fails without the feature: ind_dim > 0 was refused outright
    b, lb, pb = _run(Engine, cap, steps)
    a2, la2, pa2 = _run(Trainer, cap, steps)
    assert b.ind_dim == 8 and a.samples_seen == b.samples_seen and a.rays_seen == b.rays_seen
    np.testing.assert_allclose(la, lb, rtol=2e-4, atol=1e-7)             # tests/test_engine.py's tolerance, every step
    assert "individual_codes" in pa[0] and tuple(pa[0]["individual_codes"].shape) == (IND_NUM, 8)
    for i in (0, steps - 1):                                             # one step from the same state, and the last one
        for n in pa[i]:
            d_te, d_tt = _rel(pa[i][n], pb[i][n]), _rel(pa[i][n], pa2[i][n])
            print(f"step {i + 1} {n:36s} trainer-vs-engine {d_te:.3g}   trainer-vs-trainer {d_tt:.3g}")
            assert d_te <= 10 * d_tt + 2e-4, (i + 1, n, d_te, d_tt)
    V = len(cap)
    assert V < IND_NUM
    for tr, params in ((a, pa), (b, pb)):
        first = torch.zeros_like(params[0]["individual_codes"])
        torch.manual_seed(0)
        from nerf2mesh_amd.network import NeRFNetwork
        first = NeRFNetwork(tr.opt).individual_codes.detach().cuda()     # the state both runs started from
        last = params[-1]["individual_codes"]
        assert torch.equal(last[V:], first[V:]), "rows no view names keep their bits"
        moved = (last[:V] != first[:V]).any(dim=1)
        assert moved.all(), moved.tolist()                               # 5 x ~1000 rays over 9 views: every view was drawn
    with pytest.raises(ValueError, match=rf"{V} views.*ind_num is {V - 1}"):
        from nerf2mesh_amd.network import NeRFNetwork
        from nerf2mesh_amd.options import make_options
        opt = make_options(O=True, bound=1, dt_gamma=0, fused_mlp=True, ind_dim=8, ind_num=V - 1)
        Engine(NeRFNetwork(opt), opt, None, torch.device("cuda", 0), capture=cap)


def test_two_executor_runs_with_codes_end_in_identical_bits(cap):
    Engine, _ = _drivers()
    a, la, pa = _run(Engine, cap, 5)
    b, lb, pb = _run(Engine, cap, 5)
    assert la == lb
    for n in pa[-1]:
        assert torch.equal(pa[-1][n], pb[-1][n]), n
    # evaluation reads row 0 through the fused kernel
    assert np.isfinite(a.eval_psnr(cam=1, downscale=1))


def test_without_codes_the_executor_makes_the_calls_it_made_before(cap, monkeypatch):
    from nerf2mesh_amd import _lib as L
    Engine, _ = _drivers()
    calls, real = [], L.call

    def spy(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(L, "call", spy)
    tr = _make(Engine, cap, 0)
    for _ in range(4):
        tr.train_step()
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert calls.count("n2m_field_forward_train") == 4 and calls.count("n2m_field_backward_train") == 4
    new = [c for c in calls if "_ind" in c or c in ("n2m_batch_views", "n2m_field_sample_views")]
    assert not new, new
    # ... and with codes the new entry points take their place, one view-id launch per prepared batch
    calls.clear()
    monkeypatch.setattr(L, "call", spy)
    tr = _make(Engine, cap, 8)
    for _ in range(4):
        tr.train_step()
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert calls.count("n2m_field_forward_ind_train") == 4 and calls.count("n2m_field_backward_ind_train") == 4
    assert "n2m_field_forward_train" not in calls and calls.count("n2m_batch_views") >= 4


def test_train_capture_tool_trains_with_codes_and_reports_the_loss_tail(cap, tmp_path):
    """Both stages and the export with --ind_dim 8 (stage 1 trains with the view's row, everything else reads row 0).  Whether the codes
    lower the training loss is REPORTED here (`train_loss_tail`), not asserted: on this 24 x 20 px set the loss stops falling after a few
    steps with or without codes, and its level moves more with the model's seed than with the codes (DESIGN 4.22 has the figures)."""
    import json
    import subprocess
    import sys
    from nerf2mesh_amd.capture import Capture
    tiny = Capture.load_colmap(TINY, split="trainval", scale=1.0, keep_model=True)
    root = str(tmp_path / "set")
    cap.save_colmap(root, tiny.colmap["points"], errors=tiny.colmap["errors"])
    cmd = [sys.executable, os.path.join(os.path.dirname(HERE), "tools", "train_capture.py"), root, "--workspace", str(tmp_path / "ws"), "--data_format",
           "colmap", "--iters0", "60", "--iters1", "20", "--scale", "1.0", "--resolution", "64", "--texture", "256", "--eval_views", "2", "--ind_dim", "8",
           "--ind_num", "16"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "(Stage0Engine)" in r.stdout, "codes stay on the step executor"
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print("ind_dim", out["ind_dim"], "train_loss_tail", out["train_loss_tail"])
    assert out["ind_dim"] == 8 and np.isfinite(out["train_loss_tail"]) and out["train_loss_tail"] > 0
    assert np.isfinite(out["psnr_stage0"]) and np.isfinite(out["psnr_stage1"])
