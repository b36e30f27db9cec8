"""Both stage-0 drivers on a COLMAP capture: the tiny reconstruction of tests/golden/colmap_tiny with its views rendered again at 24 x 20 px,
written by save_colmap and read by load_colmap.  With sparse depth off the capture behaves like the same data in the nerf format; with it
on, engine.Stage0Engine and trainer.Stage0Trainer take the same depth / plain steps on the same views and stay as close as
tests/test_engine.py asks of them on every step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TINY = os.path.join(HERE, "golden", "colmap_tiny")
STEPS = 30


@pytest.fixture(scope="module")
def recon(tmp_path_factory):
    """The enlarged reconstruction on disk: same cameras and points as the tiny one, 24 x 20 px views of the box scene."""
    from nerf2mesh_amd.capture import Capture
    tiny = Capture.load_colmap(TINY, split="trainval", scale=1.0, keep_model=True)
    fx, fy, cx, cy = tiny.intrinsics
    big = Capture.synthetic(tiny.poses, H=20, W=24, intrinsics=(2 * fx, 2 * fy, 2 * cx, 2 * cy), alpha=True)
    root = str(tmp_path_factory.mktemp("colmap24"))
    big.save_colmap(root, tiny.colmap["points"], errors=tiny.colmap["errors"])
    return root


def _load(recon, **kw):
    from nerf2mesh_amd.capture import Capture
    return Capture.load_colmap(recon, split="train", scale=1.0, device="cuda", **kw)


def _rel(p, q):
    return ((p.float() - q.float()).norm() / p.float().norm().clamp_min(1e-30)).item()


def _run(cls, cap, steps=STEPS, against=None, **over):
    """-> driver, per-step losses, per-step parameters.  The parameters are {name: clone} of every entry of named_parameters(), the hash-grid
    tables included -- or, given such a list as `against`, {name: relative distance to it} (so only one run keeps its clones)."""
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    torch.manual_seed(0)
    opt = make_options(O=True, bound=1, dt_gamma=0, iters=30000, fused_mlp=True, diffuse_step=12, enable_cam_near_far=True, **over)
    opt.num_rays, opt.num_points = 1024, 1 << 14
    model = NeRFNetwork(opt).to("cuda")
    model.update_aabb(cap.pts_aabb.cuda())
    tr = cls(model, opt, None, torch.device("cuda", 0), seed=0, capture=cap)
    tr.mark_untrained()
    losses, params = [], []
    for _ in range(steps):
        losses.append(float(tr.train_step()))
        if against is None:
            params.append({n: p.detach().clone() for n, p in tr.model.named_parameters()})
        else:
            params.append({n: _rel(against[len(params)][n], p.detach()) for n, p in tr.model.named_parameters()})
        if hasattr(tr, "_work_cap"):                                     # the step workspace is sized once: a depth step never regrows it
            cap0 = tr._work_cap if len(losses) == 1 else cap0
            assert tr._work_cap[1] == cap0[1] >= (0 if tr.depth_schedule is None else max(cap.sparse_depth.counts))
    torch.cuda.synchronize()
    return tr, losses, params


def _drivers():
    from nerf2mesh_amd.engine import Stage0Engine
    from nerf2mesh_amd.trainer import Stage0Trainer
    return Stage0Engine, Stage0Trainer


@pytest.mark.parametrize("driver", ["engine", "trainer"])
def test_depth_off_equals_the_same_data_in_the_nerf_format(recon, tmp_path, driver):
    from nerf2mesh_amd.capture import Capture
    cls = _drivers()[driver == "trainer"]
    cap = _load(recon, sparse_depth=True)
    cap.save_nerf(str(tmp_path), scale=1.0)
    nerf = Capture.load_nerf(str(tmp_path), split="train", scale=1.0, device="cuda")
    assert torch.equal(nerf.poses, cap.poses) and torch.equal(nerf.bank, cap.bank) and nerf.intrinsics == cap.intrinsics
    nerf.cam_near_far, nerf.pts_aabb = cap.cam_near_far, cap.pts_aabb
    a, la, pa = _run(cls, cap, enable_sparse_depth=False)
    b, lb, pb = _run(cls, nerf, enable_sparse_depth=False)
    assert a.depth_schedule is None and b.depth_schedule is None
    assert a.samples_seen == b.samples_seen and la == lb
    for (n, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(p, q), n


def test_depth_steps_engine_against_trainer(recon):
    Engine, Trainer = _drivers()
    cap = _load(recon, sparse_depth=True)
    a, la, pa = _run(Trainer, cap, enable_sparse_depth=True)
    b, lb, d_te = _run(Engine, cap, against=pa, enable_sparse_depth=True)
    assert Engine.supported(b.model, b.opt)                              # depth in density mode stays on the step executor
    a2, la2, d_tt = _run(Trainer, cap, against=pa, enable_sparse_depth=True)
    sa, sb = a.depth_schedule.log[:STEPS], b.depth_schedule.log[:STEPS]
    assert sa == sb and sum(v is not None for v in sa) >= 2, sa          # same depth / plain steps on the same views
    print("depth steps:", [(i + 1, v) for i, v in enumerate(sa) if v is not None])
    assert a.samples_seen == b.samples_seen and a.rays_seen == b.rays_seen
    assert a.num_rays == b.num_rays
    np.testing.assert_allclose(la, lb, rtol=2e-4, atol=1e-7)             # every step, depth steps included (tests/test_engine.py's tolerance)
    assert any("encoder" in n for n in pa[0]) and len(pa[0]) == len(list(a.model.named_parameters()))
    for n in pa[0]:                                                      # the clones are of tensors that training moves
        assert not torch.equal(pa[0][n], pa[-1][n]), n
    for i in range(STEPS):                                               # ... and its yardstick for the parameters: a second trainer run,
        for n in pa[i]:                                                  # every named parameter on its own, the encoder tables included
            if i == STEPS - 1 or sa[i] is not None:
                print(f"step {i + 1:2d} {'depth' if sa[i] is not None else 'plain'} {n:36s} trainer-vs-engine {d_te[i][n]:.3g}   "
                      f"trainer-vs-trainer {d_tt[i][n]:.3g}")
            assert d_te[i][n] <= 10 * d_tt[i][n] + 2e-4, (i + 1, sa[i], n, d_te[i][n], d_tt[i][n])
    # the depth term is in the loss: the same run with lambda_depth = 0 has other losses from the first depth step on
    c, lc, _ = _run(Engine, cap, enable_sparse_depth=True, lambda_depth=0.0)
    first = next(i for i, v in enumerate(sa) if v is not None)
    assert lc[:first] == lb[:first] and lc[first] != lb[first]


def test_two_engine_runs_from_one_seed_end_in_identical_bits(recon):
    Engine, _ = _drivers()
    cap = _load(recon, sparse_depth=True)
    a, la, _ = _run(Engine, cap, enable_sparse_depth=True)
    b, lb, _ = _run(Engine, cap, enable_sparse_depth=True)
    assert la == lb and a.depth_schedule.log == b.depth_schedule.log
    for (n, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(p, q), n


def test_sdf_with_depth_goes_to_the_trainer(recon):
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    Engine, _ = _drivers()
    for depth, want in ((False, True), (True, False)):
        opt = make_options(O=True, bound=1, dt_gamma=0, fused_mlp=True, sdf=True, enable_sparse_depth=depth)
        assert Engine.supported(NeRFNetwork(opt), opt) == want


def test_train_capture_tool_runs_a_colmap_set_with_depth(recon, tmp_path):
    cmd = [sys.executable, os.path.join(os.path.dirname(HERE), "tools", "train_capture.py"), recon, "--workspace", str(tmp_path), "--data_format", "colmap",
           "--enable_sparse_depth", "--enable_cam_near_far", "--iters0", "60", "--iters1", "20", "--scale", "1.0", "--resolution", "64", "--texture",
           "256", "--eval_views", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["data_format"] == "colmap" and out["depth_steps"] >= 1 and out["train_views"] == 7 and out["held_out_views"] == 2
    assert out["held_out_is_test_split"] and np.isfinite(out["psnr_stage0"]) and np.isfinite(out["psnr_stage1"])
    assert os.path.exists(os.path.join(str(tmp_path), "mesh_stage1"))
