"""Both stages and tools/train_capture.py on sets with per-view intrinsics: the lego cameras through Capture.synthetic(intrinsics=[V,4]) at
24 x 20 px, 9 views, focal lengths spread +-15 %, principal points off-centre by up to 2 px.

(1) engine.Stage0Engine and trainer.Stage0Trainer agree on it step by step -- tests/test_capture_engine_gpu.py compares two runs of ONE
driver bit for bit (uint8 bank against fp32 bank), which has no counterpart here (the fp32 bank has no per-view intrinsics); the criterion
for the two DRIVERS is the one tests/test_colmap_engine_gpu.py restates from tests/test_engine.py: the same rays and samples, losses within
rtol 2e-4 on every step, every parameter as close as two trainer runs are, times 10, + 2e-4.  (2) With equal rows the table form
(per_view=True) ends in the bits of the shared form, both drivers.  (3) The per-view set trains.  (4) Dense and sparse depth on a per-view
COLMAP set written by save_colmap.  (5) Stage 1.  (6) The tool on a DTU folder written by save_dtu."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dense_depth_case as DC   # noqa: E402
import stage1_case as S1        # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 30
V, H, W = 9, 20, 24
BASE = (30.0, 28.0, 12.0, 10.0)


def _rows(equal=False):
    """[V,4]: focal lengths spread over +-15 %, centres off by up to 2 px, every row different (equal=True: row 0 for every view)."""
    t = np.linspace(-1.0, 1.0, V)
    rows = np.stack([BASE[0] * (1 + 0.15 * t), BASE[1] * (1 - 0.15 * t[::-1] * np.cos(3 * t)), BASE[2] + 2.0 * np.sin(2.5 * t),
                     BASE[3] - 2.0 * np.cos(4 * t) * t], -1)
    assert len({tuple(r) for r in rows}) == V and np.abs(rows[:, :2] / np.array(BASE[:2]) - 1).max() <= 0.15 + 1e-12
    assert np.abs(rows[:, 2:] - np.array(BASE[2:])).max() <= 2.0
    return np.tile(rows[0], (V, 1)) if equal else rows


def _poses():
    from nerf2mesh_amd import synthetic
    return synthetic.make_cameras(V, seed=0)


@pytest.fixture(scope="module")
def pv_capture():
    from nerf2mesh_amd.capture import Capture
    cap = Capture.synthetic(_poses(), H=H, W=W, intrinsics=_rows(), device="cuda")
    assert cap.per_view_intrinsics and tuple(cap.intrinsics.shape) == (V, 4) and cap.intrinsics.is_cuda
    return cap


def _drivers():
    from nerf2mesh_amd.engine import Stage0Engine
    from nerf2mesh_amd.trainer import Stage0Trainer
    return Stage0Engine, Stage0Trainer


def _rel(p, q):
    return ((p.float() - q.float()).norm() / p.float().norm().clamp_min(1e-30)).item()


def _run(cls, cap, steps=STEPS, against=None, keep=True, plain_recipe=False, **over):
    """-> driver, per-step losses, per-step parameters ({name: clone}, or {name: relative distance to `against`})."""
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    torch.manual_seed(0)
    if plain_recipe:          # tests/test_capture_engine_gpu.py's options: the recipe as it is (no early switch to full shading, default batch)
        opt = make_options(O=True, bound=1, dt_gamma=0, iters=30000, fused_mlp=True, **over)
    else:                     # tests/test_colmap_engine_gpu.py's: full shading from step 12 on, so that 30 steps cover both, small batches
        opt = make_options(O=True, bound=1, dt_gamma=0, iters=30000, fused_mlp=True, diffuse_step=12, **over)
        opt.num_rays, opt.num_points = 1024, 1 << 14
    model = NeRFNetwork(opt).to("cuda")
    if getattr(cap, "pts_aabb", None) is not None:
        model.update_aabb(cap.pts_aabb.cuda())
    tr = cls(model, opt, None, torch.device("cuda", 0), seed=0, capture=cap)
    tr.mark_untrained()
    losses, params = [], []
    for _ in range(steps):
        losses.append(float(tr.train_step().detach()))
        if against is not None:
            params.append({n: _rel(against[len(params)][n], p.detach()) for n, p in tr.model.named_parameters()})
        elif keep:
            params.append({n: p.detach().clone() for n, p in tr.model.named_parameters()})
    torch.cuda.synchronize()
    return tr, losses, params


def _engine_against_trainer(cap, **over):
    Engine, Trainer = _drivers()
    a, la, pa = _run(Trainer, cap, **over)
    b, lb, d_te = _run(Engine, cap, against=pa, **over)
    a2, la2, d_tt = _run(Trainer, cap, against=pa, **over)
    assert Engine.supported(b.model, b.opt)
    print("engine :", [f"{x:.5f}" for x in lb])
    print("trainer:", [f"{x:.5f}" for x in la])
    assert a.samples_seen == b.samples_seen and a.rays_seen == b.rays_seen
    np.testing.assert_allclose(la, lb, rtol=2e-4, atol=1e-7)
    for n in pa[0]:
        assert not torch.equal(pa[0][n], pa[-1][n]), n
    for i in range(len(pa)):
        for n in pa[i]:
            if i == len(pa) - 1:
                print(f"step {i + 1:2d} {n:36s} trainer-vs-engine {d_te[i][n]:.3g}   trainer-vs-trainer {d_tt[i][n]:.3g}")
            assert d_te[i][n] <= 10 * d_tt[i][n] + 2e-4, (i + 1, n, d_te[i][n], d_tt[i][n])
    return a, b, la, lb


def test_engine_against_trainer_on_the_per_view_set(pv_capture):
    _engine_against_trainer(pv_capture)


@pytest.mark.parametrize("driver", ["engine", "trainer"])
def test_equal_rows_table_form_equals_the_shared_form(driver):
    from nerf2mesh_amd.capture import Capture
    cls = _drivers()[driver == "trainer"]
    table = Capture.synthetic(_poses(), H=H, W=W, intrinsics=_rows(equal=True), device="cuda", per_view=True)
    shared = Capture.synthetic(_poses(), H=H, W=W, intrinsics=_rows(equal=True), device="cuda")
    assert table.per_view_intrinsics and not shared.per_view_intrinsics
    assert torch.equal(table.bank, shared.bank) and torch.equal(table.mvps, shared.mvps)
    a, la, _ = _run(cls, table, keep=False)
    b, lb, _ = _run(cls, shared, keep=False)
    assert np.array_equal(np.float32(la).view(np.int32), np.float32(lb).view(np.int32)), (la, lb)
    assert a.samples_seen == b.samples_seen and a.rays_seen == b.rays_seen
    for (n, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(p, q), n
    assert torch.equal(a.model.density_grid, b.model.density_grid)                 # mark_untrained_grid's two forms


def test_per_view_set_trains(pv_capture):
    """tests/test_capture_engine_gpu.py's assertion for its non-square off-centre set, under its options and step count: finite losses, the
    last five below the first five.  (Under this file's other options the switch to full shading at step 12 lifts the loss -- 0.07 -> 0.12
    measured -- whatever the intrinsics are; that says nothing about training.)"""
    Engine, _ = _drivers()
    eng, losses, _ = _run(Engine, pv_capture, steps=40, keep=False, plain_recipe=True)
    print("losses:", losses)
    assert np.isfinite(losses).all()
    assert np.mean(losses[-5:]) < np.mean(losses[:5])
    assert np.isfinite(eng.eval_psnr(cam=1, downscale=1)) and np.isfinite(eng.eval_psnr(cam=8, downscale=2))


@pytest.fixture(scope="module")
def pv_recon(tmp_path_factory):
    """A per-view COLMAP reconstruction written by save_colmap: the tiny reconstruction's cameras, 24 x 20 px views rendered at 9 different
    rows, the scene's lattice points, and a depth map per view (ray-box depth at that view's row)."""
    from nerf2mesh_amd import synthetic
    from nerf2mesh_amd.capture import Capture
    tiny = Capture.load_colmap(DC.TINY, split="trainval", scale=1.0)
    assert len(tiny) == V
    rows = _rows()
    big = Capture.synthetic(tiny.poses, H=H, W=W, intrinsics=rows, alpha=True)
    root = str(tmp_path_factory.mktemp("colmap24pv"))
    depths = [DC.box_depth_maps(tiny.poses[v:v + 1], H, W, tuple(rows[v]))[0] for v in range(V)]
    big.save_colmap(root, synthetic.scene_points().numpy(), depths=depths)
    return root


def _load(root, **kw):
    from nerf2mesh_amd.capture import Capture
    cap = Capture.load_colmap(root, split="train", scale=1.0, device="cuda", per_view_intrinsics=True, **kw)
    assert cap.per_view_intrinsics and len(cap) == 7 and np.array_equal(cap.intrinsics_host, _rows()[1:8])
    return cap


def test_dense_depth_on_a_per_view_colmap_set(pv_recon):
    """tests/test_dense_depth_engine_gpu.py's criterion: same rays and samples, losses within rtol 2e-4 on every step (lambda_depth = 10)."""
    Engine, Trainer = _drivers()
    cap = _load(pv_recon, dense_depth=True)
    assert (cap.dense_depth_scale_bias[:, 0] > 0).all()
    over = dict(enable_dense_depth=True, enable_cam_near_far=True, lambda_depth=10.0)
    b, lb, _ = _run(Engine, cap, keep=False, **over)
    a, la, _ = _run(Trainer, cap, keep=False, **over)
    assert Engine.supported(b.model, b.opt) and b.dense_depth is not None
    assert a.samples_seen == b.samples_seen and a.rays_seen == b.rays_seen
    np.testing.assert_allclose(la, lb, rtol=2e-4, atol=1e-7)
    off = _run(Engine, cap, keep=False, enable_cam_near_far=True)[1]
    assert all(x != y for x, y in zip(lb[1:], off[1:]))                            # the term is in the loss


def test_sparse_depth_on_a_per_view_colmap_set(pv_recon):
    """tests/test_colmap_engine_gpu.py's criterion: the same depth / plain steps on the same views, losses within rtol 2e-4 on every step,
    every parameter within 10 x the trainer-vs-trainer distance + 2e-4."""
    cap = _load(pv_recon, sparse_depth=True)
    a, b, la, lb = _engine_against_trainer(cap, enable_sparse_depth=True, enable_cam_near_far=True)
    sa, sb = a.depth_schedule.log[:STEPS], b.depth_schedule.log[:STEPS]
    assert sa == sb and sum(v is not None for v in sa) >= 2, sa
    assert len({tuple(cap.intrinsics_host[v]) for v in sa if v is not None}) >= 2      # depth steps on views with different rows


# ----------------------------------------------------------------------------------------------------------------------------- stage 1
def _stage1(cap, steps=10, engine=False):
    from nerf2mesh_amd.engine_stage1 import Stage1Engine
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    from nerf2mesh_amd.trainer import Stage1Trainer
    torch.manual_seed(0)
    from nerf2mesh_amd import synthetic
    v, f = synthetic.scene_mesh(S1.FACES)                             # the mesh of tests/stage1_case.py
    opt = make_options(O=True, bound=1, dt_gamma=0, stage=1, fused_mlp=True)
    tr = Stage1Trainer(NeRFNetwork(opt), opt, None, v, f, torch.device("cuda", 0), capture=cap)
    for _ in range(500):
        tr.scheduler.step()
    step = tr.train_step
    if engine:
        assert Stage1Engine.supported(tr)
        step = Stage1Engine(tr).train_step
    losses = [float(torch.as_tensor(step()).detach()) for _ in range(steps)]
    torch.cuda.synchronize()
    m = tr.model
    params = {"colour table": m.encoder_color.embeddings.detach().float().clone(), "offsets": m.vertices_offsets.detach().clone(),
              **{f"mlp{i}": p.detach().clone() for i, p in enumerate(list(m.color_net.parameters()) + list(m.specular_net.parameters()))}}
    return tr, losses, params


@pytest.fixture(scope="module")
def stage1_captures():
    from nerf2mesh_amd.capture import Capture
    rows = _rows() * (64 / 24)                                        # the stage-1 case's 64 x 64 view
    rows[:, 3] += 32 - rows[0, 3]
    eq = np.tile(rows[0], (V, 1))
    mk = lambda r, pv: Capture.synthetic(_poses(), H=S1.H0, W=S1.W0, intrinsics=r, device="cuda", per_view=pv)
    return {"table": mk(eq, True), "shared": mk(eq, None), "rows": mk(rows, None)}


@pytest.mark.parametrize("engine", [False, True])
def test_stage1_equal_rows_equal_the_shared_capture(stage1_captures, engine):
    """The raster and antialias backward add with float atomics, so two runs of one configuration are the yardstick for `bitwise` here: the
    first step's loss (no atomics in the forward) must be bit-equal, and the view cache -- everything the capture hands to stage 1 -- too."""
    table, shared = stage1_captures["table"], stage1_captures["shared"]
    assert table.per_view_intrinsics and not shared.per_view_intrinsics and torch.equal(table.mvps, shared.mvps)
    for v in range(V):
        for a, b in zip(table.view(v, dirs_ssaa=2), shared.view(v, dirs_ssaa=2)):
            assert torch.equal(a, b), v
    a, la, pa = _stage1(table, engine=engine)
    b, lb, pb = _stage1(shared, engine=engine)
    b2, lb2, pb2 = _stage1(shared, engine=engine)
    assert torch.equal(a.mvps, b.mvps) and la[0] == lb[0]
    if lb == lb2 and all(torch.equal(pb[k], pb2[k]) for k in pb):                  # the configuration is reproducible: then it is bitwise
        assert la == lb
        for k in pa:
            assert torch.equal(pa[k], pb[k]), k
    else:
        rel = lambda x, y: float((x - y).norm() / x.norm().clamp_min(1e-30))
        for k in pa:
            assert rel(pb[k], pa[k]) <= 10 * rel(pb[k], pb2[k]) + 2e-3, k


def test_stage1_drivers_agree_on_different_rows(stage1_captures):
    """tests/test_stage1.py's criterion: first loss within 1e-5 relative, parameters within 10 x trainer-vs-trainer + 2e-3."""
    cap = stage1_captures["rows"]
    assert cap.per_view_intrinsics
    a, la, pa = _stage1(cap)
    a2, la2, pa2 = _stage1(cap)
    b, lb, pb = _stage1(cap, engine=True)
    assert np.isfinite(la).all() and np.isfinite(lb).all() and a.model.last_covered > 0
    assert abs(la[0] - lb[0]) <= 1e-5 * abs(la[0]), (la[0], lb[0])
    rel = lambda x, y: float((x - y).norm() / x.norm().clamp_min(1e-30))
    for k in pa:
        d_te, d_tt = rel(pa[k], pb[k]), rel(pa[k], pa2[k])
        print(f"{k:14s} trainer-vs-executor {d_te:.3g}   trainer-vs-trainer {d_tt:.3g}")
        assert d_te <= 10 * d_tt + 2e-3, k


# -------------------------------------------------------------------------------------------------------------------------------- tool
def test_train_capture_runs_a_dtu_folder(tmp_path):
    from nerf2mesh_amd.capture import Capture
    data, work = str(tmp_path / "scan"), str(tmp_path / "work")
    Capture.synthetic(_poses(), H=H, W=W, intrinsics=_rows()).save_dtu(data)
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "train_capture.py"), data, "--workspace", work, "--data_format", "dtu",
           "--iters0", "60", "--iters1", "20", "--resolution", "64", "--texture", "256", "--eval_views", "2"]
    run = subprocess.run(cmd, capture_output=True, text=True)
    print(run.stdout[-4000:])
    print(run.stderr[-4000:])
    assert run.returncode == 0
    assert os.path.exists(os.path.join(work, "mesh_stage0", "mesh_0.ply"))
    for name in ("mesh_0.obj", "feat0_0.jpg", "feat1_0.jpg", "mlp.json"):
        assert os.path.exists(os.path.join(work, "mesh_stage1", name)), name
    res = json.loads(run.stdout.strip().splitlines()[-1])
    assert res["data_format"] == "dtu" and res["per_view_intrinsics"] and res["train_views"] == V - 1 and res["held_out_views"] == 1
    assert res["held_out_is_test_split"] and (res["H"], res["W"]) == (H, W)
    assert math.isfinite(res["psnr_stage0"]) and math.isfinite(res["psnr_stage1"]) and res["faces"] > 0
