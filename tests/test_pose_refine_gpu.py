"""GPU: pose refinement in trainer.Stage0Trainer (options.optimize_poses) on the smallest synthetic capture of
tests/test_capture_engine_gpu.py (six views, 48 x 64), fp32, 1024 rays per batch.

(5) one step's delta.grad is the float64 model of tests/pose_ref.py on the step's own grad_xyzs / grad_dirs, and the torch statement in the
kernels' place agrees; (6) nothing changes with the option off, and nothing moves at lr_pose = 0; (7) on a frozen, trained field, pose-only
steps from perturbed poses lower the loss and the pose errors; (8) a resumed run continues."""
import copy
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pose_ref as R   # noqa: E402
from test_capture_engine_gpu import small_captures   # noqa: E402,F401  (the fixture: {alpha: Capture}, six views 48 x 64)
from test_checkpoint_engine_gpu import small_capture   # noqa: E402,F401  (the same set with a sparse-depth table)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
RAYS = 1024


@pytest.fixture(scope="module")
def cap(small_captures):   # noqa: F811
    return small_captures[True]


def _trainer(capture, model_seed=0, model=None, **over):
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    from nerf2mesh_amd.trainer import Stage0Trainer
    torch.manual_seed(model_seed)
    kw = dict(bound=1, dt_gamma=0, iters=30000, fp16=False, num_rays=RAYS, optimize_poses=True)
    kw.update(over)
    opt = make_options(**kw)
    tr = Stage0Trainer(model if model is not None else NeRFNetwork(opt), opt, None, torch.device("cuda", 0), seed=0, capture=capture)
    torch.manual_seed(1)                     # the march jitter of an unpipelined step comes from the device generator
    return tr


def _spy(tr, attach):
    """Routes the renderer's hook through `attach` and keeps what went in and what came back."""
    seen = {}

    def hook(xyzs, dirs, ts, rays, rays_d, index):
        seen.update(ts=ts, rays=rays, rays_d=rays_d, view=index)
        x, d = attach(xyzs, dirs, ts, rays, rays_d, index)
        x.register_hook(lambda g: seen.__setitem__("grad_xyzs", g.detach().clone()))
        d.register_hook(lambda g: seen.__setitem__("grad_dirs", g.detach().clone()))
        return x, d
    tr.model.ray_attach = hook
    return seen


# ------------------------------------------------------------------------------------------------------------------- (5) chain
@pytest.fixture(scope="module")
def chain(cap):
    from nerf2mesh_amd.pose_refine import attach_torch
    a = _trainer(cap, diffuse_step=0)                       # full shading from the first step: the directions carry a gradient
    seen = _spy(a, a.refiner.attach)
    loss = float(a.train_step().detach())
    b = _trainer(cap, diffuse_step=0)
    seen_b = _spy(b, lambda x, d, ts, rays, rays_d, view: attach_torch(x, d, b.refiner.delta, ts, rays, rays_d, view))
    loss_b = float(b.train_step().detach())
    return dict(a=a, seen=seen, loss=loss, grad=a.refiner.delta.grad.detach().cpu().numpy().astype(np.float64),
                grad_torch=b.refiner.delta.grad.detach().cpu().numpy().astype(np.float64), loss_b=loss_b, seen_b=seen_b)


def _model_and_bound(seen, V):
    n = lambda t: t.detach().cpu().numpy()
    rays, view = n(seen["rays"]), n(seen["view"])
    r6, S_ray = R.ray_grad(n(seen["grad_xyzs"]), n(seen["grad_dirs"]), n(seen["ts"]), rays, n(seen["rays_d"]))
    b_ray = (rays[:, 1:2].astype(np.float64) + 8) * U * S_ray                # test 2's bound, per ray
    want, S, count = R.view_grad(r6, view, np.zeros((V, 6)))
    bound = (count[:, None] + 8) * U * S                                     # test 3's bound (J_l = I at delta = 0) ...
    for v in range(V):                                                       # ... plus what the rays' own errors add up to
        carried = b_ray[view == v].sum(0)
        bound[v, 3:] += carried[:3]
        bound[v, :3] += carried[3:].sum()
    return want, bound, count


def test_delta_grad_is_the_model_on_the_steps_own_gradients(chain, cap):
    seen = chain["seen"]
    assert seen["grad_xyzs"].shape == seen["grad_dirs"].shape and seen["grad_xyzs"].shape[1] == 3 and seen["view"].shape == (RAYS,)
    assert float(seen["grad_xyzs"].abs().max()) > 0 and float(seen["grad_dirs"].abs().max()) > 0
    want, bound, count = _model_and_bound(seen, len(cap))
    err = np.abs(chain["grad"] - want)
    print("delta.grad against the float64 model: largest |gradient| %.3g, error / bound per view %s, rays per view %s"
          % (np.abs(want).max(), (err / bound).max(1), count.tolist()))
    assert math.isfinite(chain["loss"]) and np.abs(want).max() > 0 and (count > 0).all()
    assert (err <= bound).all()


def test_the_torch_statement_agrees(chain, cap):
    assert chain["loss_b"] == chain["loss"]                                  # the same step
    assert torch.equal(chain["seen_b"]["grad_xyzs"], chain["seen"]["grad_xyzs"])
    want, bound, _ = _model_and_bound(chain["seen"], len(cap))
    err = np.abs(chain["grad_torch"] - want)
    print("attach_torch in the kernels' place: error / (2 x bound) per view", (err / (2 * bound)).max(1))
    assert (err <= 2 * bound).all()


# --------------------------------------------------------------------------------------------------------- (6) no behaviour change
def _fast(capture, **over):
    return _trainer(capture, O=True, fp16=True, fused_mlp=True, optimize_poses=False, num_rays=RAYS, **over)


def test_with_the_option_off_a_step_is_what_it_was(cap):
    """Two trainers on the fused field, one whose model never saw the hook attribute assigned after construction, one that had it set and
    cleared again: losses and parameters agree bitwise over three steps."""
    ends = []
    for touch in (False, True):
        tr = _fast(cap)
        tr.mark_untrained()
        if touch:
            tr.model.ray_attach = lambda *a: a[:2]
            tr.model.ray_attach = None
        assert tr.refiner is None and tr.pipeline is True and tr._index is None
        losses = [float(tr.train_step().detach()) for _ in range(3)]
        ends.append((losses, [p.detach().clone() for p in tr.model.parameters()]))
    assert ends[0][0] == ends[1][0]
    for p, q in zip(ends[0][1], ends[1][1]):
        assert torch.equal(p, q)


def test_at_lr_pose_zero_the_poses_keep_their_bits(cap):
    tr = _trainer(cap, lr_pose=0.0)
    for _ in range(8):
        assert math.isfinite(float(tr.train_step().detach()))
    assert tr.poses is tr.refiner.poses() and torch.equal(tr.poses.view(torch.int32), cap.poses.view(torch.int32))
    assert float(tr.refiner.delta.detach().abs().max()) == 0 and float(tr.refiner.delta.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------ (7) it refines
STEPS_FIELD, STEPS_POSE = 400, 200


def _perturbed(capture, seed=7):
    """Every view turned by 1 degree about a random axis through its centre and shifted by 1 % of the camera radius."""
    g = np.random.default_rng(seed)
    poses = capture.poses.cpu().numpy().astype(np.float64)
    radius = float(np.linalg.norm(poses[:, :3, 3], axis=1).mean())
    out = poses.copy()
    for v in range(len(poses)):
        axis, shift = g.normal(size=3), g.normal(size=3)
        out[v, :3, :3] = R.rotation(axis / np.linalg.norm(axis) * math.radians(1.0)) @ poses[v, :3, :3]
        out[v, :3, 3] += shift / np.linalg.norm(shift) * 0.01 * radius
    bad = copy.copy(capture)
    bad.poses = torch.from_numpy(out).float().cuda()
    return bad


def _pose_errors(poses, true):
    """(mean rotation error in degrees, mean translation error)."""
    p, t = poses.detach().cpu().numpy().astype(np.float64), true.detach().cpu().numpy().astype(np.float64)
    cos = (np.einsum("vij,vij->v", p[:, :3, :3], t[:, :3, :3]) - 1) / 2
    return float(np.degrees(np.arccos(np.clip(cos, -1, 1))).mean()), float(np.linalg.norm(p[:, :3, 3] - t[:, :3, 3], axis=1).mean())


def _eval_loss(tr, capture, us):
    """Mean photometric loss of the frozen field over fixed batches drawn from the pose table the trainer holds now (no march jitter)."""
    from nerf2mesh_amd.capture import batch_from_uniforms_u8, batch_views
    from nerf2mesh_amd.losses import photo_loss
    model, opt = tr.model, tr.opt
    model.train()
    total = 0.0
    with torch.no_grad():
        for u in us:
            o, d, rgba, nears, fars, _, bg = batch_from_uniforms_u8(tr.poses, capture.bank, capture.lut, u, model.aabb_train, model.min_near, capture.H,
                                                                    capture.W, capture.intrinsics)
            out = model.render(o, d, index=batch_views(u, len(capture)), bg_color=bg, perturb=False, shading="diffuse", dt_gamma=opt.dt_gamma,
                               max_steps=opt.max_steps, blend_bg=False, nears_fars=(nears, fars))
            total += float(photo_loss(out["image"], out["weights_sum"], rgba, bg, opt.lambda_rgb, tr._lambda_mask()))
    return total / len(us)


@pytest.fixture(scope="module")
def refined(cap):
    from nerf2mesh_amd.engine import Stage0Engine
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    torch.manual_seed(0)
    opt = make_options(O=True, bound=1, dt_gamma=0, iters=30000, fused_mlp=True)
    eng = Stage0Engine(NeRFNetwork(opt), opt, None, torch.device("cuda", 0), seed=0, capture=cap)        # the fast path, the true poses
    eng.mark_untrained()
    for _ in range(STEPS_FIELD):
        eng.train_step()
    if hasattr(eng, "sync_parameters"):
        eng.sync_parameters()
    state, mean_density = {k: v.detach().clone() for k, v in eng.model.state_dict().items()}, eng.model.mean_density
    bad = _perturbed(cap)
    gen = torch.Generator(device="cuda").manual_seed(99)
    us = [torch.rand(RAYS, 6, device="cuda", generator=gen) for _ in range(16)]
    runs = {}
    for name, lr_pose in (("refine", None), ("control", 0.0)):
        over = {} if lr_pose is None else dict(lr_pose=lr_pose)
        tr = _trainer(bad, lr=0.0, **over)                                   # lr = 0: the field is frozen
        tr.model.load_state_dict(state)
        tr.model.mean_density = mean_density
        tr._refreshed = 1 << 30                                              # no occupancy refresh either: the field's grid stays as trained
        frozen = [p.detach().clone() for p in tr.model.parameters()]
        before = (_eval_loss(tr, bad, us),) + _pose_errors(tr.poses, cap.poses)
        for _ in range(STEPS_POSE):
            tr.train_step()
        after = (_eval_loss(tr, bad, us),) + _pose_errors(tr.poses, cap.poses)
        assert all(torch.equal(p, q) for p, q in zip(frozen, tr.model.parameters()))
        runs[name] = (before, after, tr.opt.lr_pose)
    return runs


def test_pose_only_steps_lower_the_loss(refined):
    (l0, r0, t0), (l1, r1, t1), lr_pose = refined["refine"]
    print(f"lr_pose {lr_pose:g}, {STEPS_POSE} pose-only steps: loss {l0:.6g} -> {l1:.6g} (ratio {l1 / l0:.3f}); rotation error {r0:.4f} -> {r1:.4f} deg "
          f"(ratio {r1 / r0:.3f}); translation error {t0:.5f} -> {t1:.5f} (ratio {t1 / t0:.3f})")
    assert l1 < l0
    (c0, cr0, ct0), (c1, cr1, ct1), _ = refined["control"]
    print(f"control (lr_pose 0): loss {c0:.6g} -> {c1:.6g}")
    assert c0 == l0 and c1 == c0 and (cr0, ct0) == (cr1, ct1) == (r0, t0)


def test_pose_only_steps_lower_the_pose_errors(refined):
    (_, r0, t0), (_, r1, t1), _ = refined["refine"]
    assert abs(r0 - 1.0) < 1e-3                                              # the perturbation is the one stated
    assert r1 < r0 and t1 < t0


# ------------------------------------------------------------------------------------------------------------------ (8) checkpoint
def test_a_resumed_run_continues(cap, tmp_path):
    """Runs A and A' of 8 steps, run B of 4 steps whose checkpoint FILE a fresh driver (other initial weights) loads for 4 more.  The rule of
    tests/test_checkpoint_engine_gpu.py: where A and A' agree bitwise the resumed run equals A bitwise; where they do not (the position
    gradient's table backward adds with atomics), it may differ from A by 10 x what A' does plus 2e-4 -- of the loss for the loss, and of
    the distance the corrections have travelled (max |delta|, a few 1e-5 after 8 warm-up steps) for delta and the poses, so that a run
    whose Adam moments or schedule were not restored (its steps 5 .. 8 would restart at 1 % of lr_pose with fresh moments: tens of per cent
    of that distance) does not pass."""
    from nerf2mesh_amd import checkpoint

    def run(tr, n):
        return [float(tr.train_step().detach()) for _ in range(n)]

    def end(tr, losses):
        return dict(delta=tr.refiner.delta.detach().clone(), poses=tr.poses.clone(), loss=torch.tensor(losses[-1]))
    ends = []
    for _ in range(2):
        tr = _trainer(cap)
        ends.append(end(tr, run(tr, 8)))
    b = _trainer(cap, workspace=str(tmp_path))
    run(b, 4)
    path = checkpoint.save_checkpoint(b, str(tmp_path))
    c = _trainer(cap, model_seed=123, workspace=str(tmp_path))
    assert checkpoint.load_checkpoint(c, path) == path
    assert c.global_step == 4 and torch.equal(c.refiner.delta, b.refiner.delta) and torch.equal(c.poses, b.poses) and c.poses is c.refiner.poses()
    assert c.refiner.scheduler.last_epoch == 4 and c.refiner.optimizer.param_groups[0]["lr"] == b.refiner.optimizer.param_groups[0]["lr"]
    sb, sc = (t.refiner.optimizer.state[t.refiner.delta] for t in (b, c))
    assert torch.equal(sb["exp_avg"], sc["exp_avg"]) and torch.equal(sb["exp_avg_sq"], sc["exp_avg_sq"]) and float(sb["step"]) == float(sc["step"]) == 4
    resumed = end(c, run(c, 4))
    a, a2 = ends
    travelled = float(a["delta"].abs().max())
    assert travelled > 1e-5 and float((a["delta"] - b.refiner.delta.detach()).abs().max()) > 0.2 * travelled      # steps 5 .. 8 matter
    scale = {"delta": travelled, "poses": travelled, "loss": 1.0}
    for k in ("delta", "poses", "loss"):
        if torch.equal(a[k], a2[k]):
            assert torch.equal(resumed[k], a[k]), k
        else:
            noise, diff = float((a[k] - a2[k]).abs().max()), float((resumed[k] - a[k]).abs().max())
            print(f"{k}: two uninterrupted runs differ by {noise:.3g}; the resumed run differs by {diff:.3g} (allowed {10 * noise + 2e-4 * scale[k]:.3g})")
            assert diff <= 10 * noise + 2e-4 * scale[k], k
    plain = _trainer(cap, optimize_poses=False)
    with pytest.raises(ValueError, match="disagree on optimize_poses"):
        checkpoint.load_checkpoint(plain, path)


# --------------------------------------------------------------------------------------------------- the combinations that keep working
def _moves(tr, steps=2):
    """`steps` steps (up to four more while a loss scaler is still backing off from its first value and skips them): finite losses, a
    finite non-zero delta.grad, and corrections that have left zero."""
    for k in range(steps + 4):
        assert math.isfinite(float(tr.train_step().detach()))
        if k + 1 >= steps and float(tr.refiner.delta.detach().abs().max()) > 0:
            break
    g = tr.refiner.delta.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert float(tr.refiner.delta.detach().abs().max()) > 0 and not torch.equal(tr.poses, tr.refiner.poses0)
    return tr


def test_the_executor_steps_aside(cap):
    from nerf2mesh_amd.engine import Stage0Engine
    off = _fast(cap)
    assert Stage0Engine.supported(off.model, off.opt, capture=cap) is True
    off.opt.optimize_poses = True
    assert Stage0Engine.supported(off.model, off.opt, capture=cap) is False


def test_half_precision_and_a_contracted_scene(cap):
    """The tools' recipe (-O: fp16 and the loss scaler, one verdict for both optimizers through JointStep) on a contracted scene: the
    marcher hands out contracted samples and n2m_pose_ray_grad takes their gradients back through the contraction."""
    tr = _trainer(cap, O=True, fp16=True, bound=4, dt_gamma=1 / 256, contract=True)
    assert tr.scaler.is_enabled() and tr.refiner.contract and tr.opt.contract
    _moves(tr)
    assert float(tr.scaler.get_scale()) > 0


def test_a_skipped_step_skips_both_optimizers(cap):
    """An inf in the field's gradient: the scaler's one verdict leaves the corrections where they are as well."""
    tr = _trainer(cap, O=True, fp16=True)
    _moves(tr, 1)
    before, scale = tr.refiner.delta.detach().clone(), float(tr.scaler.get_scale())
    p = next(tr.model.sigma_net.parameters())
    handle = p.register_hook(lambda g: torch.full_like(g, float("inf")))
    tr.train_step()
    handle.remove()
    assert torch.equal(tr.refiner.delta.detach(), before) and float(tr.scaler.get_scale()) < scale


@pytest.mark.parametrize("over", [dict(patch_size=16), dict(ind_dim=8, ind_num=8), dict(lambda_distort=0.01), dict(enable_dense_depth=True)],
                         ids=["patch", "ind_dim", "lambda_distort", "dense_depth"])
def test_batch_kinds_and_terms_that_keep_working(cap, over):
    capture = cap
    if over.get("enable_dense_depth"):
        capture = copy.copy(cap)
        capture.dense_depth = torch.full((len(cap), cap.H * cap.W), 1.3, device="cuda")
    _moves(_trainer(capture, **over))


def test_sparse_depth_steps_name_one_view(small_capture):   # noqa: F811
    """One step in ten takes the keypoints of ONE view: the view index of such a batch is that view for every ray, and only that view's
    correction receives a gradient."""
    tr = _trainer(small_capture, enable_sparse_depth=True)
    seen = 0
    for _ in range(12):
        tr.train_step()
        view = tr.depth_schedule.log[tr.global_step - 1]                     # unpipelined: batch k is drawn in step k
        if view is not None:
            g = tr.refiner.delta.grad
            others = [v for v in range(len(small_capture)) if v != view]
            assert float(g[view].abs().max()) > 0 and float(g[others].abs().max()) == 0
            seen += 1
    assert seen >= 1


# ------------------------------------------------------------------------------------------------------------------- the front end
def test_train_capture_refines_and_writes_the_poses(tmp_path):
    """tools/train_capture.py PATH --optimize_poses on a synthetic capture written to disk: both stages run, WORKSPACE/poses_refined.npy
    holds a [V,4,4] table that differs from the stored poses, and the note on held-out views is printed once."""
    import subprocess
    from nerf2mesh_amd import synthetic
    from nerf2mesh_amd.capture import Capture
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    intr = (70.0, 60.0, 30.5, 25.25)
    data, work = str(tmp_path / "set"), str(tmp_path / "work")
    train = Capture.synthetic(synthetic.make_cameras(6, seed=0), H=48, W=64, intrinsics=intr)
    train.save_nerf(data, split="train")
    Capture.synthetic(synthetic.make_cameras(2, seed=1), H=48, W=64, intrinsics=intr).save_nerf(data, split="test")
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(root, "tools", "train_capture.py"), data, "--workspace", work, "--scale", "1",
           "--iters0", "300", "--iters1", "20", "--texture", "512", "--decimate_target", "20000", "--optimize_poses", "--lr_pose", "1e-3"]
    run = subprocess.run(cmd, capture_output=True, text=True)
    print(run.stdout[-3000:])
    print(run.stderr[-3000:])
    assert run.returncode == 0
    poses = np.load(os.path.join(work, "poses_refined.npy"))
    assert poses.shape == (6, 4, 4) and poses.dtype == np.float32 and np.isfinite(poses).all()
    moved = np.abs(poses - train.poses.cpu().numpy()).max()
    assert 0 < moved < 0.2
    assert run.stdout.count("held-out views are evaluated with their stored poses") == 1 and "(Stage0Trainer)" in run.stdout
    assert os.path.exists(os.path.join(work, "mesh_stage1", "mesh_0.obj"))
