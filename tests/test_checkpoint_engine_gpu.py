"""A resumed stage-0 run is the run that was never interrupted.  Set-up as tests/test_engine.py::_run (six cameras, default ray count,
diffuse_step = 24, 40 steps: the refreshes at 16 and 32, the diffuse -> full switch, six EMA epochs).  Run A: 40 steps.  Run B: k steps,
save_checkpoint.  Run C: a model from another seed, a fresh driver, load_checkpoint, 40 - k steps.  The yardstick comes first: two
uninterrupted runs A and A' -- where they agree bitwise, C must equal A bitwise; where they do not (the autograd trainer), C may differ from
A by 10 x what A' does, plus 2e-4, the rule of tests/test_engine.py, and the sample counts are equal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS = 40
LEGO = dict(diffuse_step=24)
RECIPES = {
    "lego": LEGO,
    "garden": dict(bound=16, dt_gamma=1 / 256, lambda_entropy=1e-3, enable_cam_near_far=True, scene="garden", diffuse_step=24),
    "sdf": dict(sdf=True, iters=120, diffuse_step=24),
    "adaptive": dict(diffuse_step=24, num_points=1 << 15),          # another sample target: the ray count settles elsewhere and keeps moving
}


def _engine():
    from nerf2mesh_amd.engine import Stage0Engine
    return Stage0Engine


def _trainer():
    from nerf2mesh_amd.trainer import Stage0Trainer
    return Stage0Trainer


class Serial:
    """overlap=False: every batch on the main stream."""
    def __new__(cls, *a, **k):
        eng = _engine()(*a, **k)
        eng.overlap = False
        return eng


def _make(cls, model_seed=0, capture=None, **over):
    """A driver in front of its first step (tests/test_engine.py::_run without the steps)."""
    from nerf2mesh_amd import synthetic
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    torch.manual_seed(model_seed)
    kw = dict(O=True, bound=1, dt_gamma=0, iters=30000, fused_mlp=True)
    kw.update(over)
    opt = make_options(**kw)
    model = NeRFNetwork(opt)
    if opt.scene == "garden":
        model.update_aabb(synthetic.pts_aabb("garden"))
    poses = None if capture is not None else synthetic.make_cameras(6, seed=0)
    tr = cls(model, opt, poses, torch.device("cuda", 0), seed=0, capture=capture)
    tr.mark_untrained()
    return tr


def _steps(tr, n):
    """-> per-step (loss, ray count in front of the next batch)."""
    out = []
    for _ in range(n):
        loss = float(tr.train_step())
        out.append((loss, int(tr.num_rays)))
    torch.cuda.synchronize()
    return out


def _snapshot(tr):
    """Everything the issue compares: parameters, both Adam moments, loss scale / step counts / growth tracker, occupancy grid and bit field,
    the EMA shadows, the counters."""
    o = tr.optimizer
    snap = {"scale": o.scale.clone(), "steps": o.steps.clone(), "growth_tracker": o.growth_tracker.clone(),
            "density_grid": tr.model.density_grid.clone(), "density_bitfield": tr.model.density_bitfield.clone()}
    for n, p in tr.model.named_parameters():
        snap["param." + n] = p.detach().clone()
        snap["exp_avg." + n] = o.state[p]["exp_avg"].clone()
        snap["exp_avg_sq." + n] = o.state[p]["exp_avg_sq"].clone()
    for i, s in enumerate(tr.ema.shadow_params):
        snap[f"ema.{i}"] = s.clone()
    counts = {"samples_seen": tr.samples_seen, "rays_seen": tr.rays_seen, "global_step": tr.global_step, "ema_updates": tr.ema.num_updates,
              "lr": [g["lr"] for g in o.param_groups], "last_fold_left": getattr(tr, "last_fold_left", None)}
    return snap, counts


def _rel(p, q):
    p, q = p.double(), q.double()
    return ((p - q).norm() / p.norm().clamp_min(1e-30)).item()


_runs = {}


def _uninterrupted(name, cls, **cfg):
    """Runs A and A' of a recipe, once per module."""
    if name not in _runs:
        pair = []
        for _ in range(2):
            tr = _make(cls, **cfg)
            trace = _steps(tr, STEPS)
            pair.append((_snapshot(tr), trace))
            del tr
        _runs[name] = pair
    return _runs[name]


def _resume(tmp_path, k, cls_save, cls_load, capture=None, **cfg):
    """Runs B and C -> C's snapshot and its per-step trace of steps k + 1 .. 40."""
    from nerf2mesh_amd import checkpoint
    b = _make(cls_save, capture=capture, **cfg)
    _steps(b, k)
    path = checkpoint.save_checkpoint(b, str(tmp_path))
    assert path.endswith(f"ngp_stage0_ep{k // 6:04d}.pth")
    del b
    c = _make(cls_load, model_seed=123, capture=capture, **cfg)          # other initial weights, another device-generator state: a loader that copies nothing is caught
    assert checkpoint.load_checkpoint(c, path) == path and c.global_step == k
    trace = _steps(c, STEPS - k)
    return _snapshot(c), trace


def _compare(name, resumed, a, a2, k, bitwise, same_driver=True):
    """bitwise: the yardstick itself is asserted (A == A' in everything) and C must equal A in everything, bitwise.  Otherwise per entry:
    bitwise where A and A' are, else the fallback rule."""
    (snap_c, cnt_c), trace_c = resumed
    (snap_a, cnt_a), trace_a = a
    (snap_2, cnt_2), trace_2 = a2
    worst = 0.0
    for key in snap_a:
        same = torch.equal(snap_a[key], snap_2[key])
        d_c, d_y = _rel(snap_a[key], snap_c[key]), _rel(snap_a[key], snap_2[key])
        worst = max(worst, d_c)
        if not same or not torch.equal(snap_a[key], snap_c[key]):
            print(f"[{name} k={k}] {key:44s} resumed-vs-A {d_c:.3g}   A'-vs-A {d_y:.3g}")
        if bitwise:
            assert same, f"{key}: two uninterrupted runs differ ({d_y:.3g}): the yardstick does not hold"
        if same:
            assert torch.equal(snap_a[key], snap_c[key]), f"{key}: the resumed run differs from the uninterrupted one by {d_c:.3g} (two uninterrupted runs: bitwise equal)"
        else:
            assert d_c <= 10 * d_y + 2e-4, f"{key}: resumed run {d_c:.3g} from A, two uninterrupted runs {d_y:.3g} apart"
    la, l2, lc = (np.array([t[0] for t in tr]) for tr in (trace_a, trace_2, trace_c))
    if bitwise:
        assert cnt_a == cnt_2 and np.array_equal(la, l2) and trace_a == trace_2, "the yardstick: two uninterrupted runs"
    # sample counts, ray counts after every step, EMA updates, learning rates, step count: equal whatever the arithmetic does
    assert cnt_c["samples_seen"] == cnt_a["samples_seen"] and cnt_c["rays_seen"] == cnt_a["rays_seen"]
    assert cnt_c["global_step"] == STEPS and cnt_c["ema_updates"] == cnt_a["ema_updates"] == STEPS // 6
    assert cnt_c["last_fold_left"] == cnt_a["last_fold_left"] or not np.array_equal(la, l2)
    np.testing.assert_allclose(cnt_c["lr"], cnt_a["lr"], rtol=1e-12)
    if same_driver:           # (the executor rewrites num_rays as it prepares ahead, the trainer a step later: compared within one driver)
        assert [t[1] for t in trace_c] == [t[1] for t in trace_a[k:]], "num_rays after every resumed step"
    if np.array_equal(la, l2) and same_driver:          # (executor and trainer sum the loss in another order: tests/test_engine.py)
        assert np.array_equal(lc, la[k:]), f"per-step losses: {np.abs(lc - la[k:]).max():.3g}"
    else:
        noise = np.abs(la - l2)[k:]
        assert (np.abs(lc - la[k:]) <= 10 * noise.max() + 2e-4 * np.abs(la[k:])).all()
    return worst


@pytest.mark.parametrize("k", [16, 17, 23])
def test_resumed_engine_is_the_uninterrupted_engine(tmp_path, k):
    """k = 16: the next batch waits for a refresh (already run when the checkpoint is taken); 17: the batch behind it is the deferred
    mid-step one; 23: a generic step, the last of the diffuse phase."""
    a, a2 = _uninterrupted("lego", _engine(), **LEGO)
    _compare("lego", _resume(tmp_path, k, _engine(), _engine(), **LEGO), a, a2, k, bitwise=True)


@pytest.mark.parametrize("recipe", ["garden", "sdf", "adaptive"])
def test_resumed_engine_other_recipes(tmp_path, recipe):
    """The outdoor recipe (entropy loss, cam_near_far, mark_untrained: the cells it set to -1 ride in density_grid), the SDF recipe (variance,
    progressive levels, fold state), and a sample target that moves the ray count."""
    cfg, k = RECIPES[recipe], 17
    a, a2 = _uninterrupted(recipe, _engine(), **cfg)
    if recipe == "garden":
        grid = a[0][0]["density_grid"]
        assert bool((grid < 0).any()), "mark_untrained has marked cells"
    if recipe == "adaptive":
        rays = [t[1] for t in a[1]]
        assert len(set(rays[17:])) > 3, "the ray count moves after the checkpoint too"
    resumed = _resume(tmp_path, k, _engine(), _engine(), **cfg)
    _compare(recipe, resumed, a, a2, k, bitwise=False)
    if recipe == "garden":
        assert torch.equal(resumed[0][0]["density_grid"] < 0, a[0][0]["density_grid"] < 0), "the marked cells survive"


def test_resumed_serial_engine(tmp_path):
    """overlap=False: the pipeline prepares every batch on the main stream; the same run."""
    a, a2 = _uninterrupted("lego-serial", Serial, **LEGO)
    _compare("serial", _resume(tmp_path, 17, Serial, Serial, **LEGO), a, a2, 17, bitwise=True)


def test_resumed_trainer_and_the_two_drivers_exchange_checkpoints(tmp_path):
    """The autograd trainer is not bit-reproducible: the fallback rule against two uninterrupted trainer runs.  An engine checkpoint
    continues in a trainer and a trainer checkpoint in an engine within the same rule."""
    a, a2 = _uninterrupted("lego-trainer", _trainer(), **LEGO)
    k = 17
    for name, save, load in (("trainer", _trainer(), _trainer()), ("engine->trainer", _engine(), _trainer()), ("trainer->engine", _trainer(), _engine())):
        where = tmp_path / name.replace("->", "_")
        where.mkdir()
        _compare(name, _resume(where, k, save, load, **LEGO), a, a2, k, bitwise=False, same_driver=load is _trainer())


# ---------------------------------------------------------------------------------------------------------------- captures
INTR = (70.0, 60.0, 30.5, 25.25)


@pytest.fixture(scope="module")
def small_capture():
    """The smallest synthetic capture of tests/test_capture_engine_gpu.py (six views, 48 x 64) with a sparse-depth table of its own: 40 to 90
    keypoints per view at the depth of the scene's centre."""
    from nerf2mesh_amd import synthetic
    from nerf2mesh_amd.capture import Capture, SparseDepth
    poses = synthetic.make_cameras(6, seed=0)
    cap = Capture.synthetic(poses, H=48, W=64, intrinsics=INTR, alpha=True, device="cuda")
    g = torch.Generator().manual_seed(5)
    counts = [40, 90, 55, 70, 64, 48]
    off = np.concatenate([[0], np.cumsum(counts)])
    K = int(off[-1])
    coords = torch.stack([torch.randint(0, 48, (K,), generator=g), torch.randint(0, 64, (K,), generator=g)], 1)
    dist = torch.repeat_interleave(poses[:, :3, 3].norm(dim=1), torch.tensor(counts))
    cap.sparse_depth = SparseDepth(off, coords, dist * (0.9 + 0.2 * torch.rand(K, generator=g)), 0.5 + torch.rand(K, generator=g), device="cuda")
    return cap


def test_depth_schedule_position_resumes(tmp_path, small_capture):
    """Sparse depth: one batch in ten is a depth batch on a view the schedule draws -- two batches ahead of the running step.  The checkpoint
    is taken between two depth batches, with a decision already drawn for a batch that has not run."""
    from nerf2mesh_amd.capture import DepthSchedule
    cfg = dict(diffuse_step=24, enable_sparse_depth=True)
    log = DepthSchedule(6, 0)
    for _ in range(STEPS + 2):
        log.next()
    depth_steps = [i + 1 for i, v in enumerate(log.log[:STEPS]) if v is not None]
    assert len(depth_steps) >= 2, depth_steps
    # k: behind the first depth step, and -- where the schedule leaves room -- with the second one already prepared in the queue (batch k + 2)
    k = max(depth_steps[0], depth_steps[1] - 2)
    a, a2 = _uninterrupted("depth", _engine(), capture=small_capture, **cfg)
    b = _make(_engine(), capture=small_capture, **cfg)
    _steps(b, k)
    assert len(b.depth_schedule.log) == k + 2, "the schedule is two decisions ahead of the step"
    sd = b.state_dict()
    assert sd["n2m"]["batches"]["depth_schedule"]["position"] == k
    del b, sd
    resumed = _resume(tmp_path, k, _engine(), _engine(), capture=small_capture, **cfg)
    _compare("depth", resumed, a, a2, k, bitwise=False)
    assert resumed[0][1]["rays_seen"] == a[0][1]["rays_seen"], "the same depth batches (their ray count is their view's keypoint count)"


def test_appearance_codes_resume_bitwise(tmp_path, small_capture):
    cfg = dict(diffuse_step=24, ind_dim=4, ind_num=8)
    a, a2 = _uninterrupted("ind", _engine(), capture=small_capture, **cfg)
    assert "param.individual_codes" in a[0][0] and float(a[0][0]["exp_avg_sq.individual_codes"].abs().sum()) > 0
    _compare("ind", _resume(tmp_path, 17, _engine(), _engine(), capture=small_capture, **cfg), a, a2, 17, bitwise=True)


# ------------------------------------------------------------------------------------------------------------- interchange
def test_file_loads_into_torch_adam_and_gradscaler_and_back(tmp_path):
    """The `optimizer` and `scaler` entries are torch.optim.Adam's and torch.amp.GradScaler's own forms: a real pair built over the same
    parameters takes them, and what that pair saves goes back into FusedAdamAMP -- one step from both sides gives the same parameters
    (tolerances: tests/test_optim.py::test_fused_adam_amp_matches_torch_adam_and_gradscaler)."""
    from nerf2mesh_amd import checkpoint
    from nerf2mesh_amd.optim import FusedAdamAMP
    eng = _make(_engine(), **LEGO)
    _steps(eng, 26)                                                  # the specular head joined at step 24: its step counts are 3, the others' 26
    path = checkpoint.save_checkpoint(eng, str(tmp_path), full=True)
    sd = torch.load(path, map_location="cuda", weights_only=True)
    params = [p for g in eng.optimizer.param_groups for p in g["params"]]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in params]
    it = iter(ref)
    adam = torch.optim.Adam([{"params": [next(it) for _ in g["params"]], "lr": g["lr"]} for g in eng.optimizer.param_groups], eps=1e-15)
    scaler = torch.amp.GradScaler("cuda")
    adam.load_state_dict(sd["optimizer"])
    scaler.load_state_dict(sd["scaler"])
    assert sd["optimizer"]["state"][0]["step"].ndim == 0 and set(sd["scaler"]) == {"scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"}
    scaler.scale(torch.zeros((), device="cuda"))                     # (the scaler builds its device state on first use)
    o = eng.optimizer
    assert scaler.get_scale() == float(o.scale) and int(scaler._get_growth_tracker()) == int(o.growth_tracker)
    steps = [float(adam.state[q]["step"]) for q in ref]
    assert steps == [float(o.steps[o._slot[p]]) for p in params] and max(steps) == float(o.steps[0]) > 3 and min(steps) == 3
    for p, q in zip(params, ref):
        assert torch.equal(adam.state[q]["exp_avg"], o.state[p]["exp_avg"]) and torch.equal(adam.state[q]["exp_avg_sq"], o.state[p]["exp_avg_sq"])
    for g, h in zip(adam.param_groups, o.param_groups):
        assert g["lr"] == h["lr"] and g["initial_lr"] == h["initial_lr"]
    # ... and back: the pair's own state into a fresh FusedAdamAMP over the same values, one step of the same gradients from both sides
    mine = [torch.nn.Parameter(p.detach().clone()) for p in params]
    it = iter(mine)
    fused = FusedAdamAMP([{"params": [next(it) for _ in g["params"]], "lr": g["lr"]} for g in o.param_groups], eps=1e-15, amp=True)
    fused.load_state_dict(checkpoint.adam_from_torch(adam.state_dict(), scaler.state_dict()))
    assert all(fused.state[p]["exp_avg"].data_ptr() != adam.state[q]["exp_avg"].data_ptr() for p, q in zip(mine, ref)), "the moments are copies"
    assert float(fused.scale) == scaler.get_scale() and float(fused.growth_tracker) == int(o.growth_tracker)
    assert [float(fused.steps[fused._slot[p]]) for p in mine] == steps
    gen = torch.Generator(device="cuda").manual_seed(7)
    for p, q in zip(mine, ref):
        g = torch.randn(p.shape, device="cuda", generator=gen) * 1e-3
        q.grad = g * scaler.get_scale()
        p.grad = g * float(fused.scale)
    scaler.step(adam)
    scaler.update()
    fused.step()
    torch.cuda.synchronize()
    for p, q in zip(mine, ref):
        np.testing.assert_allclose(p.detach().cpu().numpy(), q.detach().cpu().numpy(), rtol=2e-5, atol=2e-6)
        np.testing.assert_allclose(fused.state[p]["exp_avg"].cpu().numpy(), adam.state[q]["exp_avg"].cpu().numpy(), rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(fused.state[p]["exp_avg_sq"].cpu().numpy(), adam.state[q]["exp_avg_sq"].cpu().numpy(), rtol=1e-5, atol=1e-9)


def test_mismatched_options_raise_and_name_the_key(tmp_path):
    from nerf2mesh_amd import checkpoint
    eng = _make(_engine(), **LEGO)
    _steps(eng, 2)
    path = checkpoint.save_checkpoint(eng, str(tmp_path))
    other = _make(_engine(), bound=2, dt_gamma=1 / 256, **LEGO)     # two cascades: another occupancy grid
    with pytest.raises(RuntimeError, match="density_grid"):
        checkpoint.load_checkpoint(other, path)
