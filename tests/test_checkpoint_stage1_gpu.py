"""Stage-1 checkpoints on the small mesh and the views of tests/stage1_case.py (1500 faces, 64 x 64, ssaa 2): 6 steps against 3 + save + a
fresh trainer + load + 3, for trainer.Stage1Trainer and engine_stage1.Stage1Engine; a checkpoint taken after refine_mesh() into a trainer built
on the original mesh; stage 1 started from a workspace that holds a stage-0 file only.  Yardstick first, as in
tests/test_checkpoint_engine_gpu.py: bitwise where two uninterrupted runs are bitwise, else 10 x their distance + 2e-4."""
import pytest
import torch

pytestmark = pytest.mark.gpu

STEPS, K = 6, 3


def _make(model_seed=0, mesh=None, refine=False, workspace=None):
    import render_case as RC
    import stage1_case as SC
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    from nerf2mesh_amd.trainer import Stage1Trainer
    torch.manual_seed(model_seed)
    opt = make_options(O=True, bound=1, dt_gamma=0, stage=1, fused_mlp=True, **({"workspace": str(workspace)} if workspace else {}))
    opt.refine = bool(refine)
    v, f = mesh if mesh is not None else (torch.from_numpy(x) for x in SC.mesh())
    poses, _ = RC.cameras()
    tr = Stage1Trainer(NeRFNetwork(opt), opt, poses[:6], v, f, torch.device("cuda", 0), H=SC.H0, W=SC.W0, seed=0)
    for _ in range(500):                                             # behind the warm-up: the learning rate is the full one
        tr.scheduler.step()
    return tr


def _driver(tr, kind):
    from nerf2mesh_amd.engine_stage1 import Stage1Engine
    if kind == "trainer":
        return tr
    assert Stage1Engine.supported(tr)
    return Stage1Engine(tr)


def _snapshot(tr):
    m, o = tr.model, tr.optimizer
    snap = {"scale": o.scale.clone(), "steps": o.steps.clone(), "growth_tracker": o.growth_tracker.clone(), "vertices": m.vertices.clone(),
            "triangles": m.triangles.clone(), "triangles_errors": m.triangles_errors.clone(), "triangles_errors_cnt": m.triangles_errors_cnt.clone()}
    for n, p in m.named_parameters():
        snap["param." + n] = p.detach().clone()
        snap["exp_avg." + n] = o.state[p]["exp_avg"].clone()
        snap["exp_avg_sq." + n] = o.state[p]["exp_avg_sq"].clone()
    return snap, {"global_step": tr.global_step, "covered_seen": tr.covered_seen, "last_epoch": tr.scheduler.last_epoch,
                  "lr": [g["lr"] for g in o.param_groups]}


def _rel(p, q):
    p, q = p.double(), q.double()
    return ((p - q).norm() / p.norm().clamp_min(1e-30)).item()


def _run(kind, steps, refine=False):
    tr = _make(refine=refine)
    d = _driver(tr, kind)
    losses = [float(d.train_step()) for _ in range(steps)]
    torch.cuda.synchronize()
    return tr, d, losses


@pytest.mark.parametrize("kind", ["trainer", "engine"])
def test_resumed_stage1_is_the_uninterrupted_run(tmp_path, kind):
    from nerf2mesh_amd import checkpoint
    # the yardstick: three uninterrupted runs (float atomics in the raster / antialias backward and in the error accumulators: an entry
    # counts as reproducible only if all three agree on it)
    (a, _, la), (a2, _, la2), (a3, _, la3) = (_run(kind, STEPS, refine=True) for _ in range(3))
    b, db, _ = _run(kind, K, refine=True)
    path = checkpoint.save_checkpoint(db, str(tmp_path))
    assert path.endswith("ngp_stage1_ep0000.pth")
    c = _make(model_seed=123, refine=True)
    dc = _driver(c, kind)
    assert checkpoint.load_checkpoint(dc, path) == path and c.global_step == K
    lc = [float(dc.train_step()) for _ in range(STEPS - K)]
    torch.cuda.synchronize()
    c = getattr(dc, "tr", dc)
    (sa, ca), (s2, c2), (s3, _), (sc, cc) = _snapshot(a), _snapshot(a2), _snapshot(a3), _snapshot(c)
    failed, all_same = [], True
    for key in sa:
        same = torch.equal(sa[key], s2[key]) and torch.equal(sa[key], s3[key])
        all_same = all_same and same
        d_c, d_y = _rel(sa[key], sc[key]), max(_rel(sa[key], s2[key]), _rel(sa[key], s3[key]))
        if not same or d_c > 0:
            print(f"[{kind}] {key:40s} resumed-vs-A {d_c:.3g}   uninterrupted-vs-A {d_y:.3g}")
        if same and not torch.equal(sa[key], sc[key]):
            failed.append(f"{key}: resumed run differs by {d_c:.3g}, three uninterrupted runs are bitwise equal")
        elif not same and not d_c <= 10 * d_y + 2e-4:
            failed.append(f"{key}: resumed run {d_c:.3g} from A, uninterrupted runs {d_y:.3g} apart")
    assert not failed, failed
    assert cc["global_step"] == STEPS and cc["last_epoch"] == ca["last_epoch"] == 500 + STEPS and cc["lr"] == ca["lr"]
    if ca["covered_seen"] == c2["covered_seen"]:
        assert cc["covered_seen"] == ca["covered_seen"]
    for x, y, z in zip(la[K:], la2[K:], lc):
        assert abs(z - x) <= 10 * abs(y - x) + 2e-4 * abs(x), (la, la2, lc)
    if all_same and la == la2 == la3:
        assert lc == la[K:], "the same views on the same backgrounds (the trainer's generator resumes)"


def test_checkpoint_after_refinement_loads_into_a_trainer_on_the_original_mesh(tmp_path):
    from nerf2mesh_amd import checkpoint
    b, _, _ = _run("trainer", 6, refine=True)                        # every view once: the error accumulators cover the mesh
    before = (b.model.vertices.shape[0], b.model.triangles.shape[0])
    b.refine_mesh()
    after = (b.model.vertices.shape[0], b.model.triangles.shape[0])
    assert after != before, "the refinement changed the mesh"
    for _ in range(2):
        b.train_step()
    torch.cuda.synchronize()
    path = checkpoint.save_checkpoint(b, str(tmp_path))
    c = _make(model_seed=123, refine=True)
    assert (c.model.vertices.shape[0], c.model.triangles.shape[0]) == before
    old_optimizer = c.optimizer
    checkpoint.load_checkpoint(c, path)
    (sb, cb), (sc, cc) = _snapshot(b), _snapshot(c)
    assert (c.model.vertices.shape[0], c.model.triangles.shape[0]) == after and c.optimizer is not old_optimizer
    assert sb.keys() == sc.keys() and cb == cc
    for key in sb:
        assert torch.equal(sb[key], sc[key]), key
    assert c.model.vertices_offsets.shape == c.model.vertices.shape and float(sc["param.vertices_offsets"].abs().sum()) > 0
    assert float(sc["triangles_errors_cnt"].sum()) > 0
    assert c.laplacian.n_verts == after[0]
    # ... and both go on alike: the same view on the same background
    lb, lc = float(b.train_step()), float(c.train_step())
    assert abs(lb - lc) <= 1e-3 * abs(lb)


def test_stage1_starts_from_a_stage0_file(tmp_path):
    """A workspace with a stage-0 file only: restore_or_init loads it with model_only semantics -- model tensors equal, optimizer fresh,
    global_step 0."""
    from nerf2mesh_amd import checkpoint, synthetic
    from nerf2mesh_amd.engine import Stage0Engine
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    torch.manual_seed(0)
    opt0 = make_options(O=True, bound=1, dt_gamma=0, iters=30000, fused_mlp=True, workspace=str(tmp_path))
    eng = Stage0Engine(NeRFNetwork(opt0), opt0, synthetic.make_cameras(6, seed=0), torch.device("cuda", 0), seed=0)
    for _ in range(18):
        eng.train_step()
    torch.cuda.synchronize()
    path0 = checkpoint.save_checkpoint(eng, str(tmp_path))
    want = {k: v.detach().clone() for k, v in eng.model.state_dict().items()}
    mean_density = eng.model.mean_density
    assert mean_density > 0
    tr = _make(model_seed=123, workspace=tmp_path)
    fresh = _snapshot(tr)
    assert checkpoint.restore_or_init(tr, str(tmp_path), "latest") == (path0, "model_only")
    got = tr.model.state_dict()
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    assert tr.model.mean_density == mean_density
    assert tr.global_step == 0 and tr.scheduler.last_epoch == 500 and float(tr.optimizer.steps.sum()) == 0
    after = _snapshot(tr)
    for key in fresh[0]:
        if key.startswith("exp_avg") or key in ("scale", "steps", "growth_tracker", "param.vertices_offsets", "vertices", "triangles"):
            assert torch.equal(fresh[0][key], after[0][key]), key
    # the loaded tables are what the stage-1 forward reads: a step runs, and a stage-1 file now takes precedence
    from nerf2mesh_amd.engine_stage1 import Stage1Engine
    d = Stage1Engine(tr)
    assert torch.isfinite(d.train_step())
    p1 = checkpoint.save_checkpoint(d, str(tmp_path))
    tr2 = _make(model_seed=7, workspace=tmp_path)
    assert checkpoint.restore_or_init(tr2, str(tmp_path), "latest") == (p1, "full") and tr2.global_step == 1
