"""GPU: the stage-1 step executor under --contract (engine_stage1.Stage1Engine over n2m_gather_contract_x01) against the autograd trainer,
the executor with contraction off against the bits of the commit before it learnt to contract, and stage-1 construction from the two
meshes export_stage0 writes for the SDF recipe."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H = W = 64                     # the view; rasterised at 128 x 128 (ssaa 2)
MIN_OUTSIDE = 1.0 / 3.0        # share of the first frame's covered pixels that must lie outside the unit box


def two_cascade_mesh():
    """Cascade 0: the box scene (inside the unit box).  Cascade 1: a floor z = -1.05 over [-1.95, 1.95]^2, 24 x 24 quads: every point of
    it has |x|_inf >= 1.05, inside the marching bound 2."""
    import torch
    from nerf2mesh_amd import synthetic as S
    v0, f0 = S.scene_mesh(1500)
    k = 24
    lin = torch.linspace(-1.95, 1.95, k + 1)
    xx, yy = torch.meshgrid(lin, lin, indexing="ij")
    v1 = torch.stack([xx.reshape(-1), yy.reshape(-1), torch.full((xx.numel(),), -1.05)], -1)
    ii, jj = torch.meshgrid(torch.arange(k), torch.arange(k), indexing="ij")
    q = (ii * (k + 1) + jj).reshape(-1)
    f1 = torch.stack([q, q + (k + 1), q + (k + 2), q, q + (k + 2), q + 1], -1).reshape(-1, 3).int()
    v = torch.cat([v0, v1])
    f = torch.cat([f0.int(), f1 + v0.shape[0]])
    return v, f, [0, v0.shape[0], v.shape[0]], [0, f0.shape[0], f.shape[0]]


def cameras():
    """The four steepest of sixteen seeded cameras (elevation above 40 degrees): the floor fills the frame around the object."""
    import torch
    from nerf2mesh_amd import synthetic as S
    poses = S.make_cameras(16, seed=0)
    top = torch.argsort(poses[:, 2, 3], descending=True)[:4]
    assert float(poses[top, 2, 3].min()) > S.LEGO_RADIUS * np.sin(np.deg2rad(40.0))
    return poses[top].contiguous()


def make_trainer():
    import torch
    from nerf2mesh_amd.capture import Capture
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    from nerf2mesh_amd.trainer import Stage1Trainer
    dev = torch.device("cuda")
    torch.manual_seed(0)
    opt = make_options(O=True, bound=2, contract=True, stage=1, fused_mlp=True)
    assert opt.contract and opt.fp16 and opt.fused_mlp and not opt.enable_offset_nerf_grad
    cap = Capture.synthetic(cameras(), H=H, W=W, intrinsics=(70.0, 70.0, W / 2, H / 2), device=dev)
    v, f, vc, fc = two_cascade_mesh()
    tr = Stage1Trainer(NeRFNetwork(opt), opt, None, v, f, dev, capture=cap, v_cumsum=vc, f_cumsum=fc)
    assert tr.model.v_cumsum == vc and tr.model.f_cumsum == fc and tr.model.bound == 2
    for _ in range(500):
        tr.scheduler.step()               # past the warm-up, as tests/test_stage1.py does
    return tr


def params(tr):
    m = tr.model
    return {"colour table": m.encoder_color.embeddings.detach().float().clone(), "offsets": m.vertices_offsets.detach().clone(),
            **{f"mlp{i}": p.detach().clone() for i, p in enumerate(list(m.color_net.parameters()) + list(m.specular_net.parameters()))}}


def test_contracted_executor_reproduces_the_autograd_trainer():
    """The measure and the bounds of tests/test_stage1.py::test_stage1_executor_reproduces_the_autograd_trainer (restated: its helpers are
    local to that test), on the contracted recipe: first step, loss to 1e-5 and the gradients the optimizer reads to 2e-3 (fp16 colour
    table) / 1e-3 of their maximum; after 8 steps every parameter within 10 x the distance between two runs of the autograd trainer
    + 2e-3.  Before the executor contracted, `supported` was False here and construction raised ValueError."""
    import torch
    from nerf2mesh_amd.engine_stage1 import Stage1Engine
    from nerf2mesh_amd.renderer import contract
    STEPS = 8
    a = make_trainer()
    la = float(a.train_step().detach())
    ga = {"colour table": a._amp["color"]["grad_half"].float().clone(), "offsets": a.model.vertices_offsets.grad.clone()}
    b = make_trainer()
    assert Stage1Engine.supported(b)
    eng = Stage1Engine(b)
    seen = {}
    step = b.optimizer.step

    def spy(flagged=()):
        seen["colour table"], seen["offsets"] = eng.g2.float().clone(), b.model.vertices_offsets.grad.clone()
        seen["dw"] = eng.dw.clone()
        return step(flagged=flagged)
    b.optimizer.step = spy
    lb = float(eng.train_step())
    b.optimizer.step = step
    # ---- the condition of this test: the first frame shows the outer cascade, outside the unit box, on a third of its covered pixels
    K = int(b.model.last_covered)
    idx = eng.idx_buf[:K]
    from nerf2mesh_amd import _lib as L
    # (the RGB of the covered pixels has overwritten their positions in the RGBA image: interpolate them again)
    pos = torch.empty(eng.h * eng.w, 4, device=idx.device)
    L.call("n2m_interpolate_forward", L.ptr(eng.verts1), L.ptr(eng.rast), L.ptr(b.model.triangles), eng.verts.shape[0], b.model.triangles.shape[0], 4,
           eng.h, eng.w, L.ptr(pos), L.stream())
    world = pos[idx, :3]
    outside = world.abs().amax(dim=1) > 1
    share = float(outside.float().mean())
    print(f"covered pixels {K} of {eng.h * eng.w}, outside the unit box {share:.3f}")
    assert K > 1000 and share >= MIN_OUTSIDE and share < 1.0
    # the executor shaded the contracted points, and the table saw their coordinates in the bound-2 cube
    assert torch.equal(eng.pts[:K].cpu(), contract(world.cpu()))
    assert torch.equal(eng.x01[:K], 0.5 + eng.pts[:K] * 0.25) and float(eng.x01[:K].min()) > 0 and float(eng.x01[:K].max()) < 1
    # ---- first step
    assert abs(la - lb) <= 1e-5 * abs(la), (la, lb)
    assert float(seen["dw"].abs().sum()) > 0
    for k in ga:
        d = float((ga[k] - seen[k]).abs().max()) / float(ga[k].abs().max())
        print(f"first-step gradient, {k}: max |diff| / max = {d:.3g}")
        assert d <= (2e-3 if k == "colour table" else 1e-3), k
    assert b.model.last_covered == a.model.last_covered > 0
    assert torch.equal(a.model.triangles_errors_cnt, b.model.triangles_errors_cnt)
    # ---- STEPS steps: parameters, against two runs of the autograd trainer
    a2 = make_trainer()
    for _ in range(STEPS):
        a2.train_step()
    for _ in range(STEPS - 1):
        a.train_step(); eng.train_step()
    pa, pa2, pb = params(a), params(a2), params(b)
    rel = lambda x, y: float((x - y).norm() / x.norm().clamp_min(1e-30))
    for k in pa:
        d_te, d_tt = rel(pa[k], pb[k]), rel(pa[k], pa2[k])
        print(f"{k:14s} trainer-vs-executor {d_te:.3g}   trainer-vs-trainer {d_tt:.3g}")
        assert d_te <= 10 * d_tt + 2e-3, k
    assert b.global_step == a.global_step == STEPS and abs(b.covered_seen - a.covered_seen) <= max(16, 4 * abs(a2.covered_seen - a.covered_seen))


def test_uncontracted_step_keeps_the_recorded_bits():
    """Contraction off: one executor step on the uncontracted case (tests/stage1_executor_case.py) against the arrays
    tests/golden/make_golden_stage1_executor.py recorded from the commit before n2m_gather_contract_x01 replaced the gather and the two
    table-coordinate statements.  Loss, covered pixels, every network parameter, the colour table (digest, moved entries, sample), the
    gathered points, their table coordinates and the shaded RGBA image: the same bits.
    The vertex offsets are NOT reproducible to the bit on that commit itself -- their gradient is summed with float atomics in the raster
    / antialias backward; three recordings of it differ from each other in ~100 of 36504 entries by up to 2.9e-11 (offsets are 1e-4 after
    the step) -- so they are held to 4 x the largest distance between the three recordings, the recorded run's own spread; nothing this
    step changed lies on their path.  The antialiased image's digest differs between recordings too and is not compared."""
    import stage1_executor_case as EC
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stage1_executor_step.npz"))
    unstable = set(gold["unstable"].tolist())
    assert unstable == {"offsets", "aa_sha256"}
    got = EC.record()
    exact = [k for k in got if k not in unstable]
    assert {"loss", "covered", "mlp0", "mlp4", "table_sha256", "table_moved", "table_sample", "pts_sha256", "x01_sha256", "rgba_sha256"} <= set(exact)
    for k in exact:
        assert EC.same_bits(got[k], gold[k]), k
    recs = [gold["offsets"], gold["offsets_b"], gold["offsets_c"]]
    spread = max(float(np.abs(recs[i] - recs[j]).max()) for i in range(3) for j in range(i))
    d = float(np.abs(got["offsets"] - recs[0]).max())
    print(f"offsets: distance from the recording {d:.3g}, spread of the three recordings {spread:.3g}, magnitude {np.abs(recs[0]).max():.3g}")
    assert spread > 0 and d <= 4 * spread
    assert int((got["offsets"] != recs[0]).sum()) <= 0.02 * recs[0].size


def test_stage1_loads_both_exported_cascades(tmp_path):
    """export_stage0 on the SDF recipe's analytic field (tests/sdf_shell_case.py) -> export.load_stage0_meshes -> a stage-1 model with two
    cascades; a directory whose shell was emptied gives one."""
    import torch
    import sdf_shell_case as SC
    from nerf2mesh_amd import export, synthetic as S
    from nerf2mesh_amd.trainer import Stage1Trainer
    path = str(tmp_path / "mesh_stage0")
    model, opt, meshes = SC.export(path)
    v, f, vc, fc = export.load_stage0_meshes(path, model.cascade)
    assert len(vc) == len(fc) == 3 and vc[1] == meshes[0][0].shape[0] and vc[2] - vc[1] == meshes[1][0].shape[0]
    assert np.array_equal(v[vc[1]:], meshes[1][0].cpu().numpy()) and np.array_equal(f[fc[1]:] - vc[1], meshes[1][1].cpu().numpy())
    opt.stage = 1
    tr = Stage1Trainer(model, opt, S.make_cameras(2, seed=0), torch.from_numpy(v), torch.from_numpy(f), torch.device("cuda"), H=32, W=32,
                       v_cumsum=vc, f_cumsum=fc)
    m = tr.model
    assert len(m.v_cumsum) == 3 and len(m.f_cumsum) == 3 and m.f_cumsum[-1] == m.triangles.shape[0] == f.shape[0]
    assert int(m.triangles[fc[1]:].min()) >= vc[1]                       # the shell's faces name the shell's vertices
    os.remove(os.path.join(path, "mesh_1.ply"))                          # an emptied shell writes no file: one cascade
    v1, f1, vc1, fc1 = export.load_stage0_meshes(path, model.cascade)
    assert vc1 == vc[:2] and fc1 == fc[:2] and np.array_equal(v1, v[:vc[1]])
    os.remove(os.path.join(path, "mesh_0.ply"))
    with pytest.raises(FileNotFoundError):
        export.load_stage0_meshes(path, model.cascade)
