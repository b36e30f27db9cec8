"""Stage-1 mesh refinement on the device: NeRFRenderer.refine_and_decimate (nerf/renderer.py:209-294) against the numpy restatement
(tests/mesh_simplify_ref.py), Stage1Trainer.refine_mesh (nerf/utils.py:1204-1211) on one and two ranks, and the decimation of
export_stage0 (nerf/renderer.py:540-541, :582-583)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_simplify_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(**kw):
    import torch
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    torch.manual_seed(0)
    opt = make_options(**{"O": True, "bound": 1, "dt_gamma": 0, "stage": 1, **kw})
    return NeRFNetwork(opt).cuda()


def _error_field(v, f):
    """High error right of x = 0.3, elsewhere rising with y (so the low half forms patches whose inner vertices may move), unseen below
    z = -0.2."""
    c = v[f].mean(1)
    rng = np.random.default_rng(0)
    err = ((c[:, 1] - c[:, 1].min()) * 0.1 + rng.random(len(f)) * 1e-3).astype(np.float32)
    err[c[:, 0] > 0.3] += np.float32(5.0)
    cnt = rng.integers(1, 4, len(f)).astype(np.float32)
    cnt[c[:, 2] < -0.2] = 0
    err[cnt == 0] = 0
    return err * cnt, cnt


def _tri_set(v, f):
    return {np.asarray(v, np.float32)[t].tobytes() for t in f}


def test_refine_and_decimate_equals_the_restatement(tmp_path):
    import torch
    from nerf2mesh_amd import export, synthetic as S
    v, f = (x.numpy() for x in S.scene_mesh(3000))
    v, f = v.astype(np.float32), f.astype(np.int32)
    err, cnt = _error_field(v, f)
    model = _model()
    model.init_stage1(torch.from_numpy(v), torch.from_numpy(f))
    off = torch.randn(len(v), 3, generator=torch.Generator().manual_seed(1)) * 1e-3
    model.vertices_offsets.data.copy_(off.cuda())
    model.triangles_errors.copy_(torch.from_numpy(err))
    model.triangles_errors_cnt.copy_(torch.from_numpy(cnt))
    out = model.refine_and_decimate(save_path=str(tmp_path))
    vin = (torch.from_numpy(v) + off).numpy()                    # vertices + offsets, as the device adds them
    mask = R.refine_classes(err, cnt, len(f))
    assert out["changed"] and out["decimate"] == int((mask == 1).sum()) and out["refine"] == int((mask == 2).sum())
    rv, rf = R.refine(vin, f, mask, decimate_ratio=0.1, refine_size=0.01)
    assert np.array_equal(model.triangles.cpu().numpy(), rf)
    assert np.array_equal(model.vertices.cpu().numpy().view(np.uint32), rv.view(np.uint32))
    # class 1 reduced to int(0.9 n1) (the last collapse may remove one face more), class-2 faces subdivided
    n1 = int((mask == 1).sum())
    assert out["decimate"] == n1 and int(0.9 * n1) - 1 <= out["decimate_after"] <= int(0.9 * n1), out
    _, _, src = R.decimate(vin, f, int(0.9 * n1), selected=(mask == 1))
    assert int((mask[src] == 1).sum()) == out["decimate_after"]
    n2_faces = int((mask[src] == 2).sum())
    assert n2_faces == int((mask == 2).sum()) and len(rf) >= len(src) + 3 * n2_faces   # every class-2 face split at least into 4
    # unseen faces: decimation never moves their vertices; subdivision re-triangulates only those that share an edge with a class-2 face
    near2 = np.zeros(len(v), bool)
    near2[f[mask == 2].reshape(-1)] = True
    alone = (cnt == 0) & ~near2[f].any(1)
    assert alone.sum() > 100 and _tri_set(vin, f[alone]) <= _tri_set(rv, rf)
    # state of the new mesh
    assert model.v_cumsum == [0, len(rv)] and model.f_cumsum == [0, len(rf)]
    assert float(model.vertices_offsets.detach().abs().sum()) == 0 and float(model.triangles_errors.abs().sum()) == 0
    assert float(model.triangles_errors_cnt.abs().sum()) == 0 and model.triangles_errors.shape[0] == len(rf)
    pv, pf = export.read_ply(str(tmp_path / "mesh_0_updated.ply"))
    assert np.array_equal(pv, rv) and np.array_equal(pf, rf)


def test_refine_and_decimate_cascades_and_no_seen_faces():
    import torch
    from nerf2mesh_amd import synthetic as S
    v0, f0 = (x.numpy() for x in S.scene_mesh(2000))
    v1, f1 = R.torus(24, 12, R=3.0, r=0.5)
    v = np.concatenate([v0, v1]).astype(np.float32)
    f = np.concatenate([f0, f1 + len(v0)]).astype(np.int32)
    model = _model()
    model.init_stage1(torch.from_numpy(v), torch.from_numpy(f), v_cumsum=[0, len(v0), len(v)], f_cumsum=[0, len(f0), len(f)])
    out = model.refine_and_decimate()                             # nothing seen: unchanged
    assert not out["changed"] and model.triangles.shape[0] == len(f)
    err, cnt = _error_field(v0, f0)
    model.triangles_errors[:len(f0)] = torch.from_numpy(err).cuda()
    model.triangles_errors_cnt[:len(f0)] = torch.from_numpy(cnt).cuda()
    model.triangles_errors_cnt[len(f0):] = 1                    # the outer cascade's errors play no part
    out = model.refine_and_decimate()
    rv, rf = R.refine(v0, f0, R.refine_classes(err, cnt, len(f0)))
    vc, fc = model.v_cumsum, model.f_cumsum
    assert vc == [0, len(rv), len(rv) + len(v1)] and fc == [0, len(rf), len(rf) + len(f1)]
    mv, mf = model.vertices.cpu().numpy(), model.triangles.cpu().numpy()
    assert np.array_equal(mv[:vc[1]], rv) and np.array_equal(mf[:fc[1]], rf)
    assert np.array_equal(mv[vc[1]:], v1) and np.array_equal(mf[fc[1]:] - vc[1], f1)


def test_refine_mesh_then_a_new_executor():
    import torch
    from nerf2mesh_amd import synthetic as S
    from nerf2mesh_amd.engine_stage1 import Stage1Engine
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    from nerf2mesh_amd.trainer import Stage1Trainer
    dev = torch.device("cuda")
    v, f = S.scene_mesh(20000)
    torch.manual_seed(0)
    opt = make_options(O=True, bound=1, dt_gamma=0, stage=1, fused_mlp=True)
    poses = S.make_cameras(6, seed=0)
    a = Stage1Trainer(NeRFNetwork(opt), opt, poses, v, f, dev, H=200, W=200)
    old = Stage1Engine(a)
    for _ in range(6):
        old.train_step()
    stats = a.refine_mesh()
    assert stats["changed"] and stats["after"]["faces"] != stats["before"]["faces"], stats
    with pytest.raises(RuntimeError, match="build a new Stage1Engine"):
        old.train_step()
    assert a.global_step == 6 and float(a.model.vertices_offsets.detach().abs().sum()) == 0
    # the autograd trainer on the refined mesh, same weights, same step
    mb = NeRFNetwork(opt)
    mb.load_state_dict({k: t for k, t in a.model.state_dict().items() if k != "vertices_offsets"}, strict=False)
    b = Stage1Trainer(mb, opt, poses, a.model.vertices.clone(), a.model.triangles.clone(), dev, H=200, W=200)
    b.global_step = a.global_step
    b.gen.set_state(a.gen.get_state())                           # refine_mesh keeps the background generator's stream
    lb = float(b.train_step().detach())
    eng = Stage1Engine(a)
    la = float(eng.train_step())
    assert abs(la - lb) <= 1e-5 * abs(lb), (la, lb)
    losses = [la] + [float(eng.train_step()) for _ in range(19)]
    assert all(np.isfinite(losses)), losses


def test_two_ranks_refine_to_the_same_mesh():
    env = dict(os.environ, N2M_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29533", os.path.join(ROOT, "tools", "dist_check_refine.py")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DIST_CHECK_REFINE OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_export_stage0_decimates_to_the_target(tmp_path):
    import torch
    from nerf2mesh_amd import export, synthetic as S
    from nerf2mesh_amd.engine import Stage0Engine
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    torch.manual_seed(0)
    opt = make_options(O=True, bound=1, dt_gamma=0, iters=30000, fused_mlp=True)
    eng = Stage0Engine(NeRFNetwork(opt), opt, S.make_cameras(100, seed=0), torch.device("cuda:0"), seed=0)
    eng.mark_untrained()
    for _ in range(400):
        eng.train_step()
    model = eng.model
    raw = model.export_stage0(str(tmp_path / "raw"), resolution=192)[0]
    again = model.export_stage0(str(tmp_path / "raw2"), resolution=192, decimate=False)[0]
    assert torch.equal(raw[0], again[0]) and torch.equal(raw[1], again[1])      # the default path is unchanged
    target = raw[1].shape[0] // 4
    v, t = model.export_stage0(str(tmp_path / "dec"), resolution=192, decimate_target=target, decimate=True)[0]
    assert 0 < t.shape[0] <= target
    pv, pt = export.read_ply(str(tmp_path / "dec" / "mesh_0.ply"))
    assert np.array_equal(pv, v.cpu().numpy()) and np.array_equal(pt, t.cpu().numpy())
    # every decimated vertex stays within 1.5 voxels of the raw iso-surface (distance to the nearest raw vertex, sampled)
    voxel = 2.0 / 191
    rv = raw[0]
    sample = v[torch.randperm(v.shape[0], generator=torch.Generator().manual_seed(0))[:4000].cuda()]
    d = torch.cdist(sample, rv).min(1).values
    print(f"\nexport_stage0: {raw[1].shape[0]} -> {t.shape[0]} faces, max distance {float(d.max()) / voxel:.3f} voxels")
    assert float(d.max()) <= 1.5 * voxel


def _cascade_model():
    """bound 4 (three cascades) with an occupancy grid of boxes: one at the centre, one only cascade 1 reaches, one only cascade 2 keeps."""
    import torch
    from nerf2mesh_amd import raymarching
    model = _model(bound=4)
    H = model.grid_size
    boxes = torch.tensor([[-0.5, -0.5, -0.5, 0.5, 0.5, 0.5], [1.2, -0.6, -0.6, 1.8, 0.6, 0.6], [2.5, -1.0, -1.0, 3.5, 1.0, 1.0]], device="cuda")
    coords = raymarching.morton3D_invert(torch.arange(H ** 3, dtype=torch.int32, device="cuda")).long()
    for cas in range(model.cascade):
        b = min(2.0 ** cas, model.bound)
        p = ((coords.float() + 0.5) / H * 2 - 1) * b
        inside = ((p[:, None] >= boxes[None, :, :3]) & (p[:, None] <= boxes[None, :, 3:])).all(-1).any(-1)
        model.density_grid[cas] = inside.float() * 50.0
    model.mean_density = 20.0
    return model


def _outer_meshes_as_before(model):
    """The outer cascades exactly as export_stage0 extracts them without decimation (nerf/renderer.py:603-672, the code before
    `decimate` existed): trilinear resample to env_reso, binarise, marching cubes at 0.5, drop the centre and what lies outside aabb_train."""
    import torch
    import torch.nn.functional as F
    from nerf2mesh_amd import export
    from nerf2mesh_amd.marching_cubes import marching_cubes
    thresh = min(model.mean_density, model.density_thresh)
    reso = int(getattr(model.opt, "env_reso", 256))
    out = {}
    for cas in range(1, model.cascade):
        bound = min(2 ** cas, model.bound)
        hgs = bound / reso
        occ = F.interpolate(model._grid_as_volume(cas)[None, None], [reso] * 3, mode="trilinear")[0, 0]
        occ = (torch.nan_to_num(occ, 0) > thresh).float()
        v, t = marching_cubes(occ, 0.5, div=reso - 1.0, mul=2.0, add=-1.0)
        v, t = export.remove_vertices(v, t, (v.abs() <= 0.45).all(dim=1))
        if v.shape[0] == 0:
            continue
        v = v * (bound - hgs)
        lo, hi = model.aabb_train[:3] + hgs, model.aabb_train[3:] - hgs
        v, t = export.remove_vertices(v, t, ((v <= lo) | (v >= hi)).any(dim=1))
        if v.shape[0]:
            out[cas] = (v, t)
    return out


def test_export_stage0_outer_cascades(tmp_path):
    """bound > 1: without `decimate` the outer cascades are the raw iso-surfaces, as before; with it each is cut to decimate_target // 2."""
    import torch
    from nerf2mesh_amd import export
    model = _cascade_model()
    assert model.cascade == 3
    want = _outer_meshes_as_before(model)
    assert sorted(want) == [1, 2] and all(t.shape[0] > 1000 for _, t in want.values())
    raw = model.export_stage0(str(tmp_path / "raw"))
    for cas, (v, t) in want.items():
        assert torch.equal(raw[cas][0], v) and torch.equal(raw[cas][1], t), cas
    inner = raw[0][1].shape[0]
    target = 2 * (min(t.shape[0] for _, t in want.values()) // 3)
    dec = model.export_stage0(str(tmp_path / "dec"), decimate_target=target, decimate=True)
    assert dec[0][1].shape[0] == inner if inner <= target else dec[0][1].shape[0] <= target
    for cas in want:
        v, t = dec[cas]
        print(f"\ncascade {cas}: {want[cas][1].shape[0]} -> {t.shape[0]} faces (target {target // 2})")
        assert 0 < t.shape[0] <= target // 2
        pv, pt = export.read_ply(str(tmp_path / "dec" / f"mesh_{cas}.ply"))
        assert np.array_equal(pv, v.cpu().numpy()) and np.array_equal(pt, t.cpu().numpy())
