"""Stage-1 mesh refinement with the opt-in isotropic re-meshing: NeRFRenderer.refine_and_decimate(remesh=True) against the numpy
restatement chain decimate -> remesh -> subdivide (tests/mesh_simplify_ref.py, tests/mesh_remesh_ref.py), the untouched default, the
`--sdf` path where the re-meshing is the whole refinement, and Stage1Trainer.refine_mesh(remesh=True)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_remesh_ref as M  # noqa: E402
import mesh_simplify_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


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


def _scene():
    from nerf2mesh_amd import synthetic as S
    v, f = (x.numpy() for x in S.scene_mesh(3000))
    return v.astype(np.float32), f.astype(np.int32)


def _loaded_model(v, f, err, cnt, **kw):
    import torch
    model = _model(**kw)
    model.init_stage1(torch.from_numpy(v), torch.from_numpy(f))
    off = torch.randn(len(v), 3, generator=torch.Generator().manual_seed(1)) * 1e-3
    model.vertices_offsets.data.copy_(off.cuda())
    model.triangles_errors.copy_(torch.from_numpy(err))
    model.triangles_errors_cnt.copy_(torch.from_numpy(cnt))
    return model, (torch.from_numpy(v) + off).numpy()               # vertices + offsets, as the device adds them


def test_refine_and_decimate_with_remesh_equals_the_restatement(tmp_path):
    from nerf2mesh_amd import export
    v, f = _scene()
    err, cnt = _error_field(v, f)
    model, vin = _loaded_model(v, f, err, cnt)
    assert model.opt.refine_remesh_size == 0.02
    out = model.refine_and_decimate(save_path=str(tmp_path), remesh=True)
    mask = R.refine_classes(err, cnt, len(f))
    assert out["changed"] and out["decimate"] == int((mask == 1).sum()) and out["refine"] == int((mask == 2).sum())
    rv, rf, n_before, n_after = M.refine(vin, f, mask, decimate_ratio=0.1, remesh_size=0.02, refine_size=0.01)
    assert out["remesh"] == {"faces_before": n_before, "faces_after": n_after} and n_before != n_after
    assert np.array_equal(model.triangles.cpu().numpy(), rf)
    assert np.array_equal(model.vertices.cpu().numpy().view(np.uint32), rv.view(np.uint32))
    # unseen faces away from class 2: neither the decimation, the re-meshing (selected-only, strict) nor the subdivision touches them
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


def test_the_default_did_not_move():
    v, f = _scene()
    err, cnt = _error_field(v, f)
    model, vin = _loaded_model(v, f, err, cnt)
    out = model.refine_and_decimate()
    assert "remesh" not in out
    rv, rf = R.refine(vin, f, R.refine_classes(err, cnt, len(f)), decimate_ratio=0.1, refine_size=0.01)
    assert np.array_equal(model.triangles.cpu().numpy(), rf)
    assert np.array_equal(model.vertices.cpu().numpy().view(np.uint32), rv.view(np.uint32))


def test_sdf_refinement_is_the_remesh():
    """--sdf: every face is class 1, no decimation, no subdivision; the re-meshing is the refinement.  The `--sdf` options set
    enable_offset_nerf_grad, which Stage1Engine does not cover (Stage1Engine.supported), so the step on the re-meshed mesh is taken
    twice: by the autograd trainer with the SDF options, and by a Stage1Engine of the fused recipe on the same mesh."""
    import torch
    from nerf2mesh_amd import synthetic as S
    from nerf2mesh_amd.engine_stage1 import Stage1Engine
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    from nerf2mesh_amd.trainer import Stage1Trainer
    v, f = _scene()
    model, vin = _loaded_model(v, f, np.zeros(len(f), np.float32), np.zeros(len(f), np.float32), sdf=True, fused_mlp=True)
    opt = model.opt
    assert opt.sdf and opt.refine_decimate_ratio == 0 and opt.refine_size == 0 and opt.refine_remesh_size == 0.02
    nf_before = np.unique(R.edge_face_counts(f))
    out = model.refine_and_decimate(remesh=True)
    assert out["changed"] and out["decimate"] == out["decimate_after"] == len(f) and out["refine"] == 0
    rv, rf, _ = M.remesh_isotropic(vin, f, 0.02, iterations=3)
    mv, mf = model.vertices.cpu().numpy(), model.triangles.cpu().numpy()
    assert np.array_equal(mf, rf) and np.array_equal(mv.view(np.uint32), rv.view(np.uint32))
    assert out["remesh"] == {"faces_before": len(f), "faces_after": len(rf)} and len(rf) != len(f)
    assert np.array_equal(np.unique(R.edge_face_counts(mf)), nf_before)      # manifold where it was, the same kinds of edges
    assert R.euler(mv, mf) == R.euler(v, f)
    dev = torch.device("cuda")
    poses = S.make_cameras(4, seed=0)
    mesh_v, mesh_f = model.vertices.clone(), model.triangles.clone()
    tr = Stage1Trainer(model, opt, poses, mesh_v, mesh_f, dev, H=100, W=100)
    assert not Stage1Engine.supported(tr)                          # the SDF options: the autograd step
    loss = float(tr.train_step().detach())
    assert np.isfinite(loss), loss
    torch.manual_seed(0)
    fopt = make_options(O=True, bound=1, dt_gamma=0, stage=1, fused_mlp=True)
    loss = float(Stage1Engine(Stage1Trainer(NeRFNetwork(fopt), fopt, poses, mesh_v, mesh_f, dev, H=100, W=100)).train_step())
    assert np.isfinite(loss), loss


def test_refine_mesh_passes_remesh_on():
    import torch
    from nerf2mesh_amd import synthetic as S
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    from nerf2mesh_amd.trainer import Stage1Trainer
    v, f = _scene()
    err, cnt = _error_field(v, f)
    model, _ = _loaded_model(v, f, err, cnt)
    want = model.refine_and_decimate(remesh=True)
    torch.manual_seed(0)
    opt = make_options(O=True, bound=1, dt_gamma=0, stage=1)
    tr = Stage1Trainer(NeRFNetwork(opt), opt, S.make_cameras(4, seed=0), torch.from_numpy(v), torch.from_numpy(f), torch.device("cuda"), H=64, W=64)
    tr.model.triangles_errors.copy_(torch.from_numpy(err))
    tr.model.triangles_errors_cnt.copy_(torch.from_numpy(cnt))
    got = tr.refine_mesh(remesh=True)
    # the model call above started from offsets of 1e-3, the trainer from zero offsets: the class counts agree, the re-meshing ran in both
    assert got["decimate"] == want["decimate"] and got["refine"] == want["refine"] and "remesh" in got
    again = _loaded_model(v, f, err, cnt)[0]
    again.vertices_offsets.data.zero_()
    assert again.refine_and_decimate(remesh=True) == got
    assert tr.model.triangles.shape[0] == got["after"]["faces"] and float(tr.model.vertices_offsets.detach().abs().sum()) == 0
