"""The opt-in cleaning of NeRFRenderer.export_stage0 (nerf/renderer.py:537 for the inner mesh, :653 for the outer cascades): the exported
meshes equal the device clean_mesh of the uncleaned ones, the floaters of a density grid are gone, and clean=False changes nothing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_clean_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _model(**kw):
    import torch
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    torch.manual_seed(0)
    opt = make_options(**{"O": True, "bound": 1, "dt_gamma": 0, **kw})
    return NeRFNetwork(opt).cuda()


def _fill(model, boxes, blobs=()):
    """Occupancy grid of every cascade: 50 inside the boxes and in the single cells holding the blob points, 0 elsewhere."""
    import torch
    from nerf2mesh_amd import raymarching
    H = model.grid_size
    boxes = torch.tensor(boxes, device="cuda", dtype=torch.float32)
    coords = raymarching.morton3D_invert(torch.arange(H ** 3, dtype=torch.int32, device="cuda")).long()
    for cas in range(model.cascade):
        b = min(2.0 ** cas, model.bound)
        p = ((coords.float() + 0.5) / H * 2 - 1) * b
        inside = ((p[:, None] >= boxes[None, :, :3]) & (p[:, None] <= boxes[None, :, 3:])).all(-1).any(-1)
        for q in blobs:
            cell = ((torch.tensor(q, device="cuda") / b + 1) / 2 * H).floor().long()
            inside |= (coords == cell).all(1)
        model.density_grid[cas] = inside.float() * 50.0
    model.mean_density = 20.0


BLOBS = [(0.8, 0.8, 0.8), (-0.8, 0.7, -0.75), (0.75, -0.8, 0.1), (-0.7, -0.7, 0.8), (0.1, 0.85, -0.8)]


def _same_mesh(a, b):
    import torch
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


def test_export_stage0_clean_inner_mesh(tmp_path):
    import torch
    from nerf2mesh_amd import export
    from nerf2mesh_amd.mesh_clean import clean_mesh
    model = _model()
    _fill(model, [[-0.5, -0.4, -0.45, 0.45, 0.5, 0.4]], BLOBS)
    raw = model.export_stage0(str(tmp_path / "raw"))[0]
    off = model.export_stage0(str(tmp_path / "off"), clean=False)[0]
    _same_mesh(raw, off)                                                       # an explicit clean=False is the default path
    n_raw = len(np.unique(R.components(raw[1].cpu().numpy().astype(np.int64), raw[0].shape[0])))
    assert n_raw == 1 + len(BLOBS), n_raw
    st = {}
    cl = model.export_stage0(str(tmp_path / "clean"), clean=True)[0]
    want = clean_mesh(*raw, min_f=8, min_d=5, repair=True, stats=st)
    _same_mesh(cl, want)
    pv, pt = export.read_ply(str(tmp_path / "clean" / "mesh_0.ply"))
    assert np.array_equal(pv, cl[0].cpu().numpy()) and np.array_equal(pt, cl[1].cpu().numpy())
    # the floaters are gone, the body stays
    lab = R.components(cl[1].cpu().numpy().astype(np.int64), cl[0].shape[0])
    assert len(np.unique(lab)) == 1
    assert st["degenerate"] + st["diameter_faces"] + st["size_faces"] > 0
    assert float(cl[0].abs().max()) < 0.55
    print(f"\nexport_stage0(clean=True): {raw[1].shape[0]} -> {cl[1].shape[0]} faces, {st}")
    # cleaning, then decimation to a target
    target = cl[1].shape[0] // 3
    v, t = model.export_stage0(str(tmp_path / "dec"), clean=True, decimate=True, decimate_target=target)[0]
    assert 0 < t.shape[0] <= target
    assert float(v.abs().max()) < 0.55


def test_export_stage0_clean_outer_cascades(tmp_path):
    """bound 4: each outer cascade equals clean_mesh(..., repair=False) of the uncleaned one (a cascade it empties is skipped)."""
    from nerf2mesh_amd.mesh_clean import clean_mesh
    model = _model(bound=4)
    assert model.cascade == 3
    _fill(model, [[-0.5, -0.5, -0.5, 0.5, 0.5, 0.5], [1.2, -0.6, -0.6, 1.8, 0.6, 0.6], [2.5, -1.0, -1.0, 3.5, 1.0, 1.0]],
          [(1.5, 1.5, 1.5), (-1.6, 1.2, 0.3), (3.0, -3.0, 2.5), (-3.2, 2.8, -2.9)])
    raw = model.export_stage0(str(tmp_path / "raw"))
    cl = model.export_stage0(str(tmp_path / "clean"), clean=True)
    assert sorted(raw) == [0, 1, 2]
    for cas in (1, 2):
        st = {}
        want = clean_mesh(*raw[cas], min_f=8, min_d=5, repair=False, stats=st)
        print(f"\ncascade {cas}: {raw[cas][1].shape[0]} -> {want[1].shape[0]} faces, {st}")
        if want[0].shape[0] == 0:
            assert cas not in cl
            continue
        _same_mesh(cl[cas], want)
        assert st["nonmanifold_faces"] == 0 and st["split_vertices"] == 0
    assert sum(clean_mesh(*raw[c], repair=False)[1].shape[0] < raw[c][1].shape[0] for c in (1, 2)) >= 1   # something was removed
