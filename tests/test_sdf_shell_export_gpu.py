"""GPU: export_stage0 of the SDF recipe on an unbounded scene writes the contracted outer shell as mesh_1.ply (nerf/renderer.py:548-601),
on the analytic field of tests/sdf_shell_case.py.  On the commit before the shell branch there is no key 1."""
import os

import pytest

import sdf_shell_case as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def exported(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("shell") / "mesh_stage0")
    model, opt, meshes = SC.export(path)
    return path, model, meshes


def test_shell_is_exported_and_reads_back(exported):
    import numpy as np
    from nerf2mesh_amd import export
    path, model, meshes = exported
    assert sorted(meshes) == [0, 1]
    v, t = meshes[1]
    # the condition of the geometry checks below: a shell of a few hundred faces at least (sdf_shell_case.py expects thousands)
    print("shell:", v.shape[0], "vertices,", t.shape[0], "faces; inner mesh:", meshes[0][1].shape[0], "faces")
    assert t.shape[0] >= 300 and int(t.max()) < v.shape[0] and int(t.min()) >= 0
    rv, rt = export.read_ply(os.path.join(path, "mesh_1.ply"))
    assert np.array_equal(rv.view(np.int32), v.cpu().numpy().view(np.int32)) and np.array_equal(rt, t.cpu().numpy())


def test_shell_geometry(exported):
    import torch
    from nerf2mesh_amd.renderer import contract
    _, model, meshes = exported
    v = meshes[1][0]
    assert v.shape[0] > 0
    lo, hi = model.aabb_train[:3], model.aabb_train[3:]
    assert lo.tolist() == [-2, -2, -2] and hi.tolist() == [2, 2, 2]              # the default box
    assert bool(((v > lo) & (v < hi)).all())                                      # strictly inside
    c = contract(v.cpu())                                                         # the CPU statement
    assert not bool((c.abs() <= 0.5 * SC.SCALE).all(dim=1).any())                 # the unit box's half belongs to mesh_0
    assert bool((v.abs().amax(dim=1) > 1).any())                                  # and the shell does reach outside the unit box
    # back on the lattice: vertex / (2 - 2/R) is the normalised lattice position, the field was queried at twice that
    cell = 2 * 2 / (SC.RESOLUTION - 1)
    d = SC.zero_set_distance(2 * (c / SC.SCALE))
    print("largest distance from the analytic zero set:", float(d.max()), "cell:", cell)
    assert float(d.max()) <= cell


def test_shell_equals_the_restated_chain(exported):
    """No clean, no decimation, no dataset: the vertices are, bit for bit, the chain of nerf/renderer.py:563-593 restated here in torch on
    the CPU, from the same marching-cubes output."""
    import torch
    from nerf2mesh_amd.marching_cubes import marching_cubes
    _, model, meshes = exported
    R = SC.RESOLUTION
    sig = torch.nan_to_num(model.density_volume(R, 128, scale=2.0), 0)
    assert abs(float(sig[0, 0, 0]) - ((12 ** 0.5 - SC.SHELL_R) - SC.SHELL_HALF)) < 1e-5       # queried at (-2, -2, -2)
    v, t = marching_cubes(-sig, 0.0, div=R - 1.0, mul=2.0, add=-1.0)
    v, t = v.cpu(), t.cpu().long()

    def remove(v, t, sel):
        keep_f = ~sel[t].any(dim=1)
        remap = torch.cumsum((~sel).long(), 0) - 1
        return v[~sel], remap[t[keep_f]]
    v, t = remove(v, t, (v.abs() <= 0.5).all(dim=1))
    v = v * (2 - 2 / R)
    mag = torch.amax(torch.abs(v), dim=1, keepdim=True)
    v = torch.where(mag <= 1, v, v * (1 / (2 * mag - mag * mag)))
    a = model.aabb_train.cpu()
    v, t = remove(v, t, ((v <= a[:3]) | (v >= a[3:])).any(dim=1))
    got_v, got_t = meshes[1][0].cpu(), meshes[1][1].cpu().long()
    assert got_v.shape == v.shape and torch.equal(got_v.view(torch.int32), v.view(torch.int32))
    assert torch.equal(got_t, t)


def test_inner_mesh_is_untouched(exported, tmp_path):
    """meshes[0] and the bytes of mesh_0.ply equal those of a run without the shell branch (self.bound forced to 1) on the same field."""
    import torch
    path, model, meshes = exported
    model.bound = 1
    try:
        plain = model.export_stage0(str(tmp_path), resolution=SC.RESOLUTION)
    finally:
        model.bound = 2
    assert sorted(plain) == [0] and not os.path.exists(os.path.join(str(tmp_path), "mesh_1.ply"))
    assert torch.equal(plain[0][0], meshes[0][0]) and torch.equal(plain[0][1], meshes[0][1]) and meshes[0][1].shape[0] > 0
    assert open(os.path.join(str(tmp_path), "mesh_0.ply"), "rb").read() == open(os.path.join(path, "mesh_0.ply"), "rb").read()


def test_no_background_no_shell(tmp_path):
    _, _, meshes = SC.export(str(tmp_path), background=False)
    assert sorted(meshes) == [0] and meshes[0][1].shape[0] > 0
    assert os.listdir(str(tmp_path)) == ["mesh_0.ply"]


def test_shell_with_clean_and_decimate(tmp_path):
    """clean=True, decimate=True: the shell is cleaned without repair and decimated to 2 * decimate_target faces when it has more."""
    model, _, raw = SC.export(str(tmp_path / "raw"))
    target = raw[1][1].shape[0] // 8
    meshes = model.export_stage0(str(tmp_path / "dec"), resolution=SC.RESOLUTION, clean=True, decimate=True, decimate_target=target)
    assert 1 in meshes and 0 < meshes[1][1].shape[0] < raw[1][1].shape[0]
    v = meshes[1][0]
    assert bool(((v > model.aabb_train[:3]) & (v < model.aabb_train[3:])).all())
