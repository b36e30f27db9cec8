"""Re-meshing with re-projection onto the input surface, `remesh_isotropic(project=True)`: the numpy restatement
(tests/mesh_query_ref.py on top of tests/mesh_remesh_ref.py) keeps the invariants of the unprojected rule, puts every relaxed vertex on
the input surface and lowers the drift from the analytic surface; the device equals the restatement bit for bit, and project=False is
the call without the argument."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_query_ref as Q  # noqa: E402
import mesh_remesh_ref as M  # noqa: E402
import mesh_simplify_ref as R  # noqa: E402
import test_mesh_remesh as T  # noqa: E402

INPUTS = {"sphere": (lambda: R.icosphere(3), 0.2), "torus": (lambda: R.torus(32, 16), 0.15), "grid": (lambda: R.grid_patch(16), 0.1)}


def _analytic(name, p):
    p = np.asarray(p, np.float64)
    return np.abs(np.linalg.norm(p, axis=1) - 1.0) if name == "sphere" else T._torus_distance(p)


def _sag(name, v, f, n=12, rounds=40):
    """The input mesh's own sag: the largest distance of a point of the mesh from the analytic surface.  Per face, the largest node of an
    n-subdivision barycentric lattice, then refined: a 5 x 5 lattice around the best point so far, clipped to the face, its window halved
    every round until it is below fp64 resolution.  Every value is the distance of a point of the mesh, so the result never exceeds the
    true sag; the lattice alone stops up to one node spacing short of a face's deepest point (torus(32, 16): 0.0130350 on the
    12-lattice, 0.0130386 on a 96-lattice, 0.0130393 refined).  -> (refined sag, sag on the bare lattice)."""
    p = np.asarray(v, np.float64)[np.asarray(f)]
    F = len(p)

    def dist(w0, w1):
        return _analytic(name, w0[:, None] * p[:, 0] + w1[:, None] * p[:, 1] + (1.0 - w0 - w1)[:, None] * p[:, 2])
    best, b0, b1 = np.full(F, -1.0), np.zeros(F), np.zeros(F)
    for i in range(n + 1):
        for j in range(n + 1 - i):
            w0, w1 = np.full(F, i / n), np.full(F, j / n)
            d = dist(w0, w1)
            up = d > best
            best[up], b0[up], b1[up] = d[up], w0[up], w1[up]
    lattice = float(best.max())
    h = 1.0 / n
    for _ in range(rounds):
        c0, c1 = b0.copy(), b1.copy()
        for di in (-1.0, -0.5, 0.0, 0.5, 1.0):
            for dj in (-1.0, -0.5, 0.0, 0.5, 1.0):
                w0 = np.clip(c0 + di * h, 0.0, 1.0)
                w1 = np.clip(c1 + dj * h, 0.0, 1.0 - w0)
                d = dist(w0, w1)
                up = d > best
                best[up], b0[up], b1[up] = d[up], w0[up], w1[up]
        h *= 0.5
    return float(best.max()), lattice


# ------------------------------------------------------------------------------------------------------- CPU: the restatement
@pytest.mark.parametrize("name", ["sphere", "torus", "grid"])
def test_reference_projected_topology_is_kept(name):
    """What test_reference_topology_is_kept asserts of the unprojected rule."""
    make, L = INPUTS[name]
    v, f = make()
    v2, f2, src = Q.remesh_isotropic(v, f, L)
    assert len(f2) != len(f)
    assert R.euler(v2, f2) == R.euler(v, f)
    T._sound(v2, f2)
    if name == "grid":
        assert set(np.unique(R.edge_face_counts(f2)).tolist()) == {1, 2} and T._boundary_loops(f2) == T._boundary_loops(f) == 1
    else:
        assert T._manifold(f2)
    assert src.min() >= 0 and src.max() < len(f)


@pytest.mark.parametrize("name", ["sphere", "torus", "grid"])
def test_reference_projected_pass_invariants(name):
    """What test_reference_pass_invariants asserts: no long edge after the split pass, no valid short edge after the collapse pass, the
    valence deviation falling strictly over the flip rounds."""
    make, L = INPUTS[name]
    v, f = make()
    lo2, hi2 = M.thresholds(L)
    cos_f = M.cos_feature(30.0)
    seen = []

    def hook(stage, it, v, f, sel):
        seen.append(stage)
        if stage == "split":
            edges, _, c2e = R.edges_of(f, len(v))
            assert not M.split_marks(v, f, sel, hi2, edges, c2e).any()
            p = v.astype(np.float64)
            d = p[edges[:, 1]] - p[edges[:, 0]]
            assert (d * d).sum(1).max() <= hi2
        if stage == "collapse":
            keys, _, _ = M.collapse_keys(v, f, sel, lo2, hi2, cos_f)
            assert np.all(keys == M.NO_KEY)
    stats = {}
    Q.remesh_isotropic(v, f, L, stats=stats, hook=hook)
    assert seen == ["split", "collapse", "flip", "relax"] * 3
    work = 0
    for it in stats["iterations"]:
        assert it["split_rounds"] < M.MAX_SPLIT_ROUNDS and it["collapse_rounds"] < M.MAX_COLLAPSE_ROUNDS and it["flip_rounds"] < M.MAX_FLIP_ROUNDS
        dev = it["valence_dev"]
        assert len(dev) == it["flip_rounds"] + 1 and np.all(np.diff(dev[:it["flip_rounds"] + 1]) < 0), dev
        work += it["split_rounds"] + it["collapse_rounds"] + it["flip_rounds"]
        assert it["projected"] >= it["relax_reverts"]
    assert work > 0


def _projected(name):
    make, L = INPUTS[name]
    v, f = make()
    info = {}
    v2, _, _ = Q.remesh_isotropic(v, f, L, info=info)
    on = info["on_surface"]
    assert on.sum() > 0
    return v, f, v2, on, float(np.spacing(np.float32(np.abs(v).max())))


@pytest.mark.parametrize("name", ["sphere", "torus", "grid"])
def test_reference_projected_vertices_lie_on_the_input_surface(name):
    """Every vertex the last relaxation moved and did not put back is the fp32 rounding of a point of the input surface: its exhaustive
    distance to the input mesh is at most 4 ulp (fp32) of the largest coordinate magnitude (rounding moves a coordinate by half an ulp,
    three coordinates by sqrt(3) / 2 ulp together; the scan's own error is fp64)."""
    v, f, v2, on, ulp = _projected(name)
    d = np.sqrt(Q.closest(v, f, v2[on])[0])
    print(f"\n{name}: {int(on.sum())} of {len(v2)} vertices projected and kept, largest distance to the input {d.max():.3e}, 4 ulp {4 * ulp:.3e}")
    assert d.max() <= 4 * ulp


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_reference_projected_vertices_stay_within_the_input_sag(name):
    """A vertex on the input surface is no further from the analytic surface than the input mesh itself: at most the input's own sag
    (_sag: recomputed here, the largest distance over the points of the mesh) plus the 4 ulp of the rounding.
    Measured: sphere 0.0043315 against a sag of 0.0045284; torus 0.0130389 against 0.0130393.  On the torus the bare 12-lattice reads
    0.0130350: its nodes miss the deepest point of a face, which lies off the midpoint of the diagonal, and a projected vertex may sit
    right there."""
    v, f, v2, on, ulp = _projected(name)
    sag, lattice = _sag(name, v, f)
    far = _analytic(name, v2[on]).max()
    print(f"\n{name}: input sag {sag:.7f} (12-lattice alone {lattice:.7f}), projected vertices within {far:.7f}, rounding {4 * ulp:.1e}")
    assert lattice <= sag
    assert far <= sag + 4 * ulp


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_reference_projection_lowers_the_drift(name):
    """The largest distance of any output vertex from the analytic surface, 3 iterations: strictly smaller with the projection than
    with the unprojected rule run here on the same input.  Measured: sphere 0.02561 -> 0.02132, torus 0.02966 -> 0.02664:
    what is left comes from the vertices the last pass put back and from split and collapse midpoints, which are not projected."""
    make, L = INPUTS[name]
    v, f = make()
    plain = _analytic(name, M.remesh_isotropic(v, f, L)[0]).max()
    proj = _analytic(name, Q.remesh_isotropic(v, f, L)[0]).max()
    print(f"\n{name}: largest distance to the analytic surface {plain:.5f} unprojected, {proj:.5f} projected, input sag {_sag(name, v, f)[0]:.5f}")
    assert proj < plain


# ------------------------------------------------------------------------------------------------------- GPU: the device passes
def _bits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.gpu
def test_projected_remesh_is_bit_identical_to_the_restatement():
    """test_mesh_remesh.py's inputs; the second target length of every input runs in selected mode."""
    import torch
    from nerf2mesh_amd.mesh_remesh import remesh_isotropic
    for name, (v, f) in T._cases().items():
        mean = float(T._edge_lengths(v, f).mean())
        half = (np.asarray(v)[f].mean(1)[:, 1] > np.median(np.asarray(v)[:, 1])).astype(np.uint8)
        for L, sel in ((0.8 * mean, None), (1.3 * mean, half)):
            rstats, dstats = {}, {}
            ref = Q.remesh_isotropic(v, f, L, selected=sel, stats=rstats)
            dsel = None if sel is None else torch.from_numpy(sel).cuda()
            out = remesh_isotropic(*T._dev(v, f), L, selected=dsel, stats=dstats, project=True)
            T._same((name, L, sel is not None), out, ref)
            assert dstats == rstats, (name, L, dstats, rstats)
            if sel is not None:
                rv, rf, rs = ref
                assert np.array_equal(rv[rf[sel[rs] == 0]], np.asarray(v)[f[sel == 0]]), name


@pytest.mark.gpu
def test_project_false_is_the_default():
    import torch
    from nerf2mesh_amd.mesh_remesh import remesh_isotropic
    for name, (v, f) in T._cases().items():
        L = 1.3 * float(T._edge_lengths(v, f).mean())
        s0, s1 = {}, {}
        a = remesh_isotropic(*T._dev(v, f), L, stats=s0)
        b = remesh_isotropic(*T._dev(v, f), L, stats=s1, project=False)
        assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b)), name
        assert s0 == s1 and "projected" not in s0["iterations"][0], name


@pytest.mark.gpu
def test_projected_sphere_drifts_less_on_the_device():
    """48^3 marching-cubes sphere: closed 2-manifold, and the largest distance of a vertex from the analytic sphere is strictly smaller
    with the projection than without it."""
    from nerf2mesh_amd.mesh_remesh import remesh_isotropic
    radius = 0.7
    v, f = T._mc_sphere(48, radius)
    v0, f0 = v.cpu().numpy(), f.cpu().numpy()
    L = float(T._edge_lengths(v0, f0).mean()) * 1.5
    stats = {}
    plain, _, _ = remesh_isotropic(v, f, L)
    pv, pf, _ = remesh_isotropic(v, f, L, stats=stats, project=True)
    rv, rf = pv.cpu().numpy(), pf.cpu().numpy()
    assert T._manifold(rf) and R.euler(rv, rf) == 2
    T._sound(rv, rf)
    d_plain = np.abs(np.linalg.norm(plain.cpu().numpy().astype(np.float64), axis=1) - radius).max()
    d_proj = np.abs(np.linalg.norm(rv.astype(np.float64), axis=1) - radius).max()
    print(f"\nsphere {len(f0)} -> {len(rf)} faces: largest distance {d_plain:.5f} unprojected, {d_proj:.5f} projected; {stats}")
    assert d_proj < d_plain
    assert all(it["projected"] > 0 for it in stats["iterations"])


def _sdf_model(v, f):
    import torch
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    torch.manual_seed(0)
    model = NeRFNetwork(make_options(O=True, bound=1, dt_gamma=0, stage=1, sdf=True, refine_remesh_size=0.08)).cuda()
    model.init_stage1(torch.from_numpy(v), torch.from_numpy(f))
    return model


@pytest.mark.gpu
def test_refine_and_decimate_passes_the_projection_on():
    """--sdf: the re-meshing is the whole refinement.  NeRFRenderer.refine_and_decimate(remesh=True, remesh_project=True) equals the
    restatement and reports the projected vertices; remesh_project=False is remesh=True alone."""
    v, f = R.icosphere(3, 0.6)
    outs = []
    for kw in ({}, {"remesh_project": False}, {"remesh_project": True}):
        model = _sdf_model(v, f)
        assert model.opt.refine_decimate_ratio == 0 and model.opt.refine_size == 0
        outs.append((model.refine_and_decimate(remesh=True, **kw), model.vertices.cpu().numpy(), model.triangles.cpu().numpy()))
    (o0, v0, f0), (o1, v1, f1), (o2, v2, f2) = outs
    assert o0 == o1 and np.array_equal(v0.view(np.uint32), v1.view(np.uint32)) and np.array_equal(f0, f1) and "projected" not in o0["remesh"]
    stats = {}
    rv, rf, _ = Q.remesh_isotropic(v, f, 0.08, stats=stats)
    assert np.array_equal(f2, rf) and np.array_equal(v2.view(np.uint32), rv.view(np.uint32))
    assert o2["remesh"] == {"faces_before": len(f), "faces_after": len(rf), "projected": [it["projected"] for it in stats["iterations"]]}
    assert sum(o2["remesh"]["projected"]) > 0


@pytest.mark.gpu
def test_refine_mesh_passes_the_projection_on():
    import torch
    from nerf2mesh_amd import synthetic as S
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    from nerf2mesh_amd.trainer import Stage1Trainer
    v, f = R.icosphere(3, 0.6)
    want = _sdf_model(v, f).refine_and_decimate(remesh=True, remesh_project=True)
    torch.manual_seed(0)
    opt = make_options(O=True, bound=1, dt_gamma=0, stage=1, sdf=True, refine_remesh_size=0.08)
    tr = Stage1Trainer(NeRFNetwork(opt), opt, S.make_cameras(4, seed=0), torch.from_numpy(v), torch.from_numpy(f), torch.device("cuda"), H=32, W=32)
    got = tr.refine_mesh(remesh=True, remesh_project=True)
    assert got == want and "projected" in got["remesh"]
    assert int(tr.model.triangles.shape[0]) == want["after"]["faces"]
