"""Device isotropic re-meshing (nerf2mesh_amd/mesh_remesh.py, csrc/meshremesh.hip) against the numpy restatement of the same rule
(tests/mesh_remesh_ref.py): bit-identical outputs, plus the invariants the rule promises.  The CPU tests check the
restatement itself on small meshes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_remesh_ref as M  # noqa: E402
import mesh_simplify_ref as R  # noqa: E402


def _manifold(f):
    return set(np.unique(R.edge_face_counts(f)).tolist()) == {2}


def _edge_lengths(v, f):
    e, _, _ = R.edges_of(np.asarray(f), len(v))
    p = np.asarray(v, np.float64)
    return np.linalg.norm(p[e[:, 0]] - p[e[:, 1]], axis=1)


def _boundary_loops(f):
    """Number of connected components of the boundary edges."""
    e, nf, _ = R.edges_of(np.asarray(f), int(np.asarray(f).max()) + 1)
    b = e[nf == 1]
    parent = {int(x): int(x) for x in np.unique(b)}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for x, y in b:
        parent[find(int(x))] = find(int(y))
    return len({find(x) for x in parent})


def _sound(v, f):
    """No face with a repeated vertex, no zero-area face."""
    f = np.asarray(f)
    assert np.all((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0]))
    p = np.asarray(v, np.float64)[f]
    assert np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1).min() > 0


def cube(threshold=0.15):
    """The cube [-0.5, 0.5]^3, 12 faces, midpoint-subdivided to edges of 0.088-0.125 (dyadic coordinates)."""
    v = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]],
                 np.int32)
    return R.subdivide_midpoint(v, f, threshold, iterations=4)


def _torus_distance(p, R_=1.0, r=0.35):
    return np.abs(np.sqrt((np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2) - R_) ** 2 + p[:, 2] ** 2) - r)


def _diag(v):
    return float(np.linalg.norm(np.ptp(np.asarray(v, np.float64), axis=0)))


# ------------------------------------------------------------------------------------------------------- CPU: the restatement
@pytest.mark.parametrize("name", ["sphere", "torus", "grid"])
def test_reference_topology_is_kept(name):
    v, f = {"sphere": lambda: R.icosphere(3), "torus": lambda: R.torus(32, 16), "grid": lambda: R.grid_patch(16)}[name]()
    L = {"sphere": 0.2, "torus": 0.15, "grid": 0.1}[name]
    v2, f2, src = M.remesh_isotropic(v, f, L)
    assert len(f2) != len(f)
    assert R.euler(v2, f2) == R.euler(v, f)
    _sound(v2, f2)
    if name == "grid":
        assert set(np.unique(R.edge_face_counts(f2)).tolist()) == {1, 2} and _boundary_loops(f2) == _boundary_loops(f) == 1
    else:
        assert _manifold(f2)
    assert src.min() >= 0 and src.max() < len(f)


@pytest.mark.parametrize("name", ["sphere", "torus", "grid", "half sphere"])
def test_reference_pass_invariants(name):
    """After the split pass no edge whose faces are all selected is longer than 4/3 L; after the collapse pass every such edge shorter than
    4/5 L fails the validity predicate; the valence deviation falls strictly from flip round to flip round."""
    v, f = {"sphere": lambda: R.icosphere(3), "torus": lambda: R.torus(32, 16), "grid": lambda: R.grid_patch(16),
            "half sphere": lambda: R.icosphere(3)}[name]()
    L = {"sphere": 0.2, "torus": 0.15, "grid": 0.04, "half sphere": 0.1}[name]
    sel = (v[f].mean(1)[:, 0] > 0).astype(np.uint8) if name == "half sphere" else None
    lo2, hi2 = M.thresholds(L)
    cos_f = M.cos_feature(30.0)
    seen = []

    def hook(stage, it, v, f, sel):
        seen.append(stage)
        if stage == "split":
            edges, _, c2e = R.edges_of(f, len(v))
            assert not M.split_marks(v, f, sel, hi2, edges, c2e).any()
            free = np.ones(len(edges), bool)
            free[c2e[sel == 0].reshape(-1)] = False
            p = v.astype(np.float64)
            d = p[edges[:, 1]] - p[edges[:, 0]]
            assert (d * d).sum(1)[free].max() <= hi2
        if stage == "collapse":
            keys, _, _ = M.collapse_keys(v, f, sel, lo2, hi2, cos_f)
            assert np.all(keys == M.NO_KEY)
    stats = {}
    M.remesh_isotropic(v, f, L, selected=sel, stats=stats, hook=hook)
    assert seen == ["split", "collapse", "flip", "relax"] * 3
    work = 0
    for it in stats["iterations"]:
        assert it["split_rounds"] < M.MAX_SPLIT_ROUNDS and it["collapse_rounds"] < M.MAX_COLLAPSE_ROUNDS and it["flip_rounds"] < M.MAX_FLIP_ROUNDS
        dev = it["valence_dev"]
        assert len(dev) == it["flip_rounds"] + 1 and np.all(np.diff(dev[:it["flip_rounds"] + 1]) < 0), dev
        work += it["split_rounds"] + it["collapse_rounds"] + it["flip_rounds"]
    assert work > 0


def test_reference_orientation_is_kept():
    v, f = R.icosphere(3)
    v2, f2, _ = M.remesh_isotropic(v, f, 0.2)
    p = v2.astype(np.float64)[f2]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert np.all((n * p.mean(1)).sum(1) > 0)
    assert R.signed_volume(v2, f2) > 0.9 * R.signed_volume(v, f)


@pytest.mark.parametrize("L", [0.1, 0.04])
def test_reference_flat_patch(L):
    """Input edges 0.0625-0.088: at L = 0.1 the collapse pass has work, at L = 0.04 the split pass."""
    n = 16
    v, f = R.grid_patch(n)
    stats = {}
    v2, f2, _ = M.remesh_isotropic(v, f, L, stats=stats)
    first = stats["iterations"][0]
    assert (first["collapse_rounds"] if L == 0.1 else first["split_rounds"]) > 0
    assert (len(f2) < len(f)) if L == 0.1 else (len(f2) > len(f))
    assert np.all(v2[:, 2] == 0)
    for c in (0, n, n * (n + 1), (n + 1) ** 2 - 1):
        assert np.any(np.all(v2 == v[c], axis=1)), c
    e, nf, _ = R.edges_of(f2, len(v2))
    b = v2[np.unique(e[nf == 1])]
    assert np.all((b[:, 0] == 0) | (b[:, 0] == 1) | (b[:, 1] == 0) | (b[:, 1] == 1))
    assert b.min() >= 0 and b.max() <= 1


def _check_cube(v, v2, f2):
    corners = v[(np.abs(v) == 0.5).all(1)]
    assert len(corners) == 8
    for c in corners:
        assert np.any(np.all(v2 == c, axis=1)), c
    assert np.all((np.abs(v2) == 0.5).any(1)) and np.abs(v2).max() == 0.5           # every vertex exactly on one of the 6 planes
    t = M.Topo(v2, np.asarray(f2, np.int64), np.ones(len(f2), np.uint8), M.cos_feature(30.0))
    fe = t.edges[t.efeat]
    assert len(fe) and set(np.unique(t.nf).tolist()) == {2}
    lines = {}
    for a, b in fe:
        pa, pb = v2[a], v2[b]
        fixed = (np.abs(pa) == 0.5) & (np.abs(pb) == 0.5) & (pa == pb)
        assert fixed.sum() == 2, (pa, pb)                        # both ends on the same edge line of the cube
        axis = int(np.nonzero(~fixed)[0][0])
        lines.setdefault((axis,) + tuple(pa[fixed].tolist()), []).append(sorted((float(pa[axis]), float(pb[axis]))))
    assert len(lines) == 12
    for segs in lines.values():                                  # covered from corner to corner, without a gap or an overlap
        segs.sort()
        assert segs[0][0] == -0.5 and segs[-1][1] == 0.5
        assert all(segs[i][1] == segs[i + 1][0] for i in range(len(segs) - 1))


def test_reference_cube_keeps_its_features():
    v, f = cube()
    le = _edge_lengths(v, f)
    assert 0.08 < le.min() and le.max() <= 0.15 and len(f) > 1000
    stats = {}
    v2, f2, _ = M.remesh_isotropic(v, f, 0.15, stats=stats)
    assert len(f2) < len(f) and _manifold(f2) and R.euler(v2, f2) == 2
    _sound(v2, f2)
    _check_cube(v, v2, f2)


def test_reference_selected_leaves_the_rest():
    v, f = R.icosphere(3)
    sel = (v[f].mean(1)[:, 0] > 0).astype(np.uint8)
    for L in (0.2, 0.1):
        v2, f2, src = M.remesh_isotropic(v, f, L, selected=sel)
        assert len(f2) != len(f) and _manifold(f2)
        assert np.array_equal(v2[f2[sel[src] == 0]], v[f[sel == 0]])   # unselected faces and their vertices, bit for bit, in order
        assert np.array_equal(src[sel[src] == 0], np.nonzero(sel == 0)[0])
        assert np.all(sel[src[sel[src] != 0]] != 0)


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_reference_surface_distance(name):
    """Output vertices against the analytic surface, 3 iterations.  The cap is 1 % of the input's bounding-box diagonal, the reference
    filter's own acceptance distance (`maxsurfdist`, default PercentageValue(1): an assumption about pymeshlab's default that cannot be
    checked without pymeshlab).  Measured with this restatement: sphere 0.0256 against 0.0346, torus 0.0297 against 0.0388."""
    if name == "sphere":
        v, f = R.icosphere(3)
        v2, _, _ = M.remesh_isotropic(v, f, 0.2)
        d = np.abs(np.linalg.norm(v2.astype(np.float64), axis=1) - 1.0)
    else:
        v, f = R.torus(32, 16)
        v2, _, _ = M.remesh_isotropic(v, f, 0.15)
        d = _torus_distance(v2.astype(np.float64))
    print(f"\n{name}: max distance {d.max():.5f}, cap {0.01 * _diag(v):.5f}")
    assert d.max() <= 0.01 * _diag(v)


def _quality(v, f, L):
    le = _edge_lengths(v, f)
    val = np.bincount(R.edges_of(np.asarray(f), len(v))[0].reshape(-1), minlength=len(v))
    val = val[val > 0]
    return le.std() / le.mean(), float(np.mean((le >= 0.8 * L) & (le <= 4.0 / 3.0 * L))), float(np.mean((val >= 5) & (val <= 7)))


def test_reference_regularity_improves():
    """icosphere(4) with the half x > 0 decimated to a quarter: the coefficient of variation of the edge lengths falls and the share of
    edges inside [4/5 L, 4/3 L] rises (L = the input's mean edge length).  The valence shares are printed, not asserted."""
    v, f = R.icosphere(4)
    sel = (v[f].mean(1)[:, 0] > 0).astype(np.uint8)
    v, f, _ = R.decimate(v, f, int(sel.sum()) // 4, selected=sel)
    assert _manifold(f)
    L = float(_edge_lengths(v, f).mean())
    cv0, in0, val0 = _quality(v, f, L)
    v2, f2, _ = M.remesh_isotropic(v, f, L)
    cv1, in1, val1 = _quality(v2, f2, L)
    print(f"\nfaces {len(f)} -> {len(f2)}, L {L:.4f}: cv {cv0:.3f} -> {cv1:.3f}, in range {in0:.3f} -> {in1:.3f}, valence 5-7 {val0:.3f} -> {val1:.3f}")
    assert _manifold(f2) and R.euler(v2, f2) == 2
    assert cv1 < cv0 and in1 > in0


def test_reference_trivial_cases_return_the_input():
    v, f = R.icosphere(1)
    for kw in ({"iterations": 0}, {"selected": np.zeros(len(f), np.uint8)}):
        v2, f2, src = M.remesh_isotropic(v, f, 0.1, **kw)
        assert np.array_equal(v2, v) and np.array_equal(f2, f) and np.array_equal(src, np.arange(len(f)))
    v2, f2, src = M.remesh_isotropic(v, f[:0], 0.1)
    assert np.array_equal(v2, v) and f2.shape == (0, 3) and src.shape == (0,)


# ------------------------------------------------------------------------------------------------------- GPU: the device passes
def _mc_sphere(R_=48, radius=0.7):
    import torch
    from nerf2mesh_amd.marching_cubes import marching_cubes
    g = torch.linspace(-1, 1, R_, device="cuda")
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    return marching_cubes(radius - torch.sqrt(x * x + y * y + z * z), 0.0, div=R_ - 1.0, mul=2.0, add=-1.0)


def _cases():
    from nerf2mesh_amd import synthetic as S
    out = {}
    v, f = _mc_sphere(24)
    out["mc sphere"] = (v.cpu().numpy(), f.cpu().numpy())
    out["torus"] = R.torus(32, 16)
    out["grid"] = R.grid_patch(16)
    sv, sf = S.scene_mesh(1500)
    out["scene_mesh"] = (sv.numpy().astype(np.float32), sf.numpy().astype(np.int32))
    out["non-manifold"] = R.with_fin(*R.icosphere(2))
    out["cube"] = cube()
    return out


def _dev(v, f):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v)).cuda(), torch.from_numpy(np.ascontiguousarray(f)).cuda()


def _same(name, dev_out, ref_out):
    (dv, df, ds), (rv, rf, rs) = dev_out, ref_out
    assert df.shape == rf.shape and np.array_equal(df.cpu().numpy(), rf), name
    assert dv.shape == rv.shape and np.array_equal(dv.cpu().numpy().view(np.uint32), np.asarray(rv, np.float32).view(np.uint32)), name
    assert np.array_equal(ds.cpu().numpy(), rs), name


@pytest.mark.gpu
def test_remesh_is_bit_identical_to_the_restatement():
    import torch
    from nerf2mesh_amd.mesh_remesh import remesh_isotropic
    for name, (v, f) in _cases().items():
        mean = float(_edge_lengths(v, f).mean())
        half = (np.asarray(v)[f].mean(1)[:, 1] > np.median(np.asarray(v)[:, 1])).astype(np.uint8)
        for L in (0.8 * mean, 1.3 * mean):
            for sel in (None, half):
                rstats, dstats = {}, {}
                ref = M.remesh_isotropic(v, f, L, selected=sel, stats=rstats)
                dsel = None if sel is None else torch.from_numpy(sel).cuda()
                out = remesh_isotropic(*_dev(v, f), L, selected=dsel, stats=dstats)
                _same((name, L, sel is not None), out, ref)
                assert dstats == rstats, (name, L, dstats, rstats)
                assert len(ref[1]) != len(f), name
                again = remesh_isotropic(*_dev(v, f), L, selected=dsel)
                assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
                           for a, b in zip(out, again)), name
                if sel is not None:
                    rv, rf, rs = ref
                    assert np.array_equal(rv[rf[sel[rs] == 0]], np.asarray(v)[f[sel == 0]]), name


@pytest.mark.gpu
def test_remeshed_sphere_invariants():
    """48^3 marching-cubes sphere (the restatement is too slow to be worth running here): closed 2-manifold, Euler characteristic,
    no degenerate or flipped face, vertices within 1 % of the bounding-box diagonal of the sphere, edge lengths more even, valence
    deviation falling strictly over the flip rounds, and no round cap hit."""
    from nerf2mesh_amd.mesh_remesh import remesh_isotropic
    radius = 0.7
    v, f = _mc_sphere(48, radius)
    v0, f0 = v.cpu().numpy(), f.cpu().numpy()
    L = float(_edge_lengths(v0, f0).mean()) * 1.5
    stats = {}
    dv, df, ds = remesh_isotropic(v, f, L, stats=stats)
    rv, rf = dv.cpu().numpy(), df.cpu().numpy()
    print(f"\nsphere {len(f0)} -> {len(rf)} faces, L {L:.4f}: {stats}")
    assert _manifold(rf) and R.euler(rv, rf) == R.euler(v0, f0) == 2
    _sound(rv, rf)
    p = rv.astype(np.float64)[rf]
    assert np.all((np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]) * p.mean(1)).sum(1) > 0)
    assert np.abs(np.linalg.norm(rv.astype(np.float64), axis=1) - radius).max() <= 0.01 * _diag(v0)
    cv0, in0, _ = _quality(v0, f0, L)
    cv1, in1, _ = _quality(rv, rf, L)
    assert cv1 < cv0 and in1 > in0, (cv0, cv1, in0, in1)
    for it in stats["iterations"]:
        assert it["split_rounds"] < 32 and it["collapse_rounds"] < 128 and it["flip_rounds"] < 128
        assert np.all(np.diff(it["valence_dev"]) < 0) or it["flip_rounds"] == 0
    s = ds.cpu().numpy()
    assert s.min() >= 0 and s.max() < len(f0)


@pytest.mark.gpu
def test_remesh_device_invariants_on_the_cube_and_the_patch():
    from nerf2mesh_amd.mesh_remesh import remesh_isotropic
    v, f = cube()
    dv, df, _ = remesh_isotropic(*_dev(v, f), 0.15)
    _check_cube(v, dv.cpu().numpy(), df.cpu().numpy())
    v, f = R.grid_patch(16)
    dv, df, _ = remesh_isotropic(*_dev(v, f), 0.1)
    rv = dv.cpu().numpy()
    assert np.all(rv[:, 2] == 0)
    for c in (0, 16, 16 * 17, 17 * 17 - 1):
        assert np.any(np.all(rv == v[c], axis=1)), c


@pytest.mark.gpu
def test_remesh_trivial_cases_return_the_input():
    import torch
    from nerf2mesh_amd.mesh_remesh import remesh_isotropic
    v, f = _dev(*R.icosphere(2))
    ar = torch.arange(f.shape[0], device="cuda")
    for kw in ({"iterations": 0}, {"selected": torch.zeros(f.shape[0], dtype=torch.bool, device="cuda")}):
        dv, df, ds = remesh_isotropic(v, f, 0.1, **kw)
        assert torch.equal(dv, v) and torch.equal(df, f) and torch.equal(ds, ar)
    dv, df, ds = remesh_isotropic(v, f[:0], 0.1)
    assert torch.equal(dv, v) and df.shape == (0, 3) and ds.shape == (0,)


@pytest.mark.gpu
def test_remesh_bad_inputs_raise():
    import torch
    from nerf2mesh_amd.mesh_remesh import remesh_isotropic
    v, f = R.icosphere(1)
    with pytest.raises(RuntimeError, match="CUDA"):
        remesh_isotropic(torch.from_numpy(v), torch.from_numpy(f), 0.1)
    dv, df = _dev(v, f)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="target_len"):
            remesh_isotropic(dv, df, bad)
    with pytest.raises(ValueError, match="iterations"):
        remesh_isotropic(dv, df, 0.1, iterations=-1)
    with pytest.raises(ValueError, match="float32"):
        remesh_isotropic(dv.double(), df, 0.1)
    with pytest.raises(ValueError, match=r"\[F, 3\]"):
        remesh_isotropic(dv, df.reshape(-1), 0.1)
    with pytest.raises(ValueError, match="selection"):
        remesh_isotropic(dv, df, 0.1, selected=torch.ones(df.shape[0], dtype=torch.float32, device="cuda"))
    with pytest.raises(RuntimeError, match="selection"):
        remesh_isotropic(dv, df, 0.1, selected=torch.ones(df.shape[0], dtype=torch.bool))
