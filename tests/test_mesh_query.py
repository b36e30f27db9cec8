"""Closest-point queries on a mesh (nerf2mesh_amd/mesh_query.py, csrc/meshquery.hip): the device hierarchy
against the exhaustive fp64 scan of tests/mesh_query_ref.py, bit for bit -- squared distance, face id and closest point -- and the
mesh-to-mesh distance built on it.  The CPU tests check the scan itself."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_query_ref as Q  # noqa: E402
import mesh_simplify_ref as R  # noqa: E402
import test_mesh_remesh as T  # noqa: E402


def _edge_midpoints(v, f):
    e, _, _ = R.edges_of(np.asarray(f), len(v))
    p = np.asarray(v, np.float64)
    return (p[e[:, 0]] + p[e[:, 1]]) * 0.5


# ------------------------------------------------------------------------------------------------------- CPU: the scan
@pytest.mark.parametrize("name", ["sphere", "torus", "grid", "cube"])
def test_reference_scan_is_zero_at_the_vertices(name):
    v, f = {"sphere": lambda: R.icosphere(2), "torus": lambda: R.torus(16, 8), "grid": lambda: R.grid_patch(8), "cube": T.cube}[name]()
    d2, face, hit = Q.closest(v, f, v)
    assert np.all(d2 == 0) and np.array_equal(hit, v.astype(np.float64))
    first = np.full(len(v), len(f))
    np.minimum.at(first, np.asarray(f).reshape(-1), np.repeat(np.arange(len(f)), 3))
    assert np.array_equal(face, first)                           # the lowest face id among the vertex's faces


def test_reference_scan_breaks_ties_by_face_id():
    """The dyadic cube: its centre is equally far (exactly) from the six faces' centres, an edge midpoint lies on two faces, a vertex
    on four to eight."""
    v, f = T.cube()
    d2, face, hit = Q.closest(v, f, np.zeros((1, 3)))
    assert d2[0] == 0.25 and np.abs(hit[0]).max() == 0.5 and np.abs(hit[0]).sum() == 0.5
    each = np.array([Q.closest(v, f[i:i + 1], np.zeros((1, 3)))[0][0] for i in range(len(f))])
    assert (each == 0.25).sum() >= 6 and face[0] == np.nonzero(each == 0.25)[0][0]
    mid = _edge_midpoints(v, f)
    d2, face, hit = Q.closest(v, f, mid)
    assert np.all(d2 == 0) and np.array_equal(hit, mid)
    e, _, c2e = R.edges_of(f, len(v))
    first = np.full(len(e), len(f))
    np.minimum.at(first, c2e.reshape(-1), np.repeat(np.arange(len(f)), 3))
    assert np.array_equal(face, first)                           # of the edge's two faces, the lower id


def test_reference_scan_leaves_out_what_does_not_count():
    v, f = R.icosphere(1)
    pts = np.random.default_rng(0).normal(size=(64, 3))
    want = Q.closest(v, f, pts)
    # a face with a repeated index in front: ids shift by one, nothing else changes
    d2, face, hit = Q.closest(v, np.concatenate([[[0, 0, 1]], f]), pts)
    assert np.array_equal(d2, want[0]) and np.array_equal(face, want[1] + 1) and np.array_equal(hit, want[2])
    # a face with a NaN corner never wins
    v2 = np.concatenate([v, [[np.nan, 0, 0]]]).astype(np.float32)
    d2, face, hit = Q.closest(v2, np.concatenate([[[0, 1, len(v)]], f]), pts)
    assert np.array_equal(d2, want[0]) and np.array_equal(face, want[1] + 1)
    d2, face, hit = Q.closest(v, f[:0], pts)
    assert np.all(np.isinf(d2)) and np.all(face == -1) and np.all(np.isnan(hit))


# ------------------------------------------------------------------------------------------------------- GPU: the device index
def _meshes():
    out = {"sphere": R.icosphere(3), "torus": R.torus(32, 16), "grid": R.grid_patch(16), "non-manifold": R.with_fin(*R.icosphere(3))}
    v, f = T._mc_sphere(48)
    out["mc sphere"] = (v.cpu().numpy(), f.cpu().numpy())
    return out


def _queries(v, f, n=2048, seed=0):
    """uniform in 1.6 x the box, on the surface, the vertices and edge midpoints, far (100 x the box), fp64 points that fp32 cannot hold."""
    rng = np.random.default_rng(seed)
    p = np.asarray(v, np.float64)
    lo, hi = p.min(0), p.max(0)
    c, h = (lo + hi) * 0.5, np.maximum((hi - lo) * 0.5, 1e-3)
    k = n // 8
    box = c + (rng.random((2 * k, 3)) * 2 - 1) * 1.6 * h
    w = rng.dirichlet(np.ones(3), 2 * k)
    tri = p[np.asarray(f)[rng.integers(0, len(f), 2 * k)]]
    surf = np.einsum("ij,ijk->ik", w, tri)
    verts = p[rng.integers(0, len(p), k)]
    mids = _edge_midpoints(v, f)
    mids = mids[rng.integers(0, len(mids), k)]
    far = c + (rng.random((k, 3)) * 2 - 1) * 100 * h
    fine = c + (rng.random((n - 7 * k, 3)) * 2 - 1) * h * (1 + 2.0 ** -40)
    fine = np.where(fine.astype(np.float32).astype(np.float64) == fine, fine * (1 + 2.0 ** -30), fine)
    pts = np.concatenate([box, surf, verts, mids, far, fine])
    assert len(pts) == n and not np.array_equal(fine.astype(np.float32).astype(np.float64), fine)
    return pts


def _same(got, want, what):
    d2, face, hit = (x.cpu().numpy() for x in got)
    assert np.array_equal(face, want[1]), what
    assert np.array_equal(d2.view(np.uint64), want[0].view(np.uint64)), what
    assert np.array_equal(hit.view(np.uint64), want[2].view(np.uint64)), what


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sphere", "torus", "grid", "non-manifold", "mc sphere"])
def test_closest_equals_the_numpy_scan(name):
    import torch
    from nerf2mesh_amd.mesh_query import MeshIndex
    v, f = _meshes()[name]
    pts = _queries(v, f)
    want = Q.closest(v, f, pts)
    assert np.all(want[1] >= 0) and (want[0] == 0).sum() >= 256          # the vertices and the edge midpoints
    index = MeshIndex(*T._dev(v, f))
    dpts = torch.from_numpy(pts).cuda()
    _same(index.closest(dpts), want, name)
    _same(index.closest(dpts, prune=False), want, name + ", every leaf")
    _same(index.closest(dpts, sort_queries=False), want, name + ", unsorted")
    # float32 points are the same points
    p32 = pts.astype(np.float32)
    _same(index.closest(torch.from_numpy(p32).cuda()), Q.closest(v, f, p32), name + ", float32")


@pytest.mark.gpu
def test_closest_ties_and_faces_that_do_not_count():
    import torch
    from nerf2mesh_amd.mesh_query import MeshIndex
    v, f = T.cube()
    pts = np.concatenate([np.zeros((1, 3)), _edge_midpoints(v, f), v.astype(np.float64)])
    _same(MeshIndex(*T._dev(v, f)).closest(torch.from_numpy(pts).cuda()), Q.closest(v, f, pts), "cube")
    # repeated indices, a NaN corner, an unreferenced vertex far away
    v, f = R.icosphere(2)
    v2 = np.concatenate([v, [[np.nan, 0, 0], [50, 50, 50]]]).astype(np.float32)
    f2 = np.concatenate([[[3, 3, 5]], f[:40], [[0, 1, len(v)], [7, 9, 7]], f[40:]]).astype(np.int32)
    pts = _queries(v, f, 512, seed=1)
    want = Q.closest(v2, f2, pts)
    assert not np.isin(want[1], [0, 41, 42]).any()
    _same(MeshIndex(*T._dev(v2, f2)).closest(torch.from_numpy(pts).cuda()), want, "faces left out")
    # one face, no indexed face, no face, no point
    for ff in (f[:1], np.array([[1, 1, 2]], np.int32), f[:0]):
        got = MeshIndex(*T._dev(v, ff)).closest(torch.from_numpy(pts).cuda())
        want = Q.closest(v, ff, pts)
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
        assert np.array_equal(got[2].cpu().numpy(), want[2], equal_nan=True)
    d2, face, hit = MeshIndex(*T._dev(v, f)).closest(torch.zeros(0, 3, device="cuda"))
    assert d2.shape == (0,) and face.shape == (0,) and hit.shape == (0, 3)
    # a NaN query is at no distance from anything
    d2, face, hit = MeshIndex(*T._dev(v, f)).closest(torch.tensor([[float("nan"), 0, 0]], device="cuda"))
    assert np.isinf(d2.item()) and face.item() == -1


@pytest.mark.gpu
def test_pruned_equals_exhaustive_on_the_large_sphere():
    """256^3 marching-cubes sphere (300 524 faces), 2^16 queries: the traversal against the device scan of every leaf."""
    import torch
    from nerf2mesh_amd.mesh_query import MeshIndex, sample_surface
    v, f = T._mc_sphere(256)
    assert f.shape[0] == 300524
    g = torch.Generator(device="cuda").manual_seed(0)
    n = 1 << 16
    surf, _ = sample_surface(v, f, n // 2, g)
    box = (torch.rand(n // 4, 3, dtype=torch.float64, device="cuda", generator=g) * 2 - 1) * 1.2
    far = (torch.rand(n // 8, 3, dtype=torch.float64, device="cuda", generator=g) * 2 - 1) * 100
    own = v[torch.randint(0, v.shape[0], (n // 8,), device="cuda", generator=g)].double()
    pts = torch.cat([surf, box, far, own])
    assert pts.shape[0] == n
    index = MeshIndex(v, f)
    a = index.closest(pts)
    b = index.closest(pts, prune=False)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y)
    assert int(a[1].min()) >= 0 and float(a[0][-n // 8:].max()) == 0.0


@pytest.mark.gpu
def test_two_builds_and_a_shuffle_agree():
    import torch
    from nerf2mesh_amd.mesh_query import MeshIndex
    v, f = T._mc_sphere(48)
    pts = torch.from_numpy(_queries(v.cpu().numpy(), f.cpu().numpy(), 4096, seed=2)).cuda()
    a = MeshIndex(v, f).closest(pts)
    second = MeshIndex(v, f)
    b = second.closest(pts)
    perm = torch.randperm(pts.shape[0], device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    c = second.closest(pts[perm])
    for x, y, z in zip(a, b, c):
        bits = (lambda t: t.view(torch.int64)) if x.dtype == torch.float64 else (lambda t: t)
        assert torch.equal(bits(x), bits(y)) and torch.equal(bits(x)[perm], bits(z))


@pytest.mark.gpu
def test_mesh_distance():
    import torch
    from nerf2mesh_amd.mesh_query import mesh_distance, sample_surface
    v, f = T._dev(*R.icosphere(3))
    g = torch.Generator(device="cuda").manual_seed(0)
    pts, face = sample_surface(v, f, 4096, g)
    assert pts.dtype == torch.float64 and pts.shape == (4096, 3) and face.dtype == torch.int64 and int(face.min()) >= 0 and int(face.max()) < f.shape[0]
    tri = v.double()[f.long()[face]]
    n = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert float((((pts - tri[:, 0]) * n).sum(1).abs() / n.norm(dim=1)).max()) < 1e-12          # in the plane of its face
    area = torch.linalg.cross(v[f.long()[:, 1]] - v[f.long()[:, 0]], v[f.long()[:, 2]] - v[f.long()[:, 0]]).norm(dim=1).double()
    share = torch.bincount(face, minlength=f.shape[0]).double() / 4096
    assert float((share - area / area.sum()).abs().max()) < 5 * float((area / area.sum()).max() / 4096) ** 0.5   # 5 sigma of a binomial share
    # a mesh against itself: 0 up to the rounding of the sample's own barycentric sum -- per coordinate three products and two sums of
    # at most half an ulp (fp64) of the largest coordinate, 1 here: 2.5 ulp, 4.4 ulp for the three together; 8 ulp with the query's own
    same = mesh_distance(v, f, v, f, n=2048, generator=g)
    ulp = float(np.spacing(1.0))
    print(f"\nself distance: {same['max_ab']:.3e} {same['max_ba']:.3e}, 8 ulp {8 * ulp:.3e}")
    assert 0 <= same["mean_ab"] <= same["max_ab"] <= 8 * ulp and 0 <= same["mean_ba"] <= same["max_ba"] <= 8 * ulp
    assert same["hausdorff"] <= 8 * ulp and same["chamfer"] <= 8 * ulp
    # against a translated copy: a point of a face moves by a convex combination of its corners' moves, so no sample is further than
    # the largest move of a vertex (|t| up to the fp32 rounding of v + t)
    t = torch.tensor([0.03, -0.02, 0.01], device="cuda")
    out = mesh_distance(v, f, v + t, f, n=2048, generator=g)
    tn = float(((v + t).double() - v.double()).norm(dim=1).max())
    assert abs(tn - float(t.double().norm())) < 1e-6
    for k in ("mean_ab", "mean_ba", "max_ab", "max_ba", "chamfer", "hausdorff"):
        assert 0 < out[k] <= tn + 8 * ulp, k
    assert out["chamfer"] == 0.5 * (out["mean_ab"] + out["mean_ba"]) and out["hausdorff"] == max(out["max_ab"], out["max_ba"])
    # the values are the numpy scan's on the returned samples
    vb = (v + t).cpu().numpy()
    d_ab = np.sqrt(Q.closest(vb, f.cpu().numpy(), out["samples_a"].cpu().numpy())[0])
    d_ba = np.sqrt(Q.closest(v.cpu().numpy(), f.cpu().numpy(), out["samples_b"].cpu().numpy())[0])
    assert np.allclose(out["d_ab"].cpu().numpy(), d_ab, rtol=4e-16, atol=0) and np.allclose(out["d_ba"].cpu().numpy(), d_ba, rtol=4e-16, atol=0)
    assert np.isclose(out["max_ab"], d_ab.max(), rtol=4e-16) and np.isclose(out["max_ba"], d_ba.max(), rtol=4e-16)
    assert np.isclose(out["mean_ab"], d_ab.mean(), rtol=1e-12) and np.isclose(out["mean_ba"], d_ba.mean(), rtol=1e-12)


@pytest.mark.gpu
def test_bad_inputs_raise():
    import torch
    from nerf2mesh_amd.mesh_query import MeshIndex, mesh_distance, sample_surface
    v, f = R.icosphere(1)
    with pytest.raises(RuntimeError, match="CUDA"):
        MeshIndex(torch.from_numpy(v), torch.from_numpy(f))
    dv, df = T._dev(v, f)
    with pytest.raises(ValueError, match="float32"):
        MeshIndex(dv.double(), df)
    with pytest.raises(ValueError, match=r"\[F, 3\]"):
        MeshIndex(dv, df.reshape(-1))
    with pytest.raises(ValueError, match=r"\[V, 3\]"):
        MeshIndex(dv[:, :2], df)
    bad = df.clone()
    bad[0, 0] = len(v)
    with pytest.raises(ValueError, match="indices"):
        MeshIndex(dv, bad)
    bad[0, 0] = -1
    with pytest.raises(ValueError, match="indices"):
        MeshIndex(dv, bad)
    index = MeshIndex(dv, df)
    with pytest.raises(RuntimeError, match="CUDA"):
        index.closest(torch.zeros(4, 3))
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        index.closest(torch.zeros(4, 2, device="cuda"))
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        index.closest(torch.zeros(4, 3, device="cuda", dtype=torch.float16))
    with pytest.raises(RuntimeError, match="CUDA"):
        sample_surface(torch.from_numpy(v), torch.from_numpy(f), 8)
    with pytest.raises(ValueError, match="no surface"):
        sample_surface(dv, df[:0], 8)
    with pytest.raises(ValueError, match="n must be"):
        mesh_distance(dv, df, dv, df, n=0)
