"""Device mesh cleaning (nerf2mesh_amd/mesh_clean.py, csrc/meshclean.hip) against the sequential numpy restatement of the same rule
(tests/mesh_clean_ref.py): bit-identical outputs and statistics, the invariants the rule promises, and the opt-in cleaning of
export_stage0 (nerf/renderer.py:537, :653).  The CPU tests check the restatement itself on hand-built cases, one per rule."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_clean_ref as R  # noqa: E402

OFF = dict(v_pct=0, min_f=0, min_d=0, repair=False)


def _f32(x):
    return np.asarray(x, np.float32)


# ------------------------------------------------------------------------------------------------------- CPU: the restatement
def test_merge_threshold_is_strict():
    below = np.nextafter(np.float32(1), np.float32(0))
    dest, _ = R.merge_close(_f32([[0, 0, 0], [below, 0, 0]]), 1.0)
    assert dest.tolist() == [0, 0]
    dest, _ = R.merge_close(_f32([[0, 0, 0], [1, 0, 0]]), 1.0)
    assert dest.tolist() == [0, 1]


def test_merge_greedy_order_makes_c_a_seed():
    # a-b < r, b-c < r, a-c > r: a claims b, so c is not claimed and becomes a seed of its own
    dest, rounds = R.merge_close(_f32([[0, 0, 0], [0.8, 0, 0], [1.6, 0, 0]]), 1.0)
    assert dest.tolist() == [0, 0, 2]
    assert rounds == 3                     # a; then b (its seed decided); then c (its lower neighbour b decided)


def test_merge_through_clean_mesh_uses_percent_of_the_diagonal():
    # box diagonal 5 (3-4-5 triangle); v_pct = 2 -> r = 0.1: vertex 3 (0.05 from vertex 0) merges, the face through it degenerates
    v = _f32([[0, 0, 0], [3, 0, 0], [0, 4, 0], [0.05, 0, 0], [1, 1, 0]])
    f = np.asarray([[0, 1, 2], [0, 3, 4], [3, 1, 4]], np.int32)
    rv, rf, src, st = R.clean_mesh(v, f, v_pct=2, min_f=0, min_d=0, repair=False)
    assert st["merged"] == 1 and st["degenerate"] == 1
    assert rf.tolist() == [[0, 1, 2], [0, 1, 3]] and src.tolist() == [0, 2]
    assert np.array_equal(rv, v[[0, 1, 2, 4]])


def test_duplicate_faces_either_orientation_keep_the_lowest_id():
    v = _f32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]])
    f = np.asarray([[1, 3, 2], [0, 1, 2], [2, 1, 0], [1, 2, 0]], np.int32)
    _, rf, src, st = R.clean_mesh(v, f, **OFF)
    assert src.tolist() == [0, 1] and st["duplicate"] == 2


def test_collinear_face_is_null():
    v = _f32([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0]])
    f = np.asarray([[0, 1, 2], [0, 1, 3], [1, 1, 3]], np.int32)      # a collinear face and one with a repeated corner
    _, rf, src, st = R.clean_mesh(v, f, **OFF)
    assert src.tolist() == [1] and st["null"] == 2


def _fan(n, centre, radius=1.0):
    """An open fan of n triangles around a centre vertex (one component, n faces)."""
    a = np.linspace(0, np.pi, n + 1)
    v = np.concatenate([[centre], np.stack([centre[0] + radius * np.cos(a), centre[1] + radius * np.sin(a), np.full(n + 1, centre[2])], 1)])
    f = np.asarray([[0, i + 1, i + 2] for i in range(n)])
    return _f32(v), f


def _join(*meshes):
    vs, fs, off = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(np.asarray(f) + off)
        off += len(v)
    return np.concatenate(vs), np.concatenate(fs).astype(np.int32)


def test_components_of_7_and_8_faces_with_min_f_8():
    v, f = _join(_fan(7, [0, 0, 0]), _fan(8, [5, 0, 0]))
    rv, rf, src, st = R.clean_mesh(v, f, v_pct=0, min_f=8, min_d=0, repair=False)
    assert src.tolist() == list(range(7, 15))
    assert st["components"] == 2 and st["size_components"] == 1 and st["size_faces"] == 7


def test_component_just_under_and_just_over_the_diameter_threshold():
    # mesh box [0, 3] x [0, 4] (diagonal 5); the small triangle's box diagonal is exactly 0.625 = 12.5 % of it
    v = _f32([[0, 0, 0], [3, 0, 0], [0, 4, 0], [1, 1, 0], [1.375, 1, 0], [1, 1.5, 0]])
    f = np.asarray([[0, 1, 2], [3, 4, 5]], np.int32)
    _, _, src, st = R.clean_mesh(v, f, v_pct=0, min_f=0, min_d=12.5, repair=False)
    assert src.tolist() == [0, 1] and st["diameter_components"] == 0          # 0.625 < 0.625 is false: kept
    _, _, src, st = R.clean_mesh(v, f, v_pct=0, min_f=0, min_d=12.6, repair=False)
    assert src.tolist() == [0] and st["diameter_components"] == 1 and st["diameter_faces"] == 1


def test_three_face_fin_edge_loses_its_smallest_face():
    v = _f32([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, 0, 2], [0.5, -3, 0]])
    f = np.asarray([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int32)               # double areas 1, 2, 3 on the edge (0, 1)
    _, rf, src, st = R.clean_mesh(v, f, v_pct=0, min_f=0, min_d=0, repair=True)
    assert src.tolist() == [1, 2] and st["nonmanifold_faces"] == 1
    assert st["nonmanifold_rounds"] == 3                # each face on the edge waits for the smaller ones
    assert R.edge_face_counts(rf).max() == 2


def test_bowtie_vertex_moves_its_first_fan_to_a_new_vertex():
    v = _f32([[0, 0, 0], [1, 0, 0], [1, 1, 0], [-1, 0, 0], [-1, -1, 0]])
    f = np.asarray([[0, 1, 2], [3, 0, 4]], np.int32)
    rv, rf, src, st = R.clean_mesh(v, f, v_pct=0, min_f=0, min_d=0, repair=True)
    assert st["split_vertices"] == 1
    assert rf.tolist() == [[5, 1, 2], [3, 0, 4]] and np.array_equal(rv[5], rv[0]) and np.array_equal(rv[:5], v)
    assert (R.fan_counts(rf, len(rv))[rf.reshape(-1)] == 1).all()


def test_three_fan_vertex_splits_once():
    v = _f32([[0, 0, 0], [1, 0, 0], [1, 1, 0], [-1, 0, 0], [-1, -1, 0], [0, 1, 1], [0, 0, 1]])
    f = np.asarray([[0, 1, 2], [3, 0, 4], [5, 6, 0]], np.int32)
    rv, rf, _, st = R.clean_mesh(v, f, v_pct=0, min_f=0, min_d=0, repair=True)
    assert st["split_vertices"] == 1 and len(rv) == 8
    assert rf[0].tolist() == [7, 1, 2]
    assert R.fan_counts(rf, len(rv))[0] == 2                                  # still non-manifold: one split per vertex


def test_empty_and_everything_removed():
    rv, rf, src, st = R.clean_mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert rv.shape == (0, 3) and rf.shape == (0, 3) and src.shape == (0,)
    v, f = _join(_fan(3, [0, 0, 0]), _fan(2, [4, 0, 0]))
    rv, rf, src, st = R.clean_mesh(v, f)
    assert rv.shape == (0, 3) and rf.shape == (0, 3) and src.shape == (0,) and st["size_faces"] == 5


def test_clean_mesh_arguments_checked_before_any_device_work():
    import torch
    from nerf2mesh_amd.mesh_clean import clean_mesh
    v, f = torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="remesh"):
        clean_mesh(v, f, remesh=True)
    with pytest.raises(ValueError, match=">= 0"):
        clean_mesh(v, f, v_pct=-1)
    with pytest.raises(ValueError, match=">= 0"):
        clean_mesh(v, f, min_d=-0.5)
    with pytest.raises(RuntimeError, match="CUDA"):
        clean_mesh(v, f)


def test_clean_options_have_the_reference_defaults():
    from nerf2mesh_amd.options import make_options
    o = make_options(O=True)
    assert (o.clean_min_f, o.clean_min_d) == (8, 5)


# ------------------------------------------------------------------------------------------------------- GPU: the device passes
def _dev(v, f):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(f, np.int32)).cuda()


def _mc(vol, iso, R_):
    from nerf2mesh_amd.marching_cubes import marching_cubes
    v, f = marching_cubes(vol, iso, div=R_ - 1.0, mul=2.0, add=-1.0)
    return v.cpu().numpy(), f.cpu().numpy()


def _sphere_volume(R_, radius=0.7):
    import torch
    g = torch.linspace(-1, 1, R_, device="cuda")
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    return radius - torch.sqrt(x * x + y * y + z * z)


def _lego_volume(R_):
    import torch
    from nerf2mesh_amd import synthetic as S
    g = torch.linspace(-1, 1, R_, device="cuda")
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    d = torch.full_like(x, 1e9)
    for b in S.boxes("cuda")[:, :6]:
        q = torch.stack([(x - (b[0] + b[3]) / 2).abs() - (b[3] - b[0]) / 2, (y - (b[1] + b[4]) / 2).abs() - (b[4] - b[1]) / 2,
                         (z - (b[2] + b[5]) / 2).abs() - (b[5] - b[2]) / 2])
        d = torch.minimum(d, q.clamp(min=0).norm(dim=0) + q.max(0).values.clamp(max=0))
    return 50.0 * torch.sigmoid(-d * R_)


def with_floaters(v, f, n=40, seed=0, scale=0.02):
    """n small closed blobs (20-face icospheres) and n two-face slivers at random places inside the mesh's box."""
    rng = np.random.default_rng(seed)
    lo, hi = v.min(0), v.max(0)
    bv, bf = R.icosphere(0, scale)
    meshes = [(v, f)]
    for _ in range(n):
        c = lo + rng.random(3) * (hi - lo)
        meshes.append((_f32(bv + c), bf))
        meshes.append((_f32(c + rng.random((4, 3)) * scale), np.asarray([[0, 1, 2], [0, 2, 3]])))
    return _join(*meshes)


def jittered_patch(n=40, seed=0):
    """Planar patch with every vertex jittered, plus a seam: the column j = n // 2 duplicated within 1e-3 and the faces right of it
    re-pointed to the copies (near-coincident vertices)."""
    rng = np.random.default_rng(seed)
    v, f = R.grid_patch(n)
    v = v + _f32(rng.uniform(-1e-3, 1e-3, v.shape)) * np.float32([1, 1, 0])
    col = np.nonzero(np.isclose(v[:, 1], (n // 2) / 16, atol=2e-3))[0]
    copies = _f32(v[col] + rng.uniform(-5e-4, 5e-4, (len(col), 3)))
    remap = np.arange(len(v))
    remap[col] = len(v) + np.arange(len(col))
    right = v[f].mean(1)[:, 1] > (n // 2) / 16
    f = f.copy()
    f[right] = remap[f[right]]
    return _f32(np.concatenate([v, copies])), f.astype(np.int32)


def bowties(n=6):
    out = []
    for i in range(n):
        c = np.float32([3 * i, 0, 0])
        fan_a = _fan(4, c, 1.0)
        fan_b = (_f32(fan_a[0] * np.float32([1, -1, 1]) + np.float32([0, 0, 0.5 * (i % 2)])), fan_a[1])
        v, f = _join(fan_a, fan_b)
        f[f == 6] = 0                                          # the second fan's centre is the first's: two fans at one vertex
        out.append((v, f))
    return _join(*out)


_CASES = {}


def _cases():
    if not _CASES:
        sv, sf = _mc(_sphere_volume(24), 0.0, 24)
        _CASES["mc sphere + floaters"] = (with_floaters(sv, sf), [dict(), dict(v_pct=0), dict(repair=False),
                                                                  dict(min_d=0)])
        tv, tf = R.torus(32, 16)
        tf2 = np.concatenate([tf, tf[::7], tf[3::11][:, ::-1], [[0, 0, 1]]]).astype(np.int32)   # + a repeated corner
        _CASES["torus, duplicated and reversed faces"] = ((tv, tf2), [dict(), dict(v_pct=0, min_f=0, min_d=0)])
        _CASES["jittered patch"] = (jittered_patch(), [dict(v_pct=1), dict(v_pct=0.1), dict(v_pct=0.1, repair=False)])
        iv, i_f = R.icosphere(2)
        fin = R.with_fin(*R.with_fin(iv, i_f))
        _CASES["with_fin"] = (fin, [dict(), dict(v_pct=0, min_f=0, min_d=0)])
        _CASES["bowties"] = (bowties(), [dict(v_pct=0, min_f=0, min_d=0), dict(v_pct=0.5, min_f=0, min_d=0)])
        _CASES["lego boxes 128"] = (_mc(_lego_volume(128), 10.0, 128), [dict(), dict(v_pct=0)])
    return _CASES


def _same(out, ref, st, name):
    dv, df, ds = out
    rv, rf, rs, rst = ref
    assert str(df.dtype) == "torch.int32" and str(ds.dtype) == "torch.int64", name
    assert df.shape == rf.shape and np.array_equal(df.cpu().numpy(), rf), name
    assert dv.shape == rv.shape and np.array_equal(dv.cpu().numpy().view(np.uint32), rv.view(np.uint32)), name
    assert np.array_equal(ds.cpu().numpy(), rs), name
    assert st == rst, (name, st, rst)


@pytest.mark.gpu
def test_clean_mesh_is_bit_identical_to_the_restatement():
    from nerf2mesh_amd.mesh_clean import clean_mesh
    for name, ((v, f), params) in _cases().items():
        assert len(v) < 100_000, name
        for kw in params:
            st = {}
            out = clean_mesh(*_dev(v, f), stats=st, **kw)
            ref = R.clean_mesh(v, f, **kw)
            print(f"\n{name} {kw}: {len(f)} -> {len(ref[1])} faces, {st}")
            _same(out, ref, st, f"{name} {kw}")


@pytest.mark.gpu
def test_each_rule_fires_on_the_device_cases():
    """The bit-exact cases above exercise every step (so equality is not vacuous)."""
    seen = dict.fromkeys(R.STAT_KEYS, 0)
    for name, ((v, f), params) in _cases().items():
        for kw in params:
            for k, x in R.clean_mesh(v, f, **kw)[3].items():
                seen[k] += x
    assert all(seen[k] > 0 for k in R.STAT_KEYS if k != "unreferenced"), seen


def _invariants(v, f, src, min_f, min_d, repair, mesh_diag, n_split):
    f = np.asarray(f)
    assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 2] != f[:, 0]).all()
    assert len(np.unique(np.sort(f, 1), axis=0)) == len(f)
    assert (R._cross(v, f) != 0).any(1).all()
    assert np.all(np.diff(src) > 0)
    assert len(np.unique(f)) == len(v)                          # no unreferenced vertex
    if not repair:
        # (the repair runs after the component filters, as in the reference: deleting a non-manifold face can split a component)
        label = R.components(f.astype(np.int64), len(v))
        count = np.bincount(label)
        assert count[np.unique(label)].min() >= min_f
        for r in np.unique(label):
            p = v[f[label == r].reshape(-1)].astype(np.float64)
            assert np.linalg.norm(p.max(0) - p.min(0)) >= min_d / 100 * mesh_diag * (1 - 1e-9)
    else:
        assert R.edge_face_counts(f).max() <= 2
        # one split per vertex: only a vertex that had three or more fans may still have more than one
        assert int((R.fan_counts(f, len(v)) > 1).sum()) <= n_split


@pytest.mark.gpu
def test_larger_meshes_invariants_determinism_and_decimation():
    import torch
    from nerf2mesh_amd.mesh_clean import clean_mesh
    from nerf2mesh_amd.mesh_simplify import decimate
    lv, lf = _mc(_lego_volume(256), 10.0, 256)
    lv, lf = with_floaters(lv, lf, n=300, seed=1)
    lv, lf = R.with_fin(lv, lf.astype(np.int32))
    for v, f, kw in ((lv, lf, dict()), (lv, lf, dict(v_pct=0)), (lv, lf, dict(repair=False)),
                     (*_mc(_sphere_volume(200), 0.0, 200), dict(repair=False))):
        dv, df = _dev(v, f)
        st = {}
        out = clean_mesh(dv, df, stats=st, **kw)
        print(f"\n{len(f)} faces {kw}: -> {out[1].shape[0]}, {st}")
        rv, rf, rs = (x.cpu().numpy() for x in out)
        mesh_diag = float(np.linalg.norm(v.max(0).astype(np.float64) - v.min(0)))
        _invariants(rv, rf, rs, 8, 5, kw.get("repair", True), 0.9 * mesh_diag, st["split_vertices"])
        again = clean_mesh(dv, df, **kw)
        assert torch.equal(out[1], again[1]) and torch.equal(out[0].view(torch.int32), again[0].view(torch.int32))
        assert torch.equal(out[2], again[2])
        target = out[1].shape[0] // 3
        _, tf, _ = decimate(out[0], out[1], target)           # passes decimate's input check (three distinct corners)
        assert 0 < tf.shape[0] <= target


@pytest.mark.gpu
def test_bad_inputs_raise():
    import torch
    from nerf2mesh_amd.mesh_clean import clean_mesh
    v, f = R.icosphere(1)
    with pytest.raises(RuntimeError, match="CUDA"):
        clean_mesh(torch.from_numpy(v), torch.from_numpy(f))
    dv, df = _dev(v, f)
    with pytest.raises(ValueError, match="float32"):
        clean_mesh(dv.double(), df)
    with pytest.raises(ValueError, match="int32 or int64"):
        clean_mesh(dv, df.float())
    with pytest.raises(ValueError, match="indices"):
        clean_mesh(dv, df + 1000)
    with pytest.raises(NotImplementedError):
        clean_mesh(dv, df, remesh=True)
    # a repeated corner is accepted (it leaves as a degenerate or null face)
    rep = torch.cat([df, torch.tensor([[0, 0, 1]], dtype=torch.int32, device="cuda")])
    st = {}
    _, cf, src = clean_mesh(dv, rep, v_pct=0, stats=st)
    assert cf.shape[0] == df.shape[0] and st["null"] == 1 and int(src.max()) == df.shape[0] - 1
    ev, ef, es = clean_mesh(dv[:0], df[:0])
    assert ev.shape == (0, 3) and ef.shape == (0, 3) and es.shape == (0,)
