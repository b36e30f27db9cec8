"""Device UV atlas (nerf2mesh_amd/uv_atlas.py, csrc/uvatlas.hip; rule: DESIGN.md section 4.13).

CPU: the sequential numpy restatement tests/uv_atlas_ref.py, one hand-built case per rule.  GPU: the device result equals the
restatement bit for bit; the stated guarantees (positive UV areas, density interval, no texel centre inside two faces) hold on a large
mesh, checked with torch ops that do not call the product's canvas kernels; the atlas carries a bake and an export end to end.
PARITY with xatlas stays UNPINNED (xatlas is not available here); nothing below claims it."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uv_atlas_ref as R  # noqa: E402


# ------------------------------------------------------------------------------------------------ CPU: the restatement, rule by rule
def _cos_to_label(v, f, label):
    n, da = R.face_frames(v, f)
    return R.dots(n)[np.arange(len(f)), label] / da


@pytest.mark.parametrize("subdivided, uv_vertices", [(False, 24), (True, 54)])   # 6 sides x 4 corners; 6 sides x 3 x 3 lattice points
def test_ref_cube_is_six_charts_at_uniform_density(subdivided, uv_vertices):
    v, f = R.cube()
    if subdivided:
        v, f = R.subdivide(v, f)
    st = {}
    H = W = 256
    vt, ft, vm = R.uv_atlas(v, f, H, W, stats=st)
    assert st["charts"] == 6 and st["uv_vertices"] == uv_vertices == len(vt) == len(vm)
    assert np.array_equal(vm[ft], f) and vt.min() >= 0 and vt.max() <= 1
    assert np.all(_cos_to_label(v, f, st["label"]) == 1.0)
    assert st["relax_changed"] == [0, 0, 0, 0] and st["evicted_faces"] == 0
    # vt is rounded to fp32: at most 2^-25 per coordinate, W * 2^-25 texels; a face's legs are >= scale / 2 texels long, so its area moves by
    # a relative 4 * W * 2^-25 / (scale / 2) at most
    tol = 4 * W * 2.0 ** -25 / (st["scale"] / 2)
    assert tol < 1e-5
    for d in (st["density_min"], st["density_max"]):
        assert abs(d / st["scale"] ** 2 - 1) <= tol
    assert R.overlap_pairs(vt, ft, H, W) == 0


def _strip_with_tilted_face():
    v, f = R.grid_sheet(3, 1, (0, 0, 0), (1, 0, 0), (0, 1, 0))              # +z strip, its +x end is the edge (vertex 3, vertex 7)
    v = np.concatenate([v, np.array([[3.5, 0.5, -0.55]], np.float32)])      # normal (0.55, 0, 0.5): just past 45 degrees towards +x
    f = np.concatenate([f, np.array([[7, 3, 8]], np.int32)])
    return v, f


def test_ref_relaxation_absorbs_a_tilted_face_and_min_cos_vetoes_it():
    v, f = _strip_with_tilted_face()
    n, da = R.face_frames(v, f)
    label0 = R.initial_labels(n)
    assert list(label0) == [4] * 6 + [0]
    assert 0.5 < n[6, 2] / da[6] < 0.8
    for min_cos, absorbed in ((0.5, True), (0.8, False)):
        st = {}
        R.uv_atlas(v, f, 128, 128, relax_rounds=1, min_cos=min_cos, stats=st)
        assert st["relax_changed"] == [1 if absorbed else 0]
        assert st["label"][6] == (4 if absorbed else 0) and st["charts"] == (1 if absorbed else 2)
        assert _cos_to_label(v, f, st["label"]).min() >= min(min_cos, 0.577)


def test_ref_tie_rules():
    # step 2: two equal components -> the lowest k
    v = np.array([[0, 0, 0], [1, -1, 0], [0, 0, 1]], np.float32)
    n, _ = R.face_frames(v, np.array([[0, 1, 2]]))
    assert list(n[0]) == [-1.0, -1.0, 0.0] and R.initial_labels(n)[0] == 1                      # -x (1) before -y (3)
    n, _ = R.face_frames(v, np.array([[0, 2, 1]]))
    assert list(n[0]) == [1.0, 1.0, 0.0] and R.initial_labels(n)[0] == 0
    # step 3: a flat face between two neighbours across edges of equal length; the neighbours' labels are set by hand
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, -1, 0], [-1, 1, 0]], np.float32)
    f = np.array([[0, 1, 2], [1, 0, 3], [0, 2, 4]], np.int64)                                   # face 0 shares (0,1) and (2,0), both of length 1
    n, da = R.face_frames(v, f)
    tabs = R.edge_tables(f, len(v))
    elen = R.edge_lengths(v, f)
    assert elen[0, 0] == elen[0, 2] == 1.0
    for a, b in ((4, 2), (2, 4)):
        new, _ = R.relax_round(np.array([0, a, b], np.int32), n, da, *tabs, elen, 0.5)
        assert new[0] == 0                            # the tie goes to k = 2 (+y), which the flat face's cosine 0 vetoes: it keeps its label
    new, _ = R.relax_round(np.array([0, 4, 4], np.int32), n, da, *tabs, elen, 0.5)
    assert new[0] == 4                                # control: without the tie the face does move to +z
    new, _ = R.relax_round(np.array([0, 4, 5], np.int32), n, da, *tabs, elen, 0.5)
    assert new[0] == 4                                # a tie between +z and -z: the lowest k again, and this one passes the cosine test


def test_ref_an_edge_with_three_faces_neither_votes_nor_joins():
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1.0]], np.float32)
    two = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    st = {}
    R.uv_atlas(v, two, 64, 64, stats=st)
    assert st["charts"] == 1
    fin = np.concatenate([two, np.array([[0, 2, 4]], np.int32)])            # a third face on the diagonal (0, 2)
    R.uv_atlas(v, fin, 64, 64, stats=st)
    assert st["charts"] == 3 and st["relax_changed"] == [0, 0, 0, 0]
    # control: two faces tilted like the fin's sides but on the boundary edge (0, 1), which then has two faces: they vote and join
    v2 = np.concatenate([v, np.array([[0.5, -0.2, 0.05]], np.float32)])
    joined = np.concatenate([two, np.array([[1, 0, 5]], np.int32)])
    R.uv_atlas(v2, joined, 64, 64, stats=st)
    assert st["charts"] == 1


def test_ref_helical_ramp_is_split_by_eviction():
    v, f = R.helical_ramp()
    n, _ = R.face_frames(v, f)
    label = R.initial_labels(n)
    assert np.all(label == 4)
    tabs = R.edge_tables(f, len(v))
    assert R.charts_of(label, np.zeros(len(f), np.int32), *tabs).max() == 0       # one chart before step 7
    st = {}
    H, W = 192, 256
    vt, ft, vm = R.uv_atlas(v, f, H, W, stats=st)
    assert st["evicted_faces"] > 0 and st["evict_rounds"] >= 1 and st["charts"] > 1
    assert R.overlap_pairs(vt, ft, H, W) == 0
    area, _ = R.face_metrics(ft, vt, R.face_frames(v, f)[1], H, W)
    assert area.min() > 0


@pytest.mark.parametrize("gutter", [0, 2, 5])
def test_ref_packing(gutter):
    v, f = R.uneven_box()
    st = {}
    H, W = 200, 320
    vt, ft, vm = R.uv_atlas(v, f, H, W, gutter=gutter, stats=st)
    chart = st["chart"]
    C = st["charts"]
    T = R.texel_coords(vt, H, W)
    lo = np.array([T[ft[chart == c]].reshape(-1, 2).min(0) for c in range(C)])
    hi = np.array([T[ft[chart == c]].reshape(-1, 2).max(0) for c in range(C)])
    assert lo.min() >= gutter and hi[:, 0].max() <= W - gutter and hi[:, 1].max() <= H - gutter
    for a in range(C):
        for b in range(a + 1, C):
            gap = np.maximum(lo[a] - hi[b], lo[b] - hi[a]).max()             # separation of the two triangle boxes along their best axis
            assert gap >= 2 * gutter, (a, b, gap)
    # every chart of the unit box has extent 1 x 1 and the projected areas sum to 6: the whole trial sequence follows
    s0 = math.sqrt(H * W / 6.0)
    scales = st["pack_scales"]
    assert len(scales) == st["pack_trials"] >= 2
    for i, s in enumerate(scales):
        assert s == pytest.approx(s0 * 0.96 ** i, rel=1e-12)
        side = math.ceil(s) + 1 + 2 * gutter
        fits, origin, _ = R.shelf_pack(np.full((6, 2), side, np.int64), H, W)
        assert fits == (i == len(scales) - 1)
        if fits:                                                             # rectangles pairwise disjoint and inside the image
            assert origin.min() >= 0 and (origin[:, 0] + side).max() <= W and (origin[:, 1] + side).max() <= H
            assert all(abs(p[0] - q[0]) >= side or abs(p[1] - q[1]) >= side for k, p in enumerate(origin) for q in origin[k + 1:])
    assert st["scale"] == scales[-1]


def test_ref_argument_errors():
    v, f = R.cube()
    with pytest.raises(ValueError, match="clean_mesh"):
        R.uv_atlas(v, np.concatenate([f, [[0, 0, 1]]]), 64, 64)
    with pytest.raises(ValueError, match="clean_mesh"):
        R.uv_atlas(np.concatenate([v, v[:1] * 0 + 2, v[:1] * 0 + 3]), np.concatenate([f, [[0, 8, 9]]]), 64, 64)   # collinear: zero area
    with pytest.raises(RuntimeError, match="do not fit"):
        R.uv_atlas(v, f, 8, 8)


# ------------------------------------------------------------------------------------------------ GPU
def _sphere_mesh(R_=24):
    import torch
    from nerf2mesh_amd.marching_cubes import marching_cubes
    x = torch.linspace(-1, 1, R_, device="cuda")
    X, Y, Z = torch.meshgrid(x, x, x, indexing="ij")
    return marching_cubes((0.6 - torch.sqrt(X * X + Y * Y + Z * Z)).contiguous(), 0.0, div=R_ - 1.0, mul=2.0, add=-1.0)


def _clean_scene(faces):
    """synthetic.scene_mesh through clean_mesh (no vertex merge: 1 % of the diagonal would collapse a mesh this fine)."""
    from nerf2mesh_amd import synthetic as S
    from nerf2mesh_amd.mesh_clean import clean_mesh
    v, f = S.scene_mesh(faces, device="cuda")
    v, f, _ = clean_mesh(v, f, v_pct=0)
    return v, f


def _bit_cases():
    import torch
    yield "sphere", _sphere_mesh()
    yield "ramp", tuple(torch.from_numpy(x).cuda() for x in R.helical_ramp())
    yield "scene", _clean_scene(6000)


def _same(a, b):
    import torch
    if torch.is_tensor(a):
        a = a.cpu().numpy()
    return np.array_equal(np.asarray(a), np.asarray(b)) if isinstance(b, np.ndarray) else a == b


@pytest.mark.gpu
def test_uv_atlas_equals_the_restatement_bit_for_bit():
    from nerf2mesh_amd.uv_atlas import uv_atlas
    for name, (v, f) in _bit_cases():
        vn, fn = v.cpu().numpy(), f.cpu().numpy()
        for (H, W) in ((256, 256), (192, 320)):
            for rounds in (0, 4):
                sd, sr = {}, {}
                vt, ft, vm = uv_atlas(v, f, H, W, relax_rounds=rounds, stats=sd)
                rvt, rft, rvm = R.uv_atlas(vn, fn, H, W, relax_rounds=rounds, stats=sr)
                tag = (name, H, W, rounds)
                assert vt.dtype.is_floating_point and vt.shape == rvt.shape, tag
                assert np.array_equal(vt.cpu().numpy().view(np.int32), rvt.view(np.int32)), tag
                assert np.array_equal(ft.cpu().numpy(), rft) and np.array_equal(vm.cpu().numpy(), rvm), tag
                assert set(sd) == set(sr) >= set(R.STAT_KEYS), tag
                for k in sr:
                    assert _same(sd[k], sr[k]), (tag, k, sd[k], sr[k])
                s2 = {}
                vt2, ft2, vm2 = uv_atlas(v, f, H, W, relax_rounds=rounds, stats=s2)                # a second device run: identical bits
                assert np.array_equal(vt2.cpu().numpy().view(np.int32), rvt.view(np.int32)) and np.array_equal(ft2.cpu().numpy(), rft), tag
                assert all(_same(s2[k], sr[k]) for k in sr), tag
                print(tag, int(f.shape[0]), {k: sd[k] for k in ("charts", "uv_vertices", "relax_changed", "evict_rounds", "evicted_faces",
                                                                "pack_trials", "utilisation")})
        if name == "ramp":
            assert sd["evicted_faces"] > 0 and sd["charts"] > 1
        if name == "sphere":
            assert sum(sd["relax_changed"]) > 0                                                    # the relaxation has work on this mesh


def _texel_tris(vt, ft, H, W):
    import torch
    T = torch.stack([vt[:, 0].double() * W, vt[:, 1].double() * H], 1)
    return T[ft.long()]                                                                             # [F, 3, 2] fp64


def _signed_area(tri):
    return 0.5 * ((tri[:, 1, 0] - tri[:, 0, 0]) * (tri[:, 2, 1] - tri[:, 0, 1]) - (tri[:, 2, 0] - tri[:, 0, 0]) * (tri[:, 1, 1] - tri[:, 0, 1]))


def _surface_area(v, f):
    import torch
    p = v.double()[f.long()]
    return 0.5 * torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).norm(dim=1)


def _edge(P, Q, px, py):
    """fp64 edge function of P -> Q at (px, py), evaluated from the lexicographically smaller endpoint (x, then y): the two faces of an
    edge get exact negatives -- the test's own antisymmetric rule, keyed on coordinates, not on the product's vertex ids."""
    import torch
    swap = (Q[:, 0] < P[:, 0]) | ((Q[:, 0] == P[:, 0]) & (Q[:, 1] < P[:, 1]))
    A, B = torch.where(swap[:, None], Q, P), torch.where(swap[:, None], P, Q)
    e = (B[:, 0] - A[:, 0]) * (py - A[:, 1]) - (B[:, 1] - A[:, 1]) * (px - A[:, 0])
    return torch.where(swap, -e, e)


def _coverage(vt, ft, H, W, budget=1 << 22):
    """count [H, W]: faces whose UV triangle holds the texel centre strictly inside; owner [H, W]: one such face (-1: none).  A torch
    scatter over the faces' texel boxes, in chunks of at most `budget` box texels."""
    import torch
    tri = _texel_tris(vt, ft, H, W)
    lo, hi = tri.amin(1), tri.amax(1)
    x0 = (lo[:, 0] - 0.5).floor().clamp(0, W - 1).long(); x1 = (hi[:, 0] - 0.5).ceil().clamp(0, W - 1).long()
    y0 = (lo[:, 1] - 0.5).floor().clamp(0, H - 1).long(); y1 = (hi[:, 1] - 0.5).ceil().clamp(0, H - 1).long()
    bw, bh = (x1 - x0 + 1).clamp(min=0), (y1 - y0 + 1).clamp(min=0)
    n = bw * bh
    cum = torch.cumsum(n, 0).cpu().numpy()
    count = torch.zeros(H * W, dtype=torch.int32, device=vt.device)
    owner = torch.full((H * W,), -1, dtype=torch.int64, device=vt.device)
    start, F = 0, int(ft.shape[0])
    while start < F:
        base = int(cum[start - 1]) if start else 0
        end = min(F, max(start + 1, int(np.searchsorted(cum, base + budget, "right"))))
        ids = torch.arange(start, end, device=vt.device)
        face = torch.repeat_interleave(ids, n[start:end])
        first = torch.cumsum(n[start:end], 0) - n[start:end]
        local = torch.arange(face.numel(), device=vt.device) - torch.repeat_interleave(first, n[start:end])
        x, y = x0[face] + local % bw[face], y0[face] + local // bw[face]
        px, py = x.double() + 0.5, y.double() + 0.5
        t = tri[face]
        inside = (_edge(t[:, 0], t[:, 1], px, py) > 0) & (_edge(t[:, 1], t[:, 2], px, py) > 0) & (_edge(t[:, 2], t[:, 0], px, py) > 0)
        cell = (y * W + x)[inside]
        count.index_put_((cell,), torch.ones_like(cell, dtype=torch.int32), accumulate=True)
        owner[cell] = face[inside]
        start = end
    return count.view(H, W), owner.view(H, W)


@pytest.mark.gpu
def test_uv_atlas_invariants_on_a_large_mesh():
    import torch
    from nerf2mesh_amd.uv_atlas import uv_atlas
    v, f = _clean_scene(300000)
    H = W = 2048
    min_cos = 0.5
    st = {}
    vt, ft, vm = uv_atlas(v, f, H, W, min_cos=min_cos, stats=st)
    print({k: st[k] for k in R.STAT_KEYS if k != "pack_scales"}, "faces", int(f.shape[0]))
    assert f.shape[0] > 250000 and vt.dtype == torch.float32 and ft.dtype == torch.int32 and vm.dtype == torch.int32
    assert float(vt.min()) >= 0 and float(vt.max()) <= 1
    assert torch.equal(vm[ft.long()], f)
    chart = st["chart"].long()
    T = int(vt.shape[0])
    assert T == st["uv_vertices"] and int(chart.max()) + 1 == st["charts"]
    vchart = torch.full((T,), -1, dtype=torch.int64, device="cuda")
    vchart[ft.long().reshape(-1)] = chart[:, None].expand(-1, 3).reshape(-1)
    assert bool((vchart[ft.long()] == chart[:, None]).all())                 # every UV vertex belongs to one chart: ft row i is in chart(i)
    key = vchart * int(v.shape[0]) + vm.long()
    assert bool((key[1:] > key[:-1]).all())                                  # one UV vertex per (chart, vertex), in that order
    area = _signed_area(_texel_tris(vt, ft, H, W))
    assert float(area.min()) > 0
    density = area / _surface_area(v, f)
    s2 = st["scale"] ** 2
    # vt is rounded to fp32 (<= 2^-25 per coordinate = 2^-14 texel at 2048); a face of this mesh has legs of >= 1 texel (scale * the cell
    # edge), so its area moves by a relative 4 * 2^-14 = 2.4e-4 at most: 1e-3 covers it
    slack = 1e-3
    print("density / scale^2:", float(density.min()) / s2, float(density.max()) / s2)
    assert float(density.min()) >= min(min_cos, 0.577) * s2 * (1 - slack) and float(density.max()) <= s2 * (1 + slack)
    assert st["density_min"] == pytest.approx(float(density.min()), rel=1e-9) and st["density_max"] == pytest.approx(float(density.max()), rel=1e-9)
    count, _ = _coverage(vt, ft, H, W)
    assert int(count.max()) <= 1                                             # no texel centre strictly inside two faces
    assert float((count > 0).float().mean()) > 0.5 * st["utilisation"]


@pytest.mark.gpu
def test_convex_inputs_evict_nothing():
    import torch
    from nerf2mesh_amd.uv_atlas import uv_atlas
    for v, f in (_sphere_mesh(), tuple(torch.from_numpy(x).cuda() for x in R.uneven_box())):
        for H, W in ((256, 256), (1024, 768)):
            st = {}
            uv_atlas(v, f, H, W, stats=st)
            assert st["evicted_faces"] == 0 and st["evict_rounds"] == 0


@pytest.mark.gpu
def test_worst_face_density_beats_the_grid_atlas():
    import torch
    from nerf2mesh_amd import export
    from nerf2mesh_amd.uv_atlas import uv_atlas
    v, f = (torch.from_numpy(x).cuda() for x in R.uneven_box())
    surf = _surface_area(v, f)
    assert float(surf.max() / surf.mean()) >= 32
    H = W = 1024
    st = {}
    vt, ft, _ = uv_atlas(v, f, H, W, stats=st)
    gvt, gft = export.grid_atlas(f.shape[0], device="cuda")
    worst = [float((_signed_area(_texel_tris(a, b, H, W)).abs() / surf).min()) for a, b in ((vt, ft), (gvt, gft))]
    print("worst texel density: charts", worst[0], "grid", worst[1], "utilisation", st["utilisation"])
    assert worst[0] > worst[1]


@pytest.mark.gpu
def test_bake_textures_reproduces_a_known_field_on_the_chart_atlas():
    """test_bake_textures_reproduces_a_known_field_on_the_grid_atlas for the chart atlas: geo_feat(p) = (p + 1) / 2; every covered texel at
    least two texels inside its face holds that value at the point its uv maps to (barycentrics computed here from vt, ft)."""
    import torch
    from nerf2mesh_amd import export
    from nerf2mesh_amd.uv_atlas import uv_atlas
    from test_texture_bake import _sphere_model
    model, v, t = _sphere_model()
    model.geo_feat = lambda x, c=None: torch.cat([(x + 1) / 2, (x + 1) / 2], dim=-1)
    h = w = 768
    vt, ft, _ = uv_atlas(v, t, h, w)
    feat0, feat1, mask = model.bake_textures(v, t, vt, ft, h, w, ssaa=1)
    assert feat0.shape == (h, w, 3) and torch.equal(feat0, feat1)
    count, owner = _coverage(vt, ft, h, w)
    assert int(count.max()) <= 1
    ys, xs = torch.nonzero(owner >= 0, as_tuple=True)
    fi = owner[ys, xs]
    tri = _texel_tris(vt, ft, h, w)[fi]
    px, py = xs.double() + 0.5, ys.double() + 0.5
    a2 = 2 * _signed_area(tri)
    e = [(tri[:, j, 0] - tri[:, i, 0]) * (py - tri[:, i, 1]) - (tri[:, j, 1] - tri[:, i, 1]) * (px - tri[:, i, 0]) for i, j in ((1, 2), (2, 0), (0, 1))]
    length = [(tri[:, j] - tri[:, i]).norm(dim=1) for i, j in ((1, 2), (2, 0), (0, 1))]
    deep = (e[0] / length[0] >= 2) & (e[1] / length[1] >= 2) & (e[2] / length[2] >= 2)            # distance to every edge >= 2 texels
    assert int(deep.sum()) > 20000
    ys, xs, fi = ys[deep], xs[deep], fi[deep]
    l = [(x[deep] / a2[deep]) for x in e]                                                         # barycentrics of corners 0, 1, 2
    corners = v.double()[t.long()[fi]]
    pos = l[0][:, None] * corners[:, 0] + l[1][:, None] * corners[:, 1] + l[2][:, None] * corners[:, 2]
    assert bool(mask[ys, xs].all())
    err = (feat0[ys, xs].double() - (pos + 1) / 2 * 255).abs()
    print("deep texels", int(deep.sum()), "max error", float(err.max()))
    assert float(err.max()) <= 1.01
    gvt, gft = export.grid_atlas(t.shape[0], device="cuda")
    _, _, gmask = model.bake_textures(v, t, gvt, gft, h, w, ssaa=1)
    print("covered share: charts", float(mask.float().mean()), "grid", float(gmask.float().mean()))
    assert float(mask.float().mean()) > float(gmask.float().mean())


@pytest.mark.gpu
def test_export_stage1_with_the_chart_atlas(tmp_path):
    import torch
    from PIL import Image
    from nerf2mesh_amd.renderer import contract
    from nerf2mesh_amd.uv_atlas import uv_atlas
    from test_texture_bake import _sphere_model
    model, v, t = _sphere_model()
    model.opt.ssaa = 2
    out = model.export_stage1(str(tmp_path), 256, 256, atlas="charts")
    assert set(out) == {0}
    for name in ("mesh_0.obj", "mesh_0.mtl", "feat0_0.jpg", "feat1_0.jpg", "mlp.json"):
        assert os.path.getsize(tmp_path / name) > 0, name
    for name in ("feat0_0.jpg", "feat1_0.jpg"):
        im = Image.open(tmp_path / name)
        assert im.size == (256, 256) and im.mode == "RGB" and im.format == "JPEG"
    im = np.asarray(Image.open(tmp_path / "feat0_0.jpg"))
    assert 90 < im[im.sum(-1) > 0].mean() < 170
    vt, ft, vm = model.last_atlas[0]
    want = uv_atlas(v, t, 512, 512)                                          # the cascade's own (h0 * ssaa, w0 * ssaa)
    assert torch.equal(vt, want[0]) and torch.equal(ft, want[1]) and torch.equal(vm, want[2])
    lines = open(tmp_path / "mesh_0.obj").read().splitlines()
    vts = [l for l in lines if l.startswith("vt ")]
    fs = [l for l in lines if l.startswith("f ")]
    V, F_ = v.shape[0], t.shape[0]
    assert sum(l.startswith("v ") for l in lines) == V and len(fs) == F_
    assert len(vts) == vt.shape[0] and V <= len(vts) < 3 * F_
    ftc, tc = ft.cpu().numpy(), t.cpu().numpy()
    for i in (0, 1, F_ // 2, F_ - 1):
        pairs = [tok.split("/") for tok in fs[i].split()[1:]]
        assert [int(p[0]) - 1 for p in pairs] == list(tc[i]) and [int(p[1]) - 1 for p in pairs] == list(ftc[i])
    u, w_ = (float(x) for x in vts[5].split()[1:])
    assert u == pytest.approx(float(vt[5, 0]), abs=1e-6) and w_ == pytest.approx(1 - float(vt[5, 1]), abs=1e-6)
    with pytest.raises(ValueError, match="charts"):
        model.export_stage1(str(tmp_path), 256, 256, atlas="xatlas")
    # opt.contract: the unwrap sees contract(v) -- on a mesh that reaches beyond the unit cube, where contract is not the identity
    model.init_stage1(v * 2.0, t)
    model.opt.contract = True
    model.geo_feat = lambda x, c=None: torch.cat([(x + 2) / 4, (x + 2) / 4], dim=-1)       # (no encoder sees the larger mesh)
    model.export_stage1(str(tmp_path / "c"), 256, 256, atlas="charts")
    v2 = (v * 2.0).contiguous()
    assert not torch.equal(contract(v2), v2)
    assert torch.equal(model.last_atlas[0][0], uv_atlas(contract(v2), t, 512, 512)[0])
    assert not torch.equal(model.last_atlas[0][0], uv_atlas(v2, t, 512, 512)[0])


@pytest.mark.gpu
def test_uv_atlas_argument_errors():
    import torch
    from nerf2mesh_amd.uv_atlas import uv_atlas
    v, f = (torch.from_numpy(x) for x in R.cube())
    with pytest.raises(RuntimeError, match="CUDA"):
        uv_atlas(v, f, 64, 64)
    v, f = v.cuda(), f.cuda()
    with pytest.raises(ValueError, match="float32"):
        uv_atlas(v.double(), f, 64, 64)
    with pytest.raises(ValueError, match=r"\[F, 3\]"):
        uv_atlas(v, f[:, :2], 64, 64)
    with pytest.raises(ValueError, match="int32 or int64"):
        uv_atlas(v, f.float(), 64, 64)
    with pytest.raises(ValueError, match="must lie in"):
        uv_atlas(v, f + 1, 64, 64)
    with pytest.raises(ValueError, match="clean_mesh"):
        uv_atlas(torch.cat([v, v[:1] * 0 + 2, v[:1] * 0 + 3]), torch.cat([f, torch.tensor([[0, 8, 9]], dtype=f.dtype, device="cuda")]), 64, 64)
    with pytest.raises(ValueError, match="clean_mesh"):
        uv_atlas(v, torch.cat([f, torch.tensor([[0, 0, 1]], dtype=f.dtype, device="cuda")]), 64, 64)
    with pytest.raises(ValueError, match="gutter"):
        uv_atlas(v, f, 64, 64, gutter=-1)
    for bad in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="min_cos"):
            uv_atlas(v, f, 64, 64, min_cos=bad)
    with pytest.raises(ValueError, match="height and width"):
        uv_atlas(v, f, 0, 64)
    with pytest.raises(RuntimeError, match="do not fit"):
        uv_atlas(v, f, 8, 8)
    vt, ft, vm = uv_atlas(v, f.long(), 64, 64)                              # int64 faces are accepted
    assert ft.dtype == torch.int32 and vt.shape == (24, 2)
