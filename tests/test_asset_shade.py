"""The exported asset drawn on the device (nerf2mesh_amd/asset.py, csrc/asset.hip): the shading kernel against its float64
restatement (tests/asset_ref.py), the sampler's orientation against the bake's through the project's own rasteriser, and the export
end to end -- export_stage1 -> ExportedAsset -> image -- on an analytic field and through the files."""
import math
import os

import numpy as np
import pytest

from nerf2mesh_amd.asset import ExportedAsset, asset_shade, evaluate_export

import asset_ref

pytestmark = pytest.mark.gpu

H, W = 37, 50                       # neither a multiple of the block's 4 rows / 64 columns; ten blocks down
TOL = 5e-5                          # ~40 fp32 multiply-adds on pre-activations <~ 17 (weights uniform in +-1/sqrt(fan_in)) give <~ 4e-5 before a
                                    # sigmoid of slope <= 1/4; the texel / 255 and the barycentric uv add a few ulp, a fast exp ~1e-6


def _cube():
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
    return v, f


def _octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, f


def _rot(ax, ay):
    ca, sa, cb, sb = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay)
    return np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]) @ np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])


@pytest.fixture(scope="module")
def case():
    """Two cascades (12 + 8 triangles, textures 40 x 56 and 24 x 24) seen side by side in a 37 x 50 view with background around them,
    rasterised by the project's own rasteriser; the float64 reference of every mode and filter, computed once."""
    import torch
    from nerf2mesh_amd import raster as dr
    rng = np.random.default_rng(11)
    vc, fc = _cube()
    vo, fo = _octahedron()
    pc = vc @ _rot(0.5, 0.7).T * 0.3 + np.array([-0.45, 0.05, 0.0])
    po = vo @ _rot(0.3, -0.4).T * 0.5 + np.array([0.42, -0.1, 0.0])
    pos = np.concatenate([pc, po])
    pos = np.concatenate([pos[:, :2], pos[:, 2:] * 0.5, np.ones((pos.shape[0], 1))], axis=1).astype(np.float32)      # clip space, w = 1
    tri = np.concatenate([fc, fo + vc.shape[0]]).astype(np.int32)
    face_begin = [0, fc.shape[0]]
    F_ = tri.shape[0]
    vt = rng.random((3 * F_, 2)).astype(np.float32)
    ft = rng.permutation(3 * F_).astype(np.int32).reshape(F_, 3)
    feat0 = [rng.integers(0, 256, size=s, dtype=np.uint8) for s in ((40, 56, 3), (24, 24, 3))]
    feat1 = [rng.integers(0, 256, size=s, dtype=np.uint8) for s in ((40, 56, 3), (24, 24, 3))]
    rays_d = (rng.standard_normal((H * W, 3)) * rng.uniform(0.5, 3.0, size=(H * W, 1))).astype(np.float32)            # length != 1
    w0 = rng.uniform(-1, 1, size=(32, 6)).astype(np.float32) / np.float32(math.sqrt(6))
    w1 = rng.uniform(-1, 1, size=(3, 32)).astype(np.float32) / np.float32(math.sqrt(32))
    rast, _ = dr.rasterize(dr.RasterizeGLContext(output_db=False), torch.from_numpy(pos).cuda().unsqueeze(0), torch.from_numpy(tri).cuda(), (H, W))
    rast = rast[0].contiguous()
    rast_np = rast.cpu().numpy()
    ref = {(m, fl): asset_ref.shade(rast_np, ft, vt, rays_d, feat0, feat1, face_begin, w0, w1, m, fl)
           for m in ("full", "diffuse", "specular") for fl in ("nearest", "linear")}
    dev = {"rast": rast, "ft": torch.from_numpy(ft).cuda(), "vt": torch.from_numpy(vt).cuda(), "rays_d": torch.from_numpy(rays_d).cuda(),
           "feat0": [torch.from_numpy(t).cuda() for t in feat0], "feat1": [torch.from_numpy(t).cuda() for t in feat1],
           "w0": torch.from_numpy(w0).cuda(), "w1": torch.from_numpy(w1).cuda()}
    return {"dev": dev, "ref": ref, "face_begin": face_begin}


def test_case_has_background_and_both_cascades(case):
    r = case["ref"][("full", "nearest")]
    cas = r["cascade"]
    assert (cas == -1).sum() > 100 and (cas == 0).sum() > 100 and (cas == 1).sum() > 100
    # the nearest comparison may leave out only pixels whose float64 texel coordinate is within 1e-4 of an integer: at most 1 % of them
    out = asset_ref.near_texel_boundary(r["x"], r["y"])[r["covered"]]
    print(f"covered {int(r['covered'].sum())}, left out of the nearest comparison {int(out.sum())}")
    assert out.mean() <= 0.01


@pytest.mark.parametrize("filter", ["nearest", "linear"])
@pytest.mark.parametrize("mode", ["full", "diffuse", "specular"])
def test_kernel_matches_the_float64_shader(case, mode, filter):
    d, r = case["dev"], case["ref"][(mode, filter)]
    got = asset_shade(d["rast"], d["ft"], d["vt"], d["rays_d"], d["feat0"], d["feat1"], case["face_begin"], d["w0"], d["w1"], mode, filter)
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == (H * W, 3)
    covered = r["covered"]
    assert np.array_equal(got[~covered], np.zeros_like(got[~covered]))                       # empty pixels are exactly 0
    keep = covered.copy()
    if filter == "nearest":
        keep &= ~asset_ref.near_texel_boundary(r["x"], r["y"])                               # there fp32 may pick the neighbouring texel
        assert (covered & ~keep).sum() <= 0.01 * covered.sum()
    err = np.abs(got[keep] - r["rgb"][keep])
    print(f"{mode}/{filter}: {int(keep.sum())} of {int(covered.sum())} covered pixels compared, max |rgb - ref| = {err.max():.3e}")
    assert err.max() <= TOL


def test_kernel_rejects_bad_arguments(case):
    d = case["dev"]
    with pytest.raises(ValueError):
        asset_shade(d["rast"], d["ft"], d["vt"], d["rays_d"], d["feat0"], d["feat1"], case["face_begin"], d["w0"], d["w1"], mode="shiny")
    with pytest.raises(ValueError):
        asset_shade(d["rast"], d["ft"], d["vt"], d["rays_d"], d["feat0"], d["feat1"], case["face_begin"], d["w0"], d["w1"], filter="cubic")
    with pytest.raises(ValueError):
        asset_shade(d["rast"], d["ft"], d["vt"], d["rays_d"], d["feat0"], d["feat1"][:1], case["face_begin"], d["w0"], d["w1"])


# ---------------------------------------------------------------------------------------------- the bake's orientation
def test_sampler_reads_the_texel_the_bake_wrote():
    """Every texel the bake's rasterisation of the atlas covers, fed back as a pixel with that texel's own rast entry, must sample
    exactly that texel: T[r, c] = (r, c, 7) comes back as (r, c, 7)."""
    import torch
    from nerf2mesh_amd import raster as dr
    from nerf2mesh_amd.uv_atlas import uv_atlas
    from test_texture_bake import _sphere_model
    model, v, t = _sphere_model()
    S = 128
    vt, ft, _ = uv_atlas(v, t, S, S)
    vt, ft = vt.float().contiguous(), ft.int().contiguous()
    uv = vt * 2.0 - 1.0                                                                      # bake_textures: uv -> clip space
    uv = torch.cat((uv, torch.zeros_like(uv[..., :1]), torch.ones_like(uv[..., :1])), dim=-1).contiguous()
    rast, _ = dr.rasterize(dr.RasterizeGLContext(output_db=False), uv.unsqueeze(0), ft, (S, S))
    mask = rast[0, :, :, 3] > 0
    rows, cols = torch.nonzero(mask, as_tuple=True)
    N = int(rows.numel())
    assert N > S * S // 4
    view = rast[0][rows, cols].view(1, N, 4).contiguous()                                    # a 1 x N "image" of the covered texels
    ys, xs = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    tex = torch.stack([ys, xs, torch.full_like(ys, 7)], dim=-1).to(torch.uint8).cuda().contiguous()
    z0, z1 = torch.zeros(32, 6, device="cuda"), torch.zeros(3, 32, device="cuda")
    got = asset_shade(view, ft, vt, torch.ones(N, 3, device="cuda"), [tex], [tex], [0], z0, z1, "diffuse", "nearest")
    got = got.cpu().numpy().astype(np.float64) * 255
    r = asset_ref.shade(view.cpu().numpy(), ft.cpu().numpy(), vt.cpu().numpy(), np.ones((N, 3)), [tex.cpu().numpy()], [tex.cpu().numpy()],
                        [0], np.zeros((32, 6)), np.zeros((3, 32)), "diffuse", "nearest")
    assert not asset_ref.near_texel_boundary(r["x"], r["y"]).any()                           # a texel centre is half a texel from every boundary
    want = np.stack([rows.cpu().numpy(), cols.cpu().numpy(), np.full(N, 7)], axis=-1)
    assert np.array_equal(np.rint(got).astype(np.int64), want)
    assert np.abs(got - want).max() < 1e-4                                                   # (texel / 255 * 255 in fp32)


# ---------------------------------------------------------------------------------------------- export -> asset -> image
TEXTURE = 512


@pytest.fixture(scope="module")
def exported(tmp_path_factory):
    """The sphere with the analytic field f(p) = ((p + 1) / 2, (p + 1) / 2) in place of geo_feat, exported at 512^2 with the chart atlas."""
    import torch
    from test_texture_bake import _sphere_model
    model, v, t = _sphere_model()
    model.geo_feat = lambda x, c=None: torch.cat([(x + 1) / 2, (x + 1) / 2], dim=-1)
    path = str(tmp_path_factory.mktemp("asset_export"))
    out = model.export_stage1(path, TEXTURE, TEXTURE, atlas="charts")
    return {"model": model, "out": out, "path": path}


def _view(size=96, cam=1):
    import stage1_case
    o, d, mvp = stage1_case.view(cam, size, size)
    return d.cuda().contiguous(), mvp.cuda().contiguous()


def test_export_to_image_reproduces_the_analytic_field(exported):
    import torch
    from nerf2mesh_amd import raster as dr
    from nerf2mesh_amd.renderer import to_clip
    model, out = exported["model"], exported["out"]
    asset = ExportedAsset.from_export(model, out)
    assert asset.cascades == [0] and asset.face_begin == [0]
    assert torch.equal(asset.feat0[0], out[0][0]) and torch.equal(asset.feat1[0], out[0][1])
    S = 96
    rays_d, mvp = _view(S)
    res = asset.render(rays_d, mvp, S, S, mode="diffuse", antialias=False)
    image = res["image"].view(S * S, 3)
    # the view's own rast, as render computes it
    clip = to_clip(asset.vertices, mvp).unsqueeze(0)
    rast, _ = dr.rasterize(asset.glctx, clip, asset.triangles, (S, S))
    pos, _ = dr.interpolate(asset.vertices.unsqueeze(0).contiguous(), rast, asset.triangles)
    pos = pos.view(-1, 3)
    r4 = rast.view(-1, 4)
    covered = r4[:, 3] > 0
    b0, b1 = r4[:, 0], r4[:, 1]
    b2 = 1 - b0 - b1
    inner = covered & (b0 > 0.05) & (b1 > 0.05) & (b2 > 0.05)
    face = (r4[:, 3].long() - 1).clamp(min=0)
    tri_uv = asset.vt[asset.ft.long()[face]]                                                 # [N, 3, 2]
    uvp = b0[:, None] * tri_uv[:, 0] + b1[:, None] * tri_uv[:, 1] + b2[:, None] * tri_uv[:, 2]
    col = (uvp[:, 0] * TEXTURE).floor().long().clamp(0, TEXTURE - 1)
    row = (uvp[:, 1] * TEXTURE).floor().long().clamp(0, TEXTURE - 1)
    baked = out[0][2][row, col]
    ok = inner & baked
    # J: the largest singular value of any face's uv -> world map
    v, f = asset.vertices.double().cpu().numpy(), asset.triangles.long().cpu().numpy()
    vt, ft = asset.vt.double().cpu().numpy(), asset.ft.long().cpu().numpy()
    E = np.stack([v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]], axis=-1)               # [F, 3, 2]
    U = np.stack([vt[ft[:, 1]] - vt[ft[:, 0]], vt[ft[:, 2]] - vt[ft[:, 0]]], axis=-1)        # [F, 2, 2]
    J = float(np.linalg.svd(E @ np.linalg.inv(U), compute_uv=False).max())
    assert np.isfinite(J)
    bound = 1 / 255 + 0.5 * J * (math.sqrt(2) / 2) / TEXTURE + 1e-5     # truncation + the field's change over half a texel diagonal + fp32
    err = (image[ok] - (pos[ok] + 1) / 2).abs()
    share = float(ok.sum()) / float(covered.sum())
    print(f"covered {int(covered.sum())}, qualifying {int(ok.sum())} ({share:.2f}), J = {J:.3f}, bound = {bound:.5f}, max error = {float(err.max()):.5f}")
    assert int(covered.sum()) > 1000
    assert share >= 0.5
    assert float(err.max()) <= bound
    # background pixels are the white default
    assert torch.equal(image[~covered], torch.ones_like(image[~covered]))


def test_loading_the_files_gives_the_exported_asset(exported):
    import torch
    from PIL import Image
    model, path = exported["model"], exported["path"]
    asset = ExportedAsset.load(path)
    for name, tex in (("feat0_0.jpg", asset.feat0[0]), ("feat1_0.jpg", asset.feat1[0])):
        assert tex.dtype == torch.uint8 and tex.is_cuda
        assert np.array_equal(tex.cpu().numpy(), np.asarray(Image.open(os.path.join(path, name))))
    vt, ft, _ = model.last_atlas[0]
    assert torch.equal(asset.ft.cpu(), ft.int().cpu())
    assert float((asset.vt.cpu().double() - vt.cpu().double()).abs().max()) <= 2.4e-7
    assert torch.equal(asset.triangles.cpu(), model.triangles.cpu())
    assert torch.equal(asset.vertices.cpu(), (model.vertices + model.vertices_offsets).detach().cpu())
    net = model.specular_net.net
    assert torch.equal(asset.w0.cpu(), net[0].weight.detach().cpu()) and torch.equal(asset.w1.cpu(), net[1].weight.detach().cpu())
    assert asset.bound == model.bound and asset.cascade == model.cascade
    S = 96
    rays_d, mvp = _view(S)
    for filt in ("nearest", "linear"):
        res = asset.render(rays_d, mvp, S, S, mode="full", filter=filt)
        assert res["image"].shape == (S * S, 3) and res["depth"].shape == (S * S,) and res["weights_sum"].shape == (S, S, 1)
        for k in ("image", "depth", "weights_sum"):
            assert bool(torch.isfinite(res[k]).all())
        assert float(res["image"].min()) >= 0 and float(res["image"].max()) <= 1
        assert float(res["weights_sum"].min()) >= 0 and float(res["weights_sum"].max()) <= 1
    assert 0.1 < float(res["weights_sum"].mean()) < 0.9                                      # the sphere is in the picture, with background
    # ssaa renders at twice the size and reduces: same shapes
    res2 = asset.render(rays_d, mvp, S, S, ssaa=2)
    assert res2["image"].shape == (S * S, 3) and res2["weights_sum"].shape == (S, S, 1)
    ev = evaluate_export(model, asset, [(rays_d, mvp)], S, S)
    assert len(ev["psnr_vs_stage1"]) == 1 and ev["mean"] == ev["psnr_vs_stage1"][0] and ev["mean"] > 0
    print(f"evaluate_export on the patched model (its render_stage1 evaluates the real field, the asset holds the analytic one): {ev['mean']:.2f} dB")


def test_two_cascades_load_and_render(tmp_path):
    import torch
    from nerf2mesh_amd.marching_cubes import marching_cubes
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    R = 16
    x = torch.linspace(-1, 1, R, device="cuda")
    X, Y, Z = torch.meshgrid(x, x, x, indexing="ij")
    v0, t0 = marching_cubes((0.6 - torch.sqrt(X * X + Y * Y + Z * Z)).contiguous(), 0.0, div=R - 1.0, mul=2.0, add=-1.0)
    vo, fo = _octahedron()                                                                   # the outer shell: any small mesh
    v1 = torch.from_numpy(vo * 1.6).float().cuda()
    t1 = torch.from_numpy(fo).int().cuda()
    torch.manual_seed(0)
    opt = make_options(O=True, bound=2, dt_gamma=0, iters=1000, fused_mlp=True)
    opt.stage, opt.ssaa = 1, 1
    model = NeRFNetwork(opt).cuda()
    V0 = v0.shape[0]
    model.init_stage1(torch.cat([v0, v1]), torch.cat([t0.int(), t1 + V0]), v_cumsum=[0, V0, V0 + v1.shape[0]])
    assert model.f_cumsum == [0, t0.shape[0], t0.shape[0] + 8]
    out = model.export_stage1(str(tmp_path), 128, 128)
    assert set(out) == {0, 1}
    asset = ExportedAsset.load(str(tmp_path))
    assert asset.cascades == [0, 1] and asset.face_begin == [0, t0.shape[0]]
    assert torch.equal(asset.triangles.cpu(), model.triangles.cpu()) and len(asset.feat0) == 2
    assert asset.bound == 2 and asset.cascade == 2
    mem = ExportedAsset.from_export(model, out)
    assert torch.equal(mem.ft, asset.ft) and torch.equal(mem.triangles, asset.triangles)
    S = 64
    rays_d, mvp = _view(S)
    a = asset.render(rays_d, mvp, S, S)
    b = mem.render(rays_d, mvp, S, S)
    assert bool(torch.isfinite(a["image"]).all()) and float(a["image"].min()) >= 0 and float(a["image"].max()) <= 1
    assert float(a["weights_sum"].mean()) > 0.3                                              # the shell fills a good part of the view
    # the two differ by the JPEG alone
    assert float((a["image"] - b["image"]).abs().mean()) < 0.05
    assert torch.equal(a["weights_sum"], b["weights_sum"])
