"""The exported stage-1 asset, read back and drawn on the device: what a viewer (the reference's renderer.html) shows of the files
`export_stage1` writes.

    asset = ExportedAsset.load("mesh_stage1")                 # mesh_{cas}.obj + feat{0,1}_{cas}.jpg + mlp.json
    asset = ExportedAsset.from_export(model, out)             # the same asset before the JPEG, from export_stage1's return value
    res = asset.render(rays_d, mvp, H, W)                     # {"image", "depth", "weights_sum"} like NeRFRenderer.render_stage1
    evaluate_export(model, asset, views, H, W)                # PSNR of the asset against render_stage1, view by view

`render` is `render_stage1` with the field evaluation replaced by the viewer's fragment shader -- diffuse texel + sigmoid(2-layer
MLP(view direction, specular texel)), clamped (renderer.html:424-472) -- as ONE launch per view (csrc/asset.hip, `n2m_asset_shade`):
same `to_clip`, rasteriser, antialiasing, alpha / depth / background mixing and ssaa handling, so the two images compare pixel by
pixel.  Texture conventions are the bake's: texel (row y, column x) has its centre at uv ((x + .5) / W, (y + .5) / H), the row index grows
with v (`read_obj` has undone the 1 - v flip of the file).  No gradients: this is the product's read-out, not a training path.
"""
import ctypes
import math
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib as L
from . import export
from . import raster as dr
from .renderer import to_clip

MODES = {"full": 0, "diffuse": 1, "specular": 2}
FILTERS = {"nearest": 0, "linear": 1}


def asset_shade(rast, ft, vt, rays_d, feat0, feat1, face_begin, w0, w1, mode="full", filter="nearest"):
    """rast [H,W,4] (dr.rasterize of one view), ft [F,3] int32 / vt [T,2] of all cascades concatenated, rays_d [H*W,3] un-normalised,
    feat0 / feat1: per cascade a uint8 [Ht,Wt,3] texture, face_begin: first face of each cascade, w0 [32,6], w1 [3,32]
    -> rgb [H*W,3] float32 (empty pixels 0)."""
    if mode not in MODES:
        raise ValueError(f"asset_shade: mode must be one of {sorted(MODES)}, got {mode!r}")
    if filter not in FILTERS:
        raise ValueError(f"asset_shade: filter must be one of {sorted(FILTERS)}, got {filter!r}")
    H, W = int(rast.shape[0]), int(rast.shape[1])
    n = len(feat0)
    if not (1 <= n <= L.ASSET_MAX) or len(feat1) != n or len(face_begin) != n:
        raise ValueError(f"asset_shade: 1..{L.ASSET_MAX} cascades, one feat0 / feat1 / face_begin each")
    if rast.dim() != 3 or rast.shape[2] != 4 or rast.dtype != torch.float32 or ft.dtype != torch.int32 or vt.dtype != torch.float32:
        raise ValueError("asset_shade: rast must be float32 [H,W,4], ft int32 [F,3], vt float32 [T,2]")
    if rays_d.dtype != torch.float32 or rays_d.numel() != H * W * 3:
        raise ValueError(f"asset_shade: rays_d must be float32 [{H * W},3]")
    if tuple(w0.shape) != (32, 6) or tuple(w1.shape) != (3, 32) or w0.dtype != torch.float32 or w1.dtype != torch.float32:
        raise ValueError("asset_shade: w0 must be float32 [32,6] and w1 float32 [3,32]")
    L.check_cuda(rast=rast, ft=ft, vt=vt, rays_d=rays_d, w0=w0, w1=w1)
    tab = L.AssetTable()
    tab.count = n
    for c in range(n):
        a, b = feat0[c], feat1[c]
        if a.dtype != torch.uint8 or a.dim() != 3 or a.shape[2] != 3 or b.dtype != torch.uint8 or b.shape != a.shape:
            raise ValueError(f"asset_shade: textures of cascade {c} must be two uint8 [Ht,Wt,3] images of one size")
        L.check_cuda(feat0=a, feat1=b)
        tab.feat0[c], tab.feat1[c] = a.data_ptr(), b.data_ptr()
        tab.Ht[c], tab.Wt[c], tab.face_begin[c] = int(a.shape[0]), int(a.shape[1]), int(face_begin[c])
    rgb = torch.empty(H * W, 3, dtype=torch.float32, device=rast.device)
    L.call("n2m_asset_shade", L.ptr(rast), L.ptr(ft), L.ptr(vt), L.ptr(rays_d), ctypes.byref(tab), L.ptr(w0), L.ptr(w1),
           int(ft.shape[0]), int(vt.shape[0]), H, W, MODES[mode], FILTERS[filter], L.ptr(rgb), L.stream())
    return rgb


class ExportedAsset:
    """The cascades' meshes concatenated the way `NeRFRenderer.triangles` is (vertex and uv indices offset per cascade), one pair of
    uint8 textures per cascade, the specular head's two weight matrices."""

    def __init__(self, parts, w0, w1, bound=1, cascade=1, device="cuda"):
        """parts: per cascade present, in cascade order, a dict {"cas", "v" [V,3], "f" [F,3], "vt" [T,2], "ft" [F,3], "feat0", "feat1"
        uint8 [Ht,Wt,3]} with indices local to the cascade (arrays or tensors)."""
        if not parts:
            raise ValueError("ExportedAsset: no cascade to draw")
        if len(parts) > L.ASSET_MAX:
            raise ValueError(f"ExportedAsset: at most {L.ASSET_MAX} cascades")
        dev = torch.device(device)
        v, f, vt, ft, self.face_begin, self.cascades, self.feat0, self.feat1 = [], [], [], [], [], [], [], []
        nv = nt = nf = 0
        for p in parts:
            pv, pf = torch.as_tensor(p["v"]).float().reshape(-1, 3), torch.as_tensor(p["f"]).int().reshape(-1, 3)
            pvt, pft = torch.as_tensor(p["vt"]).float().reshape(-1, 2), torch.as_tensor(p["ft"]).int().reshape(-1, 3)
            if pf.shape[0] == 0 or pft.shape[0] != pf.shape[0]:
                raise ValueError(f"ExportedAsset: cascade {p['cas']} needs one uv triangle per face")
            if int(pf.min()) < 0 or int(pf.max()) >= pv.shape[0] or int(pft.min()) < 0 or int(pft.max()) >= pvt.shape[0]:
                raise ValueError(f"ExportedAsset: cascade {p['cas']} has a face index outside its vertices / uvs")
            v.append(pv.to(dev)); f.append(pf.to(dev) + nv); vt.append(pvt.to(dev)); ft.append(pft.to(dev) + nt)
            self.face_begin.append(nf)
            self.cascades.append(int(p["cas"]))
            self.feat0.append(torch.as_tensor(p["feat0"]).to(dev).contiguous())
            self.feat1.append(torch.as_tensor(p["feat1"]).to(dev).contiguous())
            nv, nt, nf = nv + pv.shape[0], nt + pvt.shape[0], nf + pf.shape[0]
        self.vertices, self.triangles = torch.cat(v).contiguous(), torch.cat(f).contiguous()
        self.vt, self.ft = torch.cat(vt).contiguous(), torch.cat(ft).contiguous()
        self.w0 = torch.as_tensor(w0).detach().float().to(dev).contiguous()
        self.w1 = torch.as_tensor(w1).detach().float().to(dev).contiguous()
        self.bound, self.cascade = bound, cascade
        self.glctx = dr.RasterizeGLContext(output_db=False)

    @classmethod
    def load(cls, path, device="cuda"):
        """Reads every mesh_{cas}.obj / feat0_{cas}.jpg / feat1_{cas}.jpg present under `path`, and mlp.json; a cascade without files is
        skipped (export_stage1 writes none for an empty one)."""
        mlp = export.read_mlp_json(os.path.join(path, "mlp.json"))
        parts = []
        found = (re.fullmatch(r"mesh_(\d+)\.obj", name) for name in os.listdir(path))
        for cas in sorted(int(m.group(1)) for m in found if m):
            v, f, vt, ft = export.read_obj(os.path.join(path, f"mesh_{cas}.obj"))
            parts.append({"cas": cas, "v": v, "f": f, "vt": vt, "ft": ft,
                          "feat0": export.read_jpg(os.path.join(path, f"feat0_{cas}.jpg")),
                          "feat1": export.read_jpg(os.path.join(path, f"feat1_{cas}.jpg"))})
        return cls(parts, mlp["w0"], mlp["w1"], mlp["bound"], mlp["cascade"], device)

    @classmethod
    def from_export(cls, model, out):
        """The asset as `model.export_stage1(...)` baked it, without the files: `out` is that call's return value
        ({cas: (feat0, feat1, mask)}, the uint8 textures before the JPEG), the atlas comes from `model.last_atlas`, the mesh and the
        weights from the model."""
        v_all = (model.vertices + model.vertices_offsets).detach()
        parts = []
        for cas in sorted(out):
            v0, v1, f0, f1 = model.v_cumsum[cas], model.v_cumsum[cas + 1], model.f_cumsum[cas], model.f_cumsum[cas + 1]
            vt, ft = model.last_atlas[cas][0], model.last_atlas[cas][1]
            parts.append({"cas": cas, "v": v_all[v0:v1], "f": model.triangles[f0:f1] - v0, "vt": vt, "ft": ft,
                          "feat0": out[cas][0], "feat1": out[cas][1]})
        net = model.specular_net.net
        return cls(parts, net[0].weight, net[1].weight, model.bound, model.cascade, v_all.device)

    def to(self, device):
        dev = torch.device(device)
        for name in ("vertices", "triangles", "vt", "ft", "w0", "w1"):
            setattr(self, name, getattr(self, name).to(dev))
        self.feat0 = [t.to(dev) for t in self.feat0]
        self.feat1 = [t.to(dev) for t in self.feat1]
        return self

    @torch.no_grad()
    def render(self, rays_d, mvp, h0, w0, bg_color=None, mode="full", filter="nearest", ssaa=1, antialias=True):
        """One view, as NeRFRenderer.render_stage1 returns it: {"image" [..., 3], "depth" [...], "weights_sum" [h0, w0, 1]}.
        rays_d [..., 3] (h0 * w0 rays, any length), mvp [4,4].  filter="nearest" is what renderer.html sets on both textures;
        antialias=False gives the viewer's hard silhouette edges; ssaa as opt.ssaa of render_stage1."""
        prefix = rays_d.shape[:-1]
        ssaa = int(ssaa)
        h, w = (int(h0 * ssaa), int(w0 * ssaa)) if ssaa > 1 else (int(h0), int(w0))
        if bg_color is None:
            bg_color = 1
        if torch.is_tensor(bg_color) and bg_color.dim() == 2:
            bg_color = bg_color.view(h0, w0, 3)
        rays_d = rays_d.float().contiguous().view(-1, 3)
        if ssaa > 1:
            rays_d = F.interpolate(rays_d.view(1, h0, w0, 3).permute(0, 3, 1, 2), (h, w), mode="nearest").permute(0, 2, 3, 1).reshape(-1, 3).contiguous()
        clip = to_clip(self.vertices, mvp.to(self.vertices.device)).unsqueeze(0)
        rast, _ = dr.rasterize(self.glctx, clip, self.triangles, (h, w))
        rgbs = asset_shade(rast[0], self.ft, self.vt, rays_d, self.feat0, self.feat1, self.face_begin, self.w0, self.w1, mode, filter)
        rgbs = rgbs.view(1, h, w, 3)
        alphas, _ = dr.interpolate(torch.ones_like(self.vertices[:, :1]).unsqueeze(0), rast, self.triangles)
        if antialias:
            alphas = dr.antialias(alphas, rast, clip, self.triangles)
            rgbs = dr.antialias(rgbs, rast, clip, self.triangles)
        alphas = alphas.squeeze(0).clamp(0, 1)
        rgbs = rgbs.squeeze(0).clamp(0, 1)
        image = alphas * rgbs
        depth = alphas * rast[0, :, :, [2]]
        T = 1 - alphas
        if ssaa > 1:
            def down(x):
                return F.interpolate(x.permute(2, 0, 1).unsqueeze(0), (h0, w0), mode="bilinear").squeeze(0).permute(1, 2, 0).contiguous()
            image, depth, T = down(image), down(depth), down(T)
        image = image + T * bg_color
        return {"depth": depth.view(*prefix), "image": image.view(*prefix, 3), "weights_sum": 1 - T}


def psnr(a, b):
    """10 log10(1 / mean squared error) of two images in [0, 1] (inf when they are equal)."""
    mse = float(((a.double() - b.double()) ** 2).mean())
    return math.inf if mse == 0 else -10.0 * math.log10(mse)


@torch.no_grad()
def evaluate_export(model, asset, views, h0, w0, filter="nearest"):
    """PSNR of the asset's image against `model.render_stage1` for every view of `views` (a list of (rays_d, mvp)), at the model's own
    ssaa: {"psnr_vs_stage1": [dB per view], "mean": their mean}."""
    out = []
    ssaa = int(getattr(model.opt, "ssaa", 1))
    for rays_d, mvp in views:
        ref = model.render_stage1(None, rays_d, mvp, h0, w0)["image"]
        got = asset.render(rays_d, mvp, h0, w0, filter=filter, ssaa=ssaa)["image"]
        out.append(psnr(got.float(), ref.float()))
    return {"psnr_vs_stage1": out, "mean": float(np.mean(out)) if out else float("nan")}
