"""TSDF fusion of rendered depth (include/n2m_hip.h: n2m_tsdf_integrate, csrc/tsdf.hip): the stage-0 surface as the zero
level set of a truncated signed distance volume fused from one depth map per training camera, instead of an iso-surface of the density
lattice.  Not a reference path: nerf2mesh always thresholds density (nerf/renderer.py:472-546); export_stage0(method="tsdf") opts in.

  TSDFVolume(resolution, lo, hi, ...)    the two volumes (tsdf = 1, weight = 0) and their lattice; .integrate(cams, depth) is one kernel
                                         call, .extract() the zero level set without the sheet towards what no view observed
  camera_rows(poses, intrinsics)         [n,16] rows of the kernel's camera encoding
  surface_depth(out, ...)                a render's ("depth", "weights_sum") as the kernel's depth encoding
  fuse_views(render, capture, volume)    render -> surface_depth -> integrate over a capture's views, `chunk` views per call

The fusion runs on the device only: there is no host path."""
import ctypes

import torch

from . import _lib as L


def camera_rows(poses, intrinsics):
    """poses [n,4,4] (camera-to-world, the engines' OpenGL convention) and per view (fx, fy, cx, cy) -- [n,4], or four numbers shared by
    all -- as the kernel's rows [n,16] fp32 on the poses' device: rotation row-major, centre, fx, fy, cx, cy."""
    poses = torch.as_tensor(poses).float()
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4):
        raise ValueError(f"camera_rows: poses must be [n,4,4], got {tuple(poses.shape)}")
    n = poses.shape[0]
    intr = torch.as_tensor(intrinsics, dtype=torch.float64).to(torch.float32)
    if intr.dim() == 1:
        intr = intr[None].expand(n, -1)
    if tuple(intr.shape) != (n, 4):
        raise ValueError(f"camera_rows: intrinsics must be (fx, fy, cx, cy) or [{n},4] of them, got {tuple(intr.shape)}")
    return torch.cat([poses[:, :3, :3].reshape(n, 9), poses[:, :3, 3], intr.to(poses.device)], dim=1).contiguous()


def surface_depth(out, alpha_min=0.5, carve=False, alpha_carve=0.05):
    """A render's output ("depth" = sum of w t, "weights_sum" = opacity, any one shape) in the kernel's encoding: depth / weights_sum where
    weights_sum >= alpha_min (the ray stops at a surface), +inf where `carve` is on and weights_sum < alpha_carve (it stops at nothing: every
    point along it is empty), 0 elsewhere (no information)."""
    if not 0.0 <= alpha_carve <= alpha_min:
        raise ValueError(f"surface_depth: need 0 <= alpha_carve <= alpha_min, got alpha_carve={alpha_carve}, alpha_min={alpha_min}")
    if "weights_sum" not in out:
        raise ValueError("surface_depth: the render has no 'weights_sum' (the opacity of every ray)")
    depth, alpha = out["depth"].detach().float(), out["weights_sum"].detach().float().reshape(out["depth"].shape)
    hit = alpha >= alpha_min
    d = torch.where(hit, depth / torch.where(hit, alpha, torch.ones_like(alpha)), torch.zeros_like(depth))
    if carve:
        d = torch.where(alpha < alpha_carve, torch.full_like(d, float("inf")), d)
    return d


def export_options(opt):
    """The keywords export_stage0 takes for opt.mesh_method / tsdf_trunc / tsdf_carve / tsdf_alpha_min (nothing for "density")."""
    if opt.mesh_method == "density":
        return {}
    return {"method": opt.mesh_method, "tsdf": {"trunc": float(opt.tsdf_trunc) if opt.tsdf_trunc else None, "carve": bool(opt.tsdf_carve),
                                                "alpha_min": float(opt.tsdf_alpha_min)}}


class TSDFVolume:
    """tsdf, weight [R0,R1,R2] fp32 on `device`, indexed [x,y,z] (marching_cubes' layout); lattice point (a,b,c) sits at
    lo + (a,b,c) * (hi - lo) / (R - 1) per axis.  resolution: an int or three; trunc=None: four lattice spacings of the coarsest axis;
    w_max caps the running-average weight; min_depth: points nearer to a camera (along its axis) than this are not updated by it."""

    def __init__(self, resolution, lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), trunc=None, w_max=64.0, min_depth=0.0, device="cuda"):
        res = tuple(resolution) if hasattr(resolution, "__len__") else (resolution,) * 3
        if len(res) != 3 or any(isinstance(r, bool) or int(r) != r or r < 2 for r in res):
            raise ValueError(f"TSDFVolume: resolution must be an int or three, each at least 2, got {resolution!r}")
        self.resolution = tuple(int(r) for r in res)
        self.lo, self.hi = tuple(float(x) for x in lo), tuple(float(x) for x in hi)
        if len(self.lo) != 3 or len(self.hi) != 3 or not all(h > l for l, h in zip(self.lo, self.hi)):
            raise ValueError(f"TSDFVolume: hi must be above lo on every axis, got lo={lo!r}, hi={hi!r}")
        self.spacing = tuple((h - l) / (r - 1) for l, h, r in zip(self.lo, self.hi, self.resolution))
        self.trunc = 4.0 * max(self.spacing) if trunc is None else float(trunc)
        self.w_max, self.min_depth = float(w_max), float(min_depth)
        if not self.trunc > 0:
            raise ValueError(f"TSDFVolume: trunc must be > 0, got {trunc!r}")
        if not self.w_max >= 1:
            raise ValueError(f"TSDFVolume: w_max must be >= 1, got {w_max!r}")
        if not self.min_depth >= 0:
            raise ValueError(f"TSDFVolume: min_depth must be >= 0, got {min_depth!r}")
        if self.resolution[0] * self.resolution[1] * self.resolution[2] >= 1 << 32:
            raise ValueError(f"TSDFVolume: {self.resolution} lattice points are beyond 32-bit indexing")
        self.device = torch.empty(0, device=device).device
        self.tsdf = torch.ones(self.resolution, dtype=torch.float32, device=self.device)
        self.weight = torch.zeros(self.resolution, dtype=torch.float32, device=self.device)

    def integrate(self, cams, depth):
        """cams [n,16] (camera_rows), depth [n,H,W] (surface_depth's encoding), both fp32 on the volume's device: one kernel call that
        folds the n views into every lattice point in the order given.  Returns self."""
        if not (torch.is_tensor(cams) and torch.is_tensor(depth)):
            raise ValueError("TSDFVolume.integrate: cams and depth must be tensors")
        if cams.dim() != 2 or cams.shape[1] != 16 or depth.dim() != 3 or depth.shape[0] != cams.shape[0]:
            raise ValueError(f"TSDFVolume.integrate: expected cams [n,16] and depth [n,H,W], got {tuple(cams.shape)} and {tuple(depth.shape)}")
        if cams.shape[0] == 0 or depth.shape[1] == 0 or depth.shape[2] == 0:
            raise ValueError(f"TSDFVolume.integrate: no views or empty depth maps ({tuple(depth.shape)})")
        if cams.dtype != torch.float32 or depth.dtype != torch.float32:
            raise ValueError(f"TSDFVolume.integrate: cams and depth must be float32, got {cams.dtype} and {depth.dtype}")
        if cams.device != self.device or depth.device != self.device:
            raise ValueError(f"TSDFVolume.integrate: the volume lives on {self.device}, cams on {cams.device}, depth on {depth.device}")
        if not self.device.type == "cuda":
            raise RuntimeError("TSDFVolume.integrate: the volume must be on the GPU (the fusion runs on the device; there is no host path)")
        cams, depth = cams.contiguous(), depth.contiguous()
        n, H, W = (int(s) for s in depth.shape)
        f3 = ctypes.c_float * 3
        with torch.cuda.device(self.device):
            L.call("n2m_tsdf_integrate", L.ptr(self.tsdf), L.ptr(self.weight), *self.resolution, f3(*self.lo), f3(*self.hi), L.ptr(cams),
                   L.ptr(depth), n, H, W, self.trunc, self.min_depth, self.w_max, L.stream())
        return self

    def extract(self):
        """(vertices [V,3] fp32 in [lo, hi], triangles [T,3] int32) on the device: marching cubes of tsdf at 0, minus every vertex whose
        lattice edge has an endpoint no view observed (weight == 0).  A fresh lattice point holds tsdf = 1, so the level set also runs between
        "observed, behind the surface" (tsdf < 0) and "never observed" -- a sheet that is no surface of the scene; every vertex of it sits on
        such an edge.  The edge's endpoints are the floor and the ceil of the vertex's index-space position."""
        from .export import remove_vertices
        from .marching_cubes import marching_cubes
        p, tri = marching_cubes(self.tsdf, 0.0, dtype=torch.float64)                         # index space, exact
        a, b = p.floor().long(), p.ceil().long()
        unobserved = (self.weight[a[:, 0], a[:, 1], a[:, 2]] == 0) | (self.weight[b[:, 0], b[:, 1], b[:, 2]] == 0)
        f64 = lambda x: torch.tensor(x, dtype=torch.float64, device=p.device)
        # ((index / (R - 1)) * (hi - lo)) + lo in double: marching_cubes' own mapping (div=R-1, mul=2, add=-1 on the unit box)
        v = ((p / f64([r - 1 for r in self.resolution])) * (f64(self.hi) - f64(self.lo)) + f64(self.lo)).float()
        return remove_vertices(v, tri, unobserved)


@torch.no_grad()
def fuse_views(render, capture, volume, views=None, chunk=8, **surface_depth_kw):
    """Folds the views of `capture` (default: all, in order) into `volume`: `render(v)` -- the callable metrics.evaluate_views takes, e.g.
    metrics.field_renderer(model, capture) -- gives view v's depth and opacity, surface_depth(**surface_depth_kw) encodes them, and every
    `chunk` views go into one integrate call with their rows from capture.poses and capture.intrinsics_of(v).  Returns the volume."""
    views = list(range(len(capture))) if views is None else [int(v) for v in views]
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("fuse_views: chunk must be at least 1")
    H, W = capture.H, capture.W
    for s in range(0, len(views), chunk):
        part = views[s:s + chunk]
        depth = torch.empty(len(part), H, W, dtype=torch.float32, device=volume.device)
        for k, v in enumerate(part):
            depth[k] = surface_depth(render(v), **surface_depth_kw).reshape(H, W)
        cams = camera_rows(capture.poses[part], [capture.intrinsics_of(v) for v in part]).to(volume.device)
        volume.integrate(cams, depth)
    return volume
