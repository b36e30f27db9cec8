"""A captured image set as a data source for both stages: cameras with real intrinsics and a uint8 image bank resident on the device.

The reference keeps its training images on the device as uint8 [N,H,W,3|4], divides by 255 when it gathers a batch and converts
sRGB -> linear under `--color_space linear` (nerf/provider.py:237,323-325; nerf/utils.py:640).  `Capture` holds the same data as ONE packed
RGBA8 word per pixel (R in the low byte; a 3-channel source stores alpha 255 and sets has_alpha = False) and decodes through a [2,256]
fp32 table built once per set with the reference's own torch expressions (row 0: R, G, B; row 1: alpha) -- what the kernels of
csrc/capture.hip gather is therefore bit for bit what the torch statement computes, without a device pow.

Every kernel has its torch statement here (batch_from_uniforms_u8, Capture.view, box_downscale); Python takes it when the tensors are on
the CPU, like synthetic.batch_from_uniforms, and the GPU tests compare the kernels against it.

One image size per set (H, W) and either ONE camera model (fx, fy, cx, cy) or a per-view table [V,4] of them (Capture.per_view_intrinsics:
what COLMAP writes without --single_camera, and what every DTU scan has; the reference keeps intrinsics [N,4] and samples them per ray,
nerf/colmap_provider.py:165-182, 521, 540; nerf/dtu_provider.py:93-104, 265); H != W, fx != fy and an off-centre principal point
are allowed.  `mvps` is built FROM those intrinsics (proj_matrix), so the rasteriser of stage 1 and the rays of stage 0 see the same
camera; the reference's projection (nerf/provider.py:266-276) ignores cx, cy and fl_x, so off-centre its rays and its raster disagree.

The lens models and the undistortion pass live in lens.py, COLMAP's binary files and the pose algebra in colmap_model.py; their public
names are imported here by name, so `from nerf2mesh_amd.capture import ...` finds everything it always did.
"""
import collections
import ctypes
import json
import math
import os

import numpy as np
import torch

from . import synthetic
from .colmap_model import (COLMAP_DIRS, COLMAP_MODELS, _world_flip, center_poses, decompose_projection, quat_to_rotmat,  # noqa: F401
                           read_colmap_cameras, read_colmap_images, read_colmap_points, rotmat_to_quat, write_colmap_cameras, write_colmap_images,
                           write_colmap_points)
from .lens import (LENS_BROWN, LENS_FISHEYE, LENS_MAX_ITER, LENS_STEP, ZOOM_MAX, ZOOM_TOL, as_f64, border_taps_inside, lens_distort,  # noqa: F401
                   lens_distort_f32, lens_row, lens_undistort, undistort_bank, undistort_depth, undistort_source_f32, undistort_zoom)

NEAR, FAR = 0.05, 100.0          # clip planes of mvps, as synthetic.mvp_matrix


def srgb_to_linear(x):
    """nerf/utils.py srgb_to_linear."""
    return torch.where(x < 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)


def decode_lut(linear, device="cpu"):
    """[2,256] fp32: row 0 decodes R, G, B (x / 255, through srgb_to_linear when `linear`), row 1 decodes alpha (x / 255)."""
    a = torch.arange(256, device=device).float() / 255
    return torch.stack([srgb_to_linear(a) if linear else a, a]).contiguous()


def proj_matrix(H, W, fx, fy, cx, cy, near=NEAR, far=FAR, device="cpu"):
    """OpenGL projection of a pinhole camera with its principal point at (cx, cy), y flipped like the reference's (nerf/provider.py:266-276):
    a point on the ray of pixel centre (i + 0.5, j + 0.5) lands on window coordinates (i + 0.5, j + 0.5).  With fx = fy, cx = W / 2,
    cy = H / 2 this is synthetic.mvp_matrix's projection bit for bit (the third column is then exactly 0)."""
    return torch.tensor([[2 * fx / W, 0, 1 - 2 * cx / W, 0],
                         [0, -2 * fy / H, 1 - 2 * cy / H, 0],
                         [0, 0, -(far + near) / (far - near), -(2 * far * near) / (far - near)],
                         [0, 0, -1, 0]], dtype=torch.float32, device=device)


def nerf_matrix_to_ngp(pose, scale=0.33, offset=(0, 0, 0)):
    """nerf/provider.py:16-19 (float32 pose; translation scaled in float32, offset added in float64, stored as float32)."""
    pose = np.array(pose, dtype=np.float32)
    pose[:3, 3] = pose[:3, 3] * scale + np.array(offset)
    return pose.astype(np.float32)


def pack_rgba8(images):
    """uint8 [V,H,W,3|4] -> int32 [V,H*W] packed words (R in the low byte, alpha 255 for a 3-channel source), has_alpha."""
    images = torch.as_tensor(images)
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] not in (3, 4):
        raise ValueError("images must be uint8 [V,H,W,3] or [V,H,W,4]")
    V, H, W, C = images.shape
    if C == 3:
        images = torch.cat([images, torch.full_like(images[..., :1], 255)], -1)
    return images.contiguous().view(V, H * W, 4).view(torch.int32).view(V, H * W), C == 4


def rays_from_pixels(poses, cam_idx, pix_i, pix_j, intrinsics):
    """synthetic.rays_from_pixels (get_rays, nerf/utils.py:242-290) at intrinsics (fx, fy, cx, cy): pixel column pix_i, row pix_j.  Each of the
    four is a number, or a per-ray fp32 tensor [N] (per-view intrinsics gathered at cam_idx)."""
    fx, fy, cx, cy = intrinsics
    i = pix_i.float() + 0.5
    j = pix_j.float() + 0.5
    dirs = torch.stack([(i - cx) / fx, -(j - cy) / fy, -torch.ones_like(i)], -1)
    P = poses[cam_idx]
    rays_d = dirs[:, 0:1] * P[..., :3, 0] + dirs[:, 1:2] * P[..., :3, 1] + dirs[:, 2:3] * P[..., :3, 2]
    rays_o = P[..., :3, 3].expand_as(rays_d)
    return rays_o.contiguous(), rays_d.contiguous()


def decode_words(words, lut):
    """Packed words [...] -> fp32 [...,4]: lut[0][R], lut[0][G], lut[0][B], lut[1][A]."""
    b = words.contiguous().view(-1).view(torch.uint8).view(-1, 4).long()
    return torch.cat([lut[0][b[:, :3]], lut[1][b[:, 3:]]], -1).view(*words.shape, 4)


def intrinsics_table(intrinsics, V, device):
    """None for the shared form (four numbers); for the table form of a per-view set the fp32 [V,4] tensor on `device`, contiguous (what
    Capture.intrinsics is: no copy then)."""
    if not (torch.is_tensor(intrinsics) or isinstance(intrinsics, np.ndarray)) or np.ndim(intrinsics) != 2:
        return None
    if tuple(intrinsics.shape) != (V, 4):
        raise ValueError(f"per-view intrinsics must be [{V},4] (fx, fy, cx, cy per view), not {tuple(intrinsics.shape)}")
    return torch.as_tensor(intrinsics).to(device=device, dtype=torch.float32).contiguous()


def intrinsics_row(intrinsics, view):
    """(fx, fy, cx, cy) of one view as Python floats: the four numbers of the shared form, or row `view` of a [V,4] table (a table on the
    device is read back: a driver hands the host copy, Capture.intrinsics_host, or Capture.intrinsics_of(view))."""
    if (torch.is_tensor(intrinsics) or isinstance(intrinsics, np.ndarray)) and np.ndim(intrinsics) == 2:
        row = intrinsics[int(view)]
        return tuple(float(x) for x in (row.cpu() if torch.is_tensor(row) else row))
    return tuple(float(x) for x in intrinsics)


def _uniform_index(u, col, n):
    """int64 [N]: column `col` of the uniforms u [N,6] as an index below n (a view, a pixel) -- the batch kernels' expression."""
    return (u[:, col] * n).long().clamp(max=n - 1)


def batch_from_uniforms_u8(poses, bank, lut, u, aabb, min_near, H, W, intrinsics, out=None, counter=None, cam_near_far=None, dense_depth=None,
                           patch_size=1):
    """synthetic.batch_from_uniforms with the ground truth gathered from a packed uint8 bank [V,H*W] and decoded through `lut`.  On the GPU
    one kernel (n2m_batch_rays, every form below one descriptor); below it the torch statement of the same arithmetic, taken on the CPU.
    dense_depth [V,H*W] fp32 (Capture.dense_depth, --enable_dense_depth): an eighth tensor gt_depth [N] = dense_depth[view_n, pixel_n]
    follows the seven (`out` then has eight entries).  intrinsics: (fx, fy, cx, cy), or the table form of a per-view set
    (Capture.intrinsics, fp32 [V,4] beside the poses): ray n takes the row of its view, with or without a depth bank; on the CPU the same
    statement with the rows gathered at `cam`.  patch_size P > 1 (--patch_size): N / P^2 random P x P patches instead of N random pixels
    (synthetic.patch_pixels; n2m_batch_rays_patch on the GPU, the same descriptor), every output in the patches' row-major order."""
    dev = poses.device
    N, V, P = u.shape[0], poses.shape[0], int(patch_size)
    if P != 1 and (P < 2 or P >= H or P >= W or N % (P * P) != 0):
        synthetic.patch_pixels(u, V, H, W, P)        # raises, saying which
    table = intrinsics_table(intrinsics, V, dev)
    if table is None:
        fx, fy, cx, cy = (float(x) for x in intrinsics)
    if dense_depth is not None and tuple(dense_depth.shape) != tuple(bank.shape):
        raise ValueError(f"the depth bank is {tuple(dense_depth.shape)}, the image bank {tuple(bank.shape)}")
    if dev.type == "cuda":
        from . import _lib as L
        if out is None:
            f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
            out = (f(N, 3), f(N, 3), f(N, 4), f(N), f(N), f(N), f(N, 3)) + (() if dense_depth is None else (f(N),))
        o, d, rgba, nears, fars, noises, bg = out[:7]
        gtd = None if dense_depth is None else out[7]
        desc = L.BatchRays(poses=L.ptr(poses), uniforms=L.ptr(u), V=V, N=N, H=H, W=W, intrinsics=L.ptr(table), bank=L.ptr(bank), lut=L.ptr(lut),
                           depth_bank=L.ptr(dense_depth), aabb=L.ptr(aabb), min_near=float(min_near), cam_near_far=L.ptr(cam_near_far),
                           rays_o=L.ptr(o), rays_d=L.ptr(d), rgba=L.ptr(rgba), nears=L.ptr(nears), fars=L.ptr(fars), noises=L.ptr(noises),
                           bg=L.ptr(bg), gt_depth=L.ptr(gtd), counter=L.ptr(counter))
        if table is None:
            desc.fx, desc.fy, desc.cx, desc.cy = fx, fy, cx, cy
        if P != 1:
            L.call("n2m_batch_rays_patch", ctypes.addressof(desc), P, L.stream())
        else:
            L.call("n2m_batch_rays", ctypes.addressof(desc), L.stream())
        return (o, d, rgba, nears, fars, noises, bg) + (() if gtd is None else (gtd,))
    if P != 1:
        cam, row, col = synthetic.patch_pixels(u, V, H, W, P)
        pix = row * W + col
    else:
        cam, pix = _uniform_index(u, 0, V), _uniform_index(u, 1, H * W)
    o, d = rays_from_pixels(poses, cam, pix % W, torch.div(pix, W, rounding_mode="floor"),
                            (fx, fy, cx, cy) if table is None else table[cam].unbind(-1))
    nears, fars = synthetic.near_far_clamped(o, d, aabb, min_near, cam_near_far, cam)
    if counter is not None:
        counter.zero_()
    seven = (o, d, decode_words(bank[cam, pix], lut), nears, fars, u[:, 2].contiguous(), u[:, 3:6].contiguous())
    return seven if dense_depth is None else seven + (dense_depth[cam, pix],)


def batch_views(u, V, out=None, patch_size=1):
    """int32 [N]: the view every ray of the batch drawn from the uniforms u [N,6] reads -- column 0 through the expression the batch
    kernels use (n2m_batch_views shares their device function; on the CPU the statement of batch_from_uniforms_u8).  Needed by the
    per-image appearance codes (--ind_dim) only; a sparse-depth batch has one view: torch.full((K,), view).  patch_size P > 1: every ray
    of a patch reads the view its patch's FIRST ray names (n2m_batch_rays_patch) -- that value, broadcast over the patch's P^2 rays."""
    N, P = u.shape[0], int(patch_size)
    if P != 1:
        if P < 2 or N % (P * P) != 0:
            raise ValueError(f"a patch batch holds a multiple of patch_size^2 = {P * P} rays (patch_size >= 2), got {N}")
        per_ray = batch_views(u, V)
        cam = per_ray.view(-1, P * P)[:, :1].expand(-1, P * P).reshape(-1)
        return cam.contiguous() if out is None else out[:N].copy_(cam)
    if u.device.type == "cuda":
        from . import _lib as L
        if out is None:
            out = torch.empty(N, dtype=torch.int32, device=u.device)
        L.call("n2m_batch_views", L.ptr(u), int(V), N, L.ptr(out), L.stream())
        return out[:N]
    cam = _uniform_index(u, 0, V).to(torch.int32)
    return cam if out is None else out[:N].copy_(cam)


def batch_sparse_u8(poses, bank, lut, u, view, sparse_depth, aabb, min_near, H, W, intrinsics, out=None, counter=None, cam_near_far=None):
    """The depth-bearing batch of ONE view (nerf/colmap_provider.py:510-522): a ray through the centre of every keypoint of `view` in the
    CSR table `sparse_depth` (SparseDepth), jitter and background from u [K_v,6] (columns 2 and 3..5).  Returns batch_from_uniforms_u8's
    seven tensors + gt_depth [K_v], depth_weight [K_v].  On the GPU one kernel (n2m_batch_rays in keypoint mode); below it the torch statement."""
    dev = poses.device
    V, v = poses.shape[0], int(view)
    first, K = sparse_depth.range(v)
    if u.shape[0] != K:
        raise ValueError(f"view {v} has {K} keypoints, the uniforms are for {u.shape[0]} rays")
    fx, fy, cx, cy = intrinsics_row(intrinsics, v)            # one view per batch: a per-view set passes that view's four scalars
    if dev.type == "cuda":
        from . import _lib as L
        if out is None:
            f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
            out = (f(K, 3), f(K, 3), f(K, 4), f(K), f(K), f(K), f(K, 3), f(K), f(K))
        o, d, rgba, nears, fars, noises, bg, gtd, dw = out
        desc = L.BatchRays(poses=L.ptr(poses), uniforms=L.ptr(u), V=V, N=K, H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy, bank=L.ptr(bank), lut=L.ptr(lut),
                           coords=L.ptr(sparse_depth.coords), kp_depth=L.ptr(sparse_depth.depth), kp_weight=L.ptr(sparse_depth.weight), view=v,
                           first=first, aabb=L.ptr(aabb), min_near=float(min_near), cam_near_far=L.ptr(cam_near_far), rays_o=L.ptr(o),
                           rays_d=L.ptr(d), rgba=L.ptr(rgba), nears=L.ptr(nears), fars=L.ptr(fars), noises=L.ptr(noises), bg=L.ptr(bg),
                           gt_depth=L.ptr(gtd), depth_weight=L.ptr(dw), counter=L.ptr(counter))
        L.call("n2m_batch_rays", ctypes.addressof(desc), L.stream())
        return o, d, rgba, nears, fars, noises, bg, gtd, dw
    rc = sparse_depth.coords[first:first + K].long()
    row, col = rc[:, 0].clamp(0, H - 1), rc[:, 1].clamp(0, W - 1)
    o, d = rays_from_pixels(poses, torch.full_like(row, v), col, row, (fx, fy, cx, cy))
    nears, fars = synthetic.near_far_clamped(o, d, aabb, min_near, cam_near_far, v)
    if counter is not None:
        counter.zero_()
    return (o, d, decode_words(bank[v][row * W + col], lut), nears, fars, u[:, 2].contiguous(), u[:, 3:6].contiguous(),
            sparse_depth.depth[first:first + K].clone(), sparse_depth.weight[first:first + K].clone())


def resize_linear_at(src, H, W, rows, cols):
    """src [h,w] fp32 resized to [H,W] and read at output pixels (rows, cols) (int tensors): cv2.INTER_LINEAR's geometry -- source coordinate
    (x + 0.5) * (w / W) - 0.5 per axis (the ratio rounded to fp32 once), the two taps of an axis clamped to the edge, fp32 weights,
    a + (b - a) * t per axis (columns, then rows), so a pixel between two equal taps -- every pixel at h == H, w == W -- has their value
    exactly.  Torch statement of n2m_depth_bank_fill: every operation below is one fp32 rounding in the kernel's operand order."""
    h, w = src.shape
    ry, rx = (torch.tensor(float(np.float32(a / b)), dtype=torch.float32, device=src.device) for a, b in ((h, H), (w, W)))
    sy, sx = (rows.float() + 0.5) * ry - 0.5, (cols.float() + 0.5) * rx - 0.5
    fy0, fx0 = sy.floor(), sx.floor()
    ty, tx = sy - fy0, sx - fx0
    y0, y1 = fy0.long().clamp(0, h - 1), (fy0.long() + 1).clamp(0, h - 1)
    x0, x1 = fx0.long().clamp(0, w - 1), (fx0.long() + 1).clamp(0, w - 1)
    a, b, c, e = src[y0, x0], src[y0, x1], src[y1, x0], src[y1, x1]
    top, bot = a + (b - a) * tx, c + (e - c) * tx
    return top + (bot - top) * ty


def dense_depth_fill(src, H, W, scale=1.0, bias=0.0, out=None):
    """One row of the dense-depth bank: src [h,w] fp32 -> [H*W] fp32 = resize_linear_at(every pixel) * scale + bias (scale, bias rounded to
    fp32; multiply, then add).  On the GPU one kernel (n2m_depth_bank_fill) writing `out`; below it the torch statement, taken on the CPU."""
    if src.dim() != 2 or src.dtype != torch.float32:
        raise ValueError("a depth map must be a 2-D fp32 tensor")
    h, w = src.shape
    if src.is_cuda:
        from . import _lib as L
        src = src.contiguous()
        if out is None:
            out = torch.empty(H * W, dtype=torch.float32, device=src.device)
        L.call("n2m_depth_bank_fill", L.ptr(src), h, w, int(H), int(W), float(np.float32(h / H)), float(np.float32(w / W)), float(scale), float(bias),
               L.ptr(out), L.stream())
        return out
    jj, ii = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    s32, b32 = torch.tensor(float(scale), dtype=torch.float32), torch.tensor(float(bias), dtype=torch.float32)
    val = resize_linear_at(src.contiguous(), H, W, jj.reshape(-1), ii.reshape(-1)) * s32 + b32
    return val if out is None else out.copy_(val)


def fit_scale_bias(x, y, w):
    """(scale, bias) that map a dense depth map onto a view's sparse depths: x [K] the map at the keypoints, y [K] their triangulated depth,
    w [K] their weight (nerf/colmap_provider.py:298-321).  The reference fits with sklearn's RANSACRegressor, whose random draws cannot be
    reproduced; here the deterministic weighted least squares, float64, in closed form from the five sums -- no random consensus: an
    outlier is down-weighted by its reprojection error, not rejected.  The reference's two fall-backs follow as written: a negative scale
    -> the line through the two most confident samples; still negative -> y0 / x0 with bias 0.  Fewer than two samples, all x equal or no
    weight at all go straight to the fall-backs (a two-sample line with x0 == x1 counts as failed)."""
    x, y, w = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (x, y, w))
    if len(x) == 0:
        raise ValueError("no keypoint to calibrate the depth map with")
    scale, bias = -1.0, 0.0
    if len(x) >= 2 and x.min() != x.max():
        sw, swx, swy, swxx, swxy = w.sum(), (w * x).sum(), (w * y).sum(), (w * x * x).sum(), (w * x * y).sum()
        det = sw * swxx - swx * swx
        if sw > 0 and det > 0:
            scale = (sw * swxy - swx * swy) / det
            bias = (swy - scale * swx) / sw
    if scale < 0:
        order = np.argsort(w, kind="stable")[::-1]
        x0, y0 = x[order[0]], y[order[0]]
        scale = -1.0
        if len(x) >= 2 and x[order[1]] != x0:
            x1, y1 = x[order[1]], y[order[1]]
            scale = (y0 - y1) / (x0 - x1)
            bias = y0 - x0 * scale
        if scale < 0:
            if x0 == 0:
                raise ValueError("the depth map is 0 at the most confident keypoint: no scale can be taken from it")
            scale, bias = y0 / x0, 0.0
    return float(scale), float(bias)


class SparseDepth:
    """Keypoints with a triangulated depth, per view, as a CSR table on the device (nerf/colmap_provider.py:227-278): offsets [V+1] int32,
    coords [K,2] int32 (row, col), depth [K] fp32, weight [K] fp32.  `counts` is the host copy of the per-view sizes (a driver sizes its
    launches from it without reading the device)."""

    def __init__(self, offsets, coords, depth, weight, device="cpu"):
        off = torch.as_tensor(offsets).to(torch.int32).cpu()
        self.host_offsets = [int(x) for x in off]
        self.counts = [b - a for a, b in zip(self.host_offsets[:-1], self.host_offsets[1:])]
        K = self.host_offsets[-1]
        self.offsets = off.to(device).contiguous()
        self.coords = torch.as_tensor(coords).to(torch.int32).reshape(K, 2).to(device).contiguous()
        self.depth = torch.as_tensor(depth).float().reshape(K).to(device).contiguous()
        self.weight = torch.as_tensor(weight).float().reshape(K).to(device).contiguous()

    def __len__(self):
        return len(self.counts)

    def range(self, v):
        """(first entry, number of entries) of view v."""
        return self.host_offsets[v], self.counts[v]

    def view(self, v):
        a, k = self.range(v)
        return self.coords[a:a + k], self.depth[a:a + k], self.weight[a:a + k]


class DepthSchedule:
    """Which steps of a run are depth steps, and on which view: the reference's loader takes a depth batch when `random.random() > 0.9`
    (nerf/colmap_provider.py:510-511) on the view its shuffled sampler hands it (:513).  Here one seeded host generator per driver draws
    both, one decision per prepared batch, so trainer.Stage0Trainer and engine.Stage0Engine walk the same sequence however far ahead they
    prepare.  `log` keeps the decisions (None: a plain step)."""

    def __init__(self, n_views, seed=0):
        import random
        self.seed = seed
        self.rng, self.n, self.order, self.log = random.Random(seed), int(n_views), [], []

    def state_dict(self, position=None):
        """The schedule's position: how many decisions it has handed out (`position`: an earlier one -- a driver that prepares batches ahead
        saves the position in front of the oldest batch it has not run yet)."""
        return {"position": len(self.log) if position is None else int(position), "n_views": self.n}

    def load_state_dict(self, sd):
        """Walks a schedule of the same seed to the saved position: the sequence is a function of the seed alone."""
        if int(sd["n_views"]) != self.n:
            raise ValueError(f"depth_schedule.n_views: the checkpoint has {int(sd['n_views'])} views, the capture {self.n}")
        self.__init__(self.n, self.seed)
        for _ in range(int(sd["position"])):
            self.next()

    def next(self):
        view = None
        if self.rng.random() > 0.9:
            if not self.order:
                self.order = list(range(self.n))
                self.rng.shuffle(self.order)
            view = self.order.pop()
        self.log.append(view)
        return view


def depth_schedule_for(capture, opt, seed):
    """The DepthSchedule of a driver, or None when the capture carries no sparse depth or opt.enable_sparse_depth is off."""
    sd = getattr(capture, "sparse_depth", None)
    if sd is None or not getattr(opt, "enable_sparse_depth", False):
        return None
    return DepthSchedule(len(sd), seed)


def dense_depth_for(capture, opt):
    """The depth bank a driver gathers from on every step, or None with opt.enable_dense_depth off.  The option needs a capture that holds
    a bank, and excludes opt.enable_sparse_depth: the reference builds only one of the two (nerf/colmap_provider.py:333-337)."""
    if not getattr(opt, "enable_dense_depth", False):
        return None
    if capture is None:
        raise ValueError("enable_dense_depth needs a capture (Capture.load_colmap(..., dense_depth=True)): the synthetic scene has no depth maps")
    if getattr(capture, "dense_depth", None) is None:
        raise ValueError("enable_dense_depth is set, but the capture holds no dense-depth bank: load it with Capture.load_colmap(..., dense_depth=True)")
    if getattr(opt, "enable_sparse_depth", False):
        raise ValueError("enable_dense_depth and enable_sparse_depth exclude each other: a step has one depth target")
    return capture.dense_depth


def _read_image(name):
    from PIL import Image
    with Image.open(name) as im:
        if im.mode not in ("RGB", "RGBA"):
            im = im.convert("RGBA" if "A" in im.getbands() or "transparency" in im.info else "RGB")
        return np.asarray(im, dtype=np.uint8)


def _read_images(pairs, require_mask):
    """The uint8 images of (image file, mask file) pairs, a mask's first channel as the alpha.  A missing mask: FileNotFoundError with
    require_mask; else that view is opaque, and every image is padded to four channels when any has a mask."""
    images = []
    for iname, mname in pairs:
        im = _read_image(iname)
        if os.path.exists(mname):
            mk = _read_image(mname)
            if mk.shape[:2] != im.shape[:2]:
                raise ValueError(f"{mname} is {mk.shape[0]} x {mk.shape[1]}, its image {im.shape[0]} x {im.shape[1]}")
            im = np.concatenate([im[..., :3], mk[..., :1]], -1)
        elif require_mask:
            raise FileNotFoundError(f"image/{os.path.basename(iname)} has no mask: {mname} is missing")
        images.append(im)
    if any(im.shape[-1] == 4 for im in images):
        images = [im if im.shape[-1] == 4 else np.concatenate([im, np.full_like(im[..., :1], 255)], -1) for im in images]
    return images


def box_downscale(bank, H, W, k):
    """Packed words [V,H*W] -> [V,(H//k)*(W//k)]: per-channel integer mean of every k x k block, (sum + k*k//2) // (k*k); rows and columns
    that do not fill a block are dropped.  (The reference resizes with cv2.INTER_AREA on the host; parity with its rounding is unpinned.)"""
    V = bank.shape[0]
    h, w = H // k, W // k
    if bank.is_cuda:
        from . import _lib as L
        out = torch.empty(V, h * w, dtype=torch.int32, device=bank.device)
        L.call("n2m_capture_box_downscale", L.ptr(bank.contiguous()), V, H, W, int(k), L.ptr(out), L.stream())
        return out
    b = bank.contiguous().view(torch.uint8).view(V, H, W, 4)[:, :h * k, :w * k].long().view(V, h, k, w, k, 4)
    m = ((b.sum((2, 4)) + (k * k) // 2) // (k * k)).to(torch.uint8)
    return m.contiguous().view(V, h * w, 4).view(torch.int32).view(V, h * w)


# ------------------------------------------------------------------------------- the stages of Capture.load_colmap (its docstring has the rules)
_Cameras = collections.namedtuple("_Cameras", "h0 w0 H W per_view intrinsics family src_rows out_rows lens_rows zooms")


def _colmap_model(path, downscale):
    """Locates and reads the model: cameras, images, (point ids, xyz, errors), the image folder, whether it is images_{downscale}, and the
    sorted keys of the images that have a file in it."""
    root = next((os.path.join(path, *c) for c in COLMAP_DIRS if os.path.exists(os.path.join(path, *c))), None)
    if root is None:
        raise ValueError(f"no COLMAP model under {path} (colmap_sparse/0, sparse/0, colmap)")
    cams = read_colmap_cameras(os.path.join(root, "cameras.bin"))
    ims = read_colmap_images(os.path.join(root, "images.bin"))
    points = read_colmap_points(os.path.join(root, "points3D.bin"))
    if len(points[0]) == 0:
        raise ValueError(f"{root}: the reconstruction has no 3D points")
    folder = os.path.join(path, f"images_{downscale}")
    own_folder = os.path.exists(folder)
    if not own_folder:
        folder = os.path.join(path, "images")
    keys = [k for k in sorted(ims) if os.path.exists(os.path.join(folder, os.path.basename(ims[k]["name"])))]
    if not keys:
        raise FileNotFoundError(f"{root}/images.bin lists no image that exists under {folder}")
    return cams, ims, points, folder, own_folder, keys


def _colmap_cameras(cams, cam_ids, undistort, per_view_intrinsics, ds):
    """The cameras of the kept images (cam_ids: one id per image): full and stored image size, the intrinsics at the stored size ((fx, fy, cx,
    cy), or [V,4] when they differ: per_view) and, with coefficients to undistort, the family and per image the rows and the zoom (else None)."""
    used = sorted(set(cam_ids))
    intr, lens = [], []
    for c in used:
        model = cams[c]["model"]
        if not undistort and model in ("RADIAL", "OPENCV_FISHEYE"):         # accepted for the undistortion pass only
            raise ValueError(f"unsupported COLMAP camera model: {model}")
        f4, fam, row = lens_row(model, cams[c]["params"])
        if undistort:                                                       # without it the coefficients are ignored
            lens.append((fam,) + tuple(row))
        intr.append((cams[c]["height"], cams[c]["width"]) + f4)
    # the lens of the set: rows with a coefficient share one family; none has one -> no pass at all
    family = None
    if any(any(l[1:]) for l in lens):
        fams = {l[0] for l in lens if any(l[1:])}
        if len(fams) != 1:
            raise ValueError("the kept images mix fisheye and polynomial lens models; a set is undistorted with one model family")
        family = fams.pop()
        intr = [i + l[1:] for i, l in zip(intr, lens)]             # cameras that differ in their lens alone are different cameras
    per_view = any(i != intr[0] for i in intr[1:])
    if per_view and not per_view_intrinsics:
        raise ValueError(f"the kept images use {len(used)} cameras with different parameters; a Capture holds one camera model per set "
                         "unless it is loaded with per_view_intrinsics=True (tools/train_capture.py --per_view_intrinsics)")
    if any(i[:2] != intr[0][:2] for i in intr[1:]):
        raise ValueError(f"the kept images use cameras of differing image sizes ({sorted({i[:2] for i in intr})} as height x width); "
                         "per-view intrinsics still need one image size per set")
    by_id = dict(zip(used, intr))
    h0, w0 = intr[0][:2]
    H, W = int(round(h0 / ds)), int(round(w0 / ds))
    fx, fy, cx, cy = (x / ds for x in intr[0][2:6])
    src_rows = np.array([by_id[c][2:6] for c in cam_ids], dtype=np.float64) / ds
    if family is None:
        return _Cameras(h0, w0, H, W, per_view, src_rows if per_view else (fx, fy, cx, cy), None, None, None, None, None)
    # per kept image: its lens row, its source intrinsics at the bank's size, and the zoom of its camera (one bisection per camera)
    lens_rows = np.array([by_id[c][6:] for c in cam_ids], dtype=np.float64)
    zoom_of = {c: undistort_zoom(H, W, np.asarray(by_id[c][2:6]) / ds, family, by_id[c][6:], name=f"camera {c}") for c in used}
    zooms = np.array([zoom_of[c] for c in cam_ids], dtype=np.float64)
    out_rows = src_rows * np.stack([zooms, zooms, np.ones_like(zooms), np.ones_like(zooms)], -1)
    return _Cameras(h0, w0, H, W, per_view, out_rows if per_view else (out_rows[0, 0], out_rows[0, 1], cx, cy), family, src_rows, out_rows,
                    lens_rows, zooms)


def _colmap_poses(ims, keys, pts3d, enable_cam_center, scale):
    """Camera-to-world poses inv([R|t]) = [R^T | -R^T t] of the kept images and the points, centred, flipped and scaled: poses [V,4,4] and
    points [M,3] float64, the scale (1 / min |camera position| for -1) and the points' box [6] fp32."""
    poses = np.tile(np.eye(4), (len(keys), 1, 1))
    for n, k in enumerate(keys):
        R = quat_to_rotmat(ims[k]["q"])
        poses[n, :3, :3] = R.T
        poses[n, :3, 3] = -R.T @ ims[k]["t"]
    poses, pts = center_poses(poses, pts3d, enable_cam_center)
    poses, pts = _world_flip(poses, pts)
    if scale == -1:
        scale = 1.0 / np.linalg.norm(poses[:, :3, 3], axis=-1).min()
    poses[:, :3, 3] *= scale
    pts = pts * scale
    return poses, pts, scale, np.concatenate([pts.min(0), pts.max(0)]).astype(np.float32)


def _colmap_keypoints(ims, keys, cam, ds, poses, pts, pids, perr, keep_model):
    """Per kept image: with keep_model its (undistorted) keypoints (xy, index into the sorted points or -1); of those with a 3D point inside
    the full-size frame (rounded (row, col) at the stored size, depth fp32, weight fp32, depth, weight); and the (min, max) depth."""
    mean_err = perr.mean()
    cnf, tab, kps = [], [], []
    for n, k in enumerate(keys):
        xy, ids = ims[k]["xys"], ims[k]["point3D_ids"]
        if cam.family is not None and len(xy):
            # distorted full-size pixels -> normalised -> ideal (host inverse) -> pixels of the zoomed camera, still at full size
            sfx, sfy, scx, scy = cam.src_rows[n] * ds
            try:
                ux, uy = lens_undistort(cam.family, cam.lens_rows[n], (xy[:, 0] - scx) / sfx, (xy[:, 1] - scy) / sfy)
            except ValueError as e:
                raise ValueError(f"image {ims[k]['name']}: {e}") from None
            xy = np.stack([cam.zooms[n] * sfx * ux + scx, cam.zooms[n] * sfy * uy + scy], -1)
        if keep_model:
            found = np.searchsorted(pids, ids).clip(0, len(pids) - 1)
            kps.append((xy, np.where((ids != -1) & (pids[found] == ids), found, -1)))       # as indices into the sorted point list
        rowcol = np.stack([xy[:, 1], xy[:, 0]], -1)
        m = (ids != -1) & (rowcol[:, 0] >= 0) & (rowcol[:, 0] < cam.h0) & (rowcol[:, 1] >= 0) & (rowcol[:, 1] < cam.w0)
        if not m.any():
            raise ValueError(f"image {ims[k]['name']} has no keypoint with a 3D point inside the image")
        at = np.searchsorted(pids, ids[m])
        if (at >= len(pids)).any() or (pids[np.minimum(at, len(pids) - 1)] != ids[m]).any():
            raise ValueError(f"image {ims[k]['name']} refers to a 3D point that points3D.bin does not hold")
        rc = np.round(rowcol[m] / ds).astype(np.int32)
        rc[:, 0] = rc[:, 0].clip(0, cam.H - 1)
        rc[:, 1] = rc[:, 1].clip(0, cam.W - 1)
        P = poses[n]
        depth = (P[:3, 3] - pts[at]) @ P[:3, 2]
        weight = 2 * np.exp(-(perr[at] / mean_err) ** 2)
        cnf.append([depth.min(), depth.max()])
        tab.append((rc, depth.astype(np.float32), weight.astype(np.float32), depth, weight))
    return kps, tab, np.asarray(cnf, dtype=np.float32)


def _split(n, split):
    """The indices of a split of n kept images: every 8th is `val`, `train` the rest, `trainval` all."""
    sel = list(range(n))
    sel = sel[::8] if split == "val" else [i for i in sel if i % 8 != 0] if split == "train" else sel
    if not sel:
        raise ValueError(f"the {split} split of {n} images is empty")
    return sel


def _dense_depth_bank(depth_files, tab, cam, sel, device):
    """The depth maps of the split's views (tab, sel: their keypoint tables and indices among the kept images), each resized, calibrated
    to its keypoints and, with a lens, resampled: the bank [V,H*W] fp32 on `device`, (scale, bias) [V,2] float64, and per view what was fitted."""
    H, W = cam.H, cam.W
    bank = torch.empty(len(sel), H * W, dtype=torch.float32, device=device)
    scale_bias, samples = np.zeros((len(sel), 2), dtype=np.float64), []
    for n, i in enumerate(sel):
        m = np.load(depth_files[n])
        if m.ndim != 2 or m.size == 0 or not np.issubdtype(m.dtype, np.number):
            raise ValueError(f"{depth_files[n]} holds an array of shape {m.shape}, not a 2-D depth map")
        m = torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32))
        rc = torch.from_numpy(tab[n][0]).long()
        if cam.family is not None:
            # the undistorted plane at the (undistorted) keypoints = the resized map at the texel the kernel takes for them
            row_f32 = [torch.from_numpy(a[i].astype(np.float32)) for a in (cam.src_rows, cam.out_rows, cam.lens_rows)]
            u, v = undistort_source_f32(rc[:, 0], rc[:, 1], *row_f32, cam.family)
            rc = torch.stack([v.floor().clamp(0, H - 1).long(), u.floor().clamp(0, W - 1).long()], -1)
        x = resize_linear_at(m, H, W, rc[:, 0], rc[:, 1]).double().numpy()        # the resized map at the keypoints, on the host
        try:
            sb = fit_scale_bias(x, tab[n][3], tab[n][4])
        except ValueError as e:
            raise ValueError(f"{depth_files[n]}: {e}") from None
        scale_bias[n] = sb
        samples.append(np.stack([x, tab[n][3], tab[n][4]], -1))
        if cam.family is None:
            dense_depth_fill(m.to(device), H, W, sb[0], sb[1], out=bank[n])      # one view at a time: no full-size host copy
        else:       # resized and calibrated as the lens saw it, then resampled: a nearest gather moves values, the affine map commutes with it
            plane = dense_depth_fill(m.to(device), H, W, sb[0], sb[1]).view(1, H * W)
            undistort_depth(plane, H, W, cam.src_rows[i], cam.out_rows[i], cam.lens_rows[i], cam.family, out=bank[n:n + 1])
    return bank, scale_bias, samples


class Capture:
    """poses [V,4,4] fp32 (camera-to-world, OpenGL: the engines' convention), H, W, intrinsics (fx, fy, cx, cy), bank [V,H*W] packed RGBA8
    (int32 storage) on `device`, has_alpha, linear (opt.color_space == 'linear'), optional cam_near_far [V,2], mvps [V,4,4].  It can be handed
    to export_stage0 as its `dataset` (.mvps, .H, .W)."""

    pts_aabb = None           # [6] fp32 (host): box of the reconstruction's sparse points (load_colmap), for renderer.update_aabb
    sparse_depth = None       # SparseDepth (load_colmap(sparse_depth=True))
    dense_depth = None        # [V,H*W] fp32 on the device (load_colmap(dense_depth=True)): depths/NAME.npy resized and calibrated per view
    dense_depth_scale_bias = None     # [V,2] float64 (host): the (scale, bias) fitted per view
    dense_depth_samples = None        # keep_model=True: per view [K,3] float64 (host), what was fitted: map at the keypoints, their depth, weight
    undistort_zoom = None     # load_colmap(undistort=True): the zoom s >= 1 the focal lengths were multiplied by (a number, or float64 [V] per view)
    colmap = None             # load_colmap(keep_model=True): the reconstruction's points, errors, keypoints and names, as save_colmap takes them

    per_view_intrinsics = False       # True: `intrinsics` is an fp32 [V,4] tensor on the device (fx, fy, cx, cy per view), `intrinsics_host` its float64 source
    intrinsics_host = None

    def __init__(self, poses, bank, H, W, intrinsics, has_alpha=True, linear=False, cam_near_far=None, device=None, per_view=None):
        """intrinsics: (fx, fy, cx, cy), or [V,4] of them.  A table whose rows are all equal collapses to the shared form (every path of a
        one-camera set stays what it is); per_view=True keeps (or makes) the table form even then, per_view=False refuses differing rows."""
        device = torch.device(device if device is not None else bank.device)
        self.device = device
        self.H, self.W = int(H), int(W)
        poses_cpu = torch.as_tensor(poses).detach().float().cpu().contiguous()
        V = poses_cpu.shape[0] if poses_cpu.dim() == 3 else 0
        intr = as_f64(intrinsics)
        if intr.shape == (4,):
            table = np.tile(intr, (V, 1)) if per_view else None
        elif intr.shape == (V, 4):
            equal = bool((intr == intr[0]).all())
            if per_view is False and not equal:
                raise ValueError("per_view=False, but the rows of the intrinsics differ")
            table = intr.copy() if (per_view or not equal) else None
            intr = intr[0]
        else:
            raise ValueError(f"intrinsics must be (fx, fy, cx, cy) or [V,4] = [{V},4] of them, not an array of shape {intr.shape}")
        if table is None:
            self.intrinsics = tuple(float(x) for x in intr)
        else:
            self.per_view_intrinsics = True
            self.intrinsics_host = table                                   # float64 [V,4]; each device entry is this rounded once to fp32
        if poses_cpu.dim() != 3 or poses_cpu.shape[1:] != (4, 4):
            raise ValueError("poses must be [V,4,4]")
        if tuple(bank.shape) != (poses_cpu.shape[0], self.H * self.W) or bank.dtype != torch.int32:
            raise ValueError("bank must be int32 [V, H*W] (pack_rgba8)")
        self.poses = poses_cpu.to(device)
        self.bank = bank.to(device).contiguous()
        self.device = device = self.bank.device               # with its index ("cuda" -> cuda:0)
        self.has_alpha, self.linear = bool(has_alpha), bool(linear)
        self.lut = decode_lut(self.linear, device)
        self.cam_near_far = None if cam_near_far is None else torch.as_tensor(cam_near_far).float().to(device).contiguous()
        if self.per_view_intrinsics:
            self.intrinsics = torch.from_numpy(self.intrinsics_host.astype(np.float32)).to(device).contiguous()
        self.mvps = torch.stack([proj_matrix(self.H, self.W, *self.intrinsics_of(v)) @ torch.inverse(p)      # per pose on the host, like
                                 for v, p in enumerate(poses_cpu)]).to(device)                                # synthetic.mvp_matrix

    def intrinsics_of(self, v):
        """(fx, fy, cx, cy) of view v as Python floats, from the host copy: no device read."""
        return tuple(float(x) for x in self.intrinsics_host[int(v)]) if self.per_view_intrinsics else self.intrinsics

    # ------------------------------------------------------------------------------------------------ constructors
    @classmethod
    def from_arrays(cls, poses, images_uint8, intrinsics, linear=False, cam_near_far=None, downscale=1, device="cpu", per_view=None):
        """poses [V,4,4], images uint8 [V,H,W,3|4] (numpy or torch), intrinsics (fx, fy, cx, cy) of the images as given, or [V,4] of them (per
        view; see __init__ for `per_view`); downscale=k takes the k x k integer block mean on `device` and divides the intrinsics by k."""
        images = torch.as_tensor(images_uint8)
        V, H, W, _ = images.shape
        bank, has_alpha = pack_rgba8(images)
        bank = bank.to(device)
        k = int(downscale)
        if k < 1:
            raise ValueError("downscale must be a positive integer")
        if k > 1:
            bank = box_downscale(bank, H, W, k)
            intrinsics = as_f64(intrinsics) / k
            H, W = H // k, W // k
        return cls(poses, bank, H, W, intrinsics, has_alpha=has_alpha, linear=linear, cam_near_far=cam_near_far, device=device, per_view=per_view)

    @classmethod
    def load_nerf(cls, path, split="train", scale=0.33, offset=(0, 0, 0), downscale=1, linear=False, device="cpu"):
        """transforms_{split}.json (else transforms.json) by the rules of nerf/provider.py:150-263: H, W from h / w or the first image, focal
        from fl_x / fl_y else camera_angle_x / camera_angle_y, cx, cy default to W / 2, H / 2, `.png` appended to a file name without an
        extension, missing files skipped, poses through nerf_matrix_to_ngp.  Images are read with PIL."""
        name = os.path.join(path, f"transforms_{split}.json")
        if not os.path.exists(name):
            name = os.path.join(path, "transforms.json")
        if not os.path.exists(name):
            raise FileNotFoundError(f"no transforms_{split}.json or transforms.json under {path}")
        with open(name) as f:
            tr = json.load(f)
        poses, images = [], []
        for fr in tr["frames"]:
            fp = os.path.join(path, fr["file_path"])
            if "." not in os.path.basename(fp):
                fp += ".png"
            if not os.path.exists(fp):
                continue
            images.append(_read_image(fp))
            poses.append(nerf_matrix_to_ngp(fr["transform_matrix"], scale, offset))
        if not images:
            raise FileNotFoundError(f"{name} lists no image that exists")
        if any(im.shape != images[0].shape for im in images):
            raise ValueError("all images of a set must share one size and channel count")
        if "h" in tr and "w" in tr:
            H, W = int(tr["h"]), int(tr["w"])
            if images[0].shape[:2] != (H, W):
                raise ValueError(f"{name} states {H} x {W}, the images are {images[0].shape[0]} x {images[0].shape[1]}")
        else:
            H, W = images[0].shape[:2]
        if "fl_x" in tr or "fl_y" in tr:
            fx = tr["fl_x"] if "fl_x" in tr else tr["fl_y"]
            fy = tr["fl_y"] if "fl_y" in tr else tr["fl_x"]
        elif "camera_angle_x" in tr or "camera_angle_y" in tr:
            fx = W / (2 * math.tan(tr["camera_angle_x"] / 2)) if "camera_angle_x" in tr else None
            fy = H / (2 * math.tan(tr["camera_angle_y"] / 2)) if "camera_angle_y" in tr else None
            fx, fy = (fy if fx is None else fx), (fx if fy is None else fy)
        else:
            raise RuntimeError(f"{name}: no focal length (fl_x / fl_y / camera_angle_x / camera_angle_y)")
        cx = tr["cx"] if "cx" in tr else W / 2.0
        cy = tr["cy"] if "cy" in tr else H / 2.0
        return cls.from_arrays(np.stack(poses), np.stack(images), (fx, fy, cx, cy), linear=linear, downscale=downscale, device=device)

    @classmethod
    def load_colmap(cls, path, split="train", scale=-1, downscale=1, linear=False, enable_cam_center=False, sparse_depth=False, device="cpu",
                    keep_model=False, dense_depth=False, per_view_intrinsics=False, undistort=False):
        """A COLMAP reconstruction by the rules of nerf/colmap_provider.py:134-278, 404-435 (own reader of cameras.bin / images.bin /
        points3D.bin, see above; looked for under colmap_sparse/0, sparse/0, colmap).  Image keys sorted, entries without a file under
        images_{downscale}/ (else images/) dropped; poses = inv([R|t]) -> center_poses -> convention flip -> scale (-1: 1 / min |camera
        position|); pts_aabb = box of the scaled points; per kept image the keypoints with a 3D point inside the full-resolution image give
        cam_near_far (min, max depth) and, with sparse_depth=True, the CSR table Capture.sparse_depth.  Every 8th kept image is `val`,
        `train` the rest, `trainval` all.  mask/NAME.png supplies alpha.  Without an images_{downscale} folder the bank's own box downscale
        is taken (integer downscale that divides the size).  One camera model per set: kept images whose cameras differ are a ValueError
        -- unless per_view_intrinsics=True: then they give the table form (Capture.per_view_intrinsics), row n the camera of kept image n
        divided by `downscale` (nerf/colmap_provider.py:165-182: the same models, distortion ignored); the cameras must still state one image
        size, which the keypoint test and the rounding of keypoint coordinates use.
        keep_model=True keeps the transformed points, their errors and every kept view's keypoints on the host as Capture.colmap (what
        save_colmap takes to write the set back); training needs none of it, so by default it is dropped.
        dense_depth=True (--enable_dense_depth, :281-327): every view of the split needs depths/<stem of its name>.npy, a 2-D float array of
        any size; it is resized to [H,W] (resize_linear_at), calibrated to the view's keypoints by one (scale, bias) (fit_scale_bias, a
        deterministic weighted least squares in the place of the reference's RANSAC) and stored as a row of Capture.dense_depth.
        undistort=True: the lens coefficients of SIMPLE_RADIAL and OPENCV cameras are used, RADIAL and OPENCV_FISHEYE cameras are accepted
        (lens_row), and the set is made pinhole once, here, as COLMAP's image_undistorter would: decode, box downscale (intrinsics divided,
        coefficients unchanged: they live in normalised coordinates), then undistort_bank into a camera of the same size and principal
        point whose focal lengths are multiplied by Capture.undistort_zoom (undistort_zoom(): no blank pixel; one zoom per camera).
        Capture.intrinsics holds the new values; keypoints go through lens_undistort and the new intrinsics before they are tested against
        the frame and rounded; a dense depth map is resized, resampled by undistort_depth (nearest texel) and calibrated at the
        undistorted keypoints.  A set whose kept cameras all have zero coefficients skips the pass: bit for bit undistort=False."""
        if split not in ("train", "val", "trainval"):
            raise ValueError(f"split must be train, val or trainval, not {split!r}")
        ds = downscale
        cams, ims, (pids, pts3d, perr), folder, own_folder, keys = _colmap_model(path, ds)
        cam = _colmap_cameras(cams, [ims[k]["camera_id"] for k in keys], undistort, per_view_intrinsics, ds)
        H, W = cam.H, cam.W
        poses, pts, scale, pts_aabb = _colmap_poses(ims, keys, pts3d, enable_cam_center, scale)
        kps, tab, cnf = _colmap_keypoints(ims, keys, cam, ds, poses, pts, pids, perr, keep_model)
        sel = _split(len(keys), split)
        tab = [tab[i] for i in sel]
        names = [os.path.basename(ims[keys[i]]["name"]) for i in sel]
        stems = [os.path.splitext(b)[0] for b in names]
        depth_files = [os.path.join(path, "depths", s + ".npy") for s in stems]
        if dense_depth:
            for name in depth_files:
                if not os.path.exists(name):
                    raise FileNotFoundError(f"dense depth asked for, but there is no {name}")
        images = _read_images([(os.path.join(folder, b), os.path.join(path, "mask", s + ".png")) for b, s in zip(names, stems)], require_mask=False)
        if any(im.shape != images[0].shape for im in images):
            raise ValueError("all images of a set must share one size")
        bank, has_alpha = pack_rgba8(np.stack(images))
        bank = bank.to(device)
        ih, iw = images[0].shape[:2]
        if (ih, iw) != (H, W):
            k = int(ds)
            if own_folder or k != ds or (ih, iw) != (cam.h0, cam.w0) or (ih // k, iw // k) != (H, W):
                raise ValueError(f"the images are {ih} x {iw}, the cameras state {cam.h0} x {cam.w0} at downscale {ds}: only the full-size images "
                                 "with an integer downscale that divides them can be reduced here")
            bank = box_downscale(bank, ih, iw, k)
        if cam.family is not None:
            rows = sel if cam.per_view else 0            # one row for the set, or a row per view
            bank = undistort_bank(bank, H, W, cam.src_rows[rows], cam.out_rows[rows], cam.lens_rows[rows], cam.family)
        cap = cls(poses[sel].astype(np.float32), bank, H, W, cam.intrinsics[sel] if cam.per_view else cam.intrinsics, has_alpha=has_alpha,
                  linear=linear, cam_near_far=cnf[sel], device=device)
        cap.pts_aabb = torch.from_numpy(pts_aabb)
        cap.scale = float(scale)
        if undistort:
            cap.undistort_zoom = 1.0 if cam.family is None else cam.zooms[sel] if cam.per_view else float(cam.zooms[0])
        if keep_model:
            cap.colmap = dict(points=pts, errors=perr, keypoints=[kps[i] for i in sel], names=names)
        if sparse_depth:
            off = np.concatenate([[0], np.cumsum([len(t[1]) for t in tab])])
            cap.sparse_depth = SparseDepth(off, np.concatenate([t[0] for t in tab]), np.concatenate([t[1] for t in tab]),
                                           np.concatenate([t[2] for t in tab]), device=cap.device)
        if dense_depth:
            cap.dense_depth, cap.dense_depth_scale_bias, samples = _dense_depth_bank(depth_files, tab, cam, sel, cap.device)
            if keep_model:
                cap.dense_depth_samples = samples
        return cap

    @classmethod
    def load_dtu(cls, path, split="train", scale=-1, offset=(0, 0, 0), downscale=1, linear=False, device="cpu"):
        """A DTU scan in the layout of nerf/dtu_provider.py:80-109, 173-211: cameras_sphere.npz (world_mat_i, scale_mat_i), image/*.png and
        mask/*.png, each list sorted (a mask carries its image's file name; its first channel is the alpha).  Per image P = (world_mat @
        scale_mat)[:3,:4] in fp32, as the reference forms it; then -- cv2.decomposeProjectionMatrix is not used here -- decompose_projection
        in float64: row (K00, K11, K02, K12) of K / K22 and the pose [R^T | C], through nerf_matrix_to_ngp (scale == -1 means 1) and the
        three axis fixes of :107-109.  Every view has its own K: the set comes back in the table form unless all rows are equal.  `val` is
        the first frame, `train` the rest, `trainval` / `all` every frame (the reference's test trajectory: camera_path.CameraPath).  downscale=k: the
        bank's integer box mean, H // k x W // k, and the rows divided by k -- the reference resizes the images and forgets that division
        (its rays of a downscaled DTU set use the full-size K)."""
        if split not in ("train", "val", "trainval", "all"):
            raise ValueError(f"split must be train, val, trainval or all, not {split!r}")
        k = int(downscale)
        if k < 1 or k != downscale:
            raise ValueError("downscale must be a positive integer")
        if scale == -1:
            scale = 1
        cam_file = os.path.join(path, "cameras_sphere.npz")
        if not os.path.exists(cam_file):
            raise FileNotFoundError(f"no cameras_sphere.npz under {path}")
        names = sorted(f for f in os.listdir(os.path.join(path, "image")) if f.endswith(".png")) if os.path.isdir(os.path.join(path, "image")) else []
        if not names:
            raise FileNotFoundError(f"no image/*.png under {path}")
        rows, poses = [], []
        with np.load(cam_file) as cams:
            for idx in range(len(names)):
                for key in (f"world_mat_{idx}", f"scale_mat_{idx}"):
                    if key not in cams:
                        raise ValueError(f"{cam_file} has no {key} ({len(names)} images)")
                P = (cams[f"world_mat_{idx}"].astype(np.float32) @ cams[f"scale_mat_{idx}"].astype(np.float32))[:3, :4]
                K, R, C = decompose_projection(P)
                rows.append((K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
                pose = np.eye(4, dtype=np.float32)
                pose[:3, :3] = R.T
                pose[:3, 3] = C
                poses.append(nerf_matrix_to_ngp(pose, scale, offset))
        poses = np.stack(poses)
        poses[:, :3, 1:3] *= -1
        poses = poses[:, [1, 0, 2, 3], :]
        poses[:, 2] *= -1
        sel = list(range(len(names)))
        sel = sel[1:] if split == "train" else sel[:1] if split == "val" else sel
        if not sel:
            raise ValueError(f"the {split} split of {len(names)} images is empty")
        images = _read_images([(os.path.join(path, "image", names[i]), os.path.join(path, "mask", names[i])) for i in sel], require_mask=True)
        if any(im.shape != images[0].shape for im in images):
            raise ValueError("all images of a set must share one size (per-view image sizes are not supported)")
        cap = cls.from_arrays(poses[sel], np.stack(images), np.asarray(rows, dtype=np.float64)[sel], linear=linear, downscale=k, device=device)
        cap.scale = float(scale)
        return cap

    @classmethod
    def synthetic(cls, poses, scene="lego", H=synthetic.LEGO_HW, W=synthetic.LEGO_HW, intrinsics=None, alpha=True, linear=False,
                  cam_near_far=None, device=None, chunk=1 << 20, per_view=None):
        """The box scene rendered through synthetic.render_gt at arbitrary intrinsics (default: the lego camera) and quantised with
        (x * 255 + 0.5).to(uint8); alpha=False composites on white and keeps three channels.  intrinsics [V,4]: every view is rendered at
        its own row (see __init__ for `per_view`)."""
        poses = torch.as_tensor(poses).float()
        dev = torch.device(device if device is not None else poses.device)
        if intrinsics is None:
            intrinsics = (synthetic.LEGO_FOCAL, synthetic.LEGO_FOCAL, W / 2, H / 2)
        V = poses.shape[0]
        intr = as_f64(intrinsics)
        if intr.ndim == 2 and intr.shape != (V, 4):
            raise ValueError(f"per-view intrinsics must be [{V},4], not {intr.shape}")
        rows = [intrinsics_row(intr, v) for v in range(V)]
        pd, bx = poses.to(dev), synthetic.boxes(dev, scene)
        images = torch.empty(V, H * W, 4 if alpha else 3, dtype=torch.uint8, device=dev)
        pix = torch.arange(H * W, device=dev)
        for v in range(V):
            for s in range(0, H * W, chunk):
                p = pix[s:s + chunk]
                o, d = rays_from_pixels(pd, torch.full_like(p, v), p % W, torch.div(p, W, rounding_mode="floor"), rows[v])
                rgba = synthetic.render_gt(o, d, bx)
                if not alpha:
                    rgba = rgba[:, :3] * rgba[:, 3:] + (1 - rgba[:, 3:])
                images[v, s:s + chunk] = (rgba * 255 + 0.5).to(torch.uint8)
        return cls.from_arrays(poses, images.view(V, H, W, -1), intr, linear=linear, cam_near_far=cam_near_far, device=dev, per_view=per_view)

    # ------------------------------------------------------------------------------------------------------- access
    def check_device(self, device):
        """Raises when a driver on `device` is handed this set: the bank is gathered from where it lies, never copied per batch."""
        if torch.empty(0, device=device).device != self.device:
            raise ValueError(f"the capture lives on {self.device}, the driver on {device}")

    def __len__(self):
        return int(self.poses.shape[0])

    @property
    def nbytes(self):
        return self.bank.numel() * 4 + (0 if self.dense_depth is None else self.dense_depth.numel() * 4)

    def bank_bytes(self):
        """uint8 view [V,H,W,4] of the bank (R, G, B, A)."""
        return self.bank.view(torch.uint8).view(len(self), self.H, self.W, 4)

    def decode(self, view=None):
        """The fp32 images the kernels gather from: [V,H*W,4], or [H*W,4] of one view."""
        return decode_words(self.bank if view is None else self.bank[view], self.lut)

    def view(self, v, stride=1, dirs_ssaa=0):
        """One whole view at pixel stride `stride` (h = H // stride, w = W // stride, pixel (j * stride, i * stride)): rays_o, rays_d [h*w,3],
        rgba [h*w,4], and with dirs_ssaa >= 1 the unit directions [h*ssaa * w*ssaa, 3] stage 1 shades with (safe_normalize of every pixel's
        direction, repeated ssaa x ssaa times) -- else None.  On the GPU one kernel (n2m_capture_view); a per-view set hands it row v's four
        scalars from the host copy (no device read)."""
        s, a = int(stride), int(dirs_ssaa)
        h, w = self.H // s, self.W // s
        dev = self.device
        if dev.type == "cuda":
            from . import _lib as L
            f = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
            o, d, rgba = f(h * w, 3), f(h * w, 3), f(h * w, 4)
            dirs = f(h * a * w * a, 3) if a >= 1 else None
            L.call("n2m_capture_view", L.ptr(self.poses), len(self), int(v), self.H, self.W, s, *self.intrinsics_of(v), L.ptr(self.bank), L.ptr(self.lut),
                   L.ptr(o), L.ptr(d), L.ptr(rgba), L.ptr(dirs), max(a, 1), L.stream())
            return o, d, rgba, dirs
        jj, ii = torch.meshgrid(torch.arange(h, device=dev) * s, torch.arange(w, device=dev) * s, indexing="ij")
        jj, ii = jj.reshape(-1), ii.reshape(-1)
        o, d = rays_from_pixels(self.poses, int(v), ii, jj, self.intrinsics_of(v))
        rgba = decode_words(self.bank[int(v)][jj * self.W + ii], self.lut)
        dirs = None
        if a >= 1:
            n2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            # sqrt through fp64: the kernel's sqrtf is correctly rounded, torch's fp32 sqrt on the CPU is not for every build (a vector math
            # library serves larger tensors and is off by an ulp for ~0.7 % of the values); an fp64 sqrt rounded to fp32 is the correctly
            # rounded fp32 sqrt (53 >= 2 * 24 + 2 bits)
            unit = d / torch.clamp(n2, min=1e-20).double().sqrt().float().unsqueeze(-1)
            dirs = unit.view(h, 1, w, 1, 3).expand(h, a, w, a, 3).reshape(-1, 3).contiguous()
        return o, d, rgba, dirs

    def save_nerf(self, path, split="train", scale=1.0, offset=(0, 0, 0)):
        """transforms_{split}.json + {split}/r_{v}.png (PIL), such that load_nerf(path, split, scale, offset) gives this set back: the stored
        translation is (t - offset) / scale.  RGB sets are written as 3-channel PNGs."""
        from PIL import Image
        if self.per_view_intrinsics:
            raise ValueError("the nerf format states one camera for the whole set; a set with per-view intrinsics is written by save_colmap or save_dtu")
        os.makedirs(os.path.join(path, split), exist_ok=True)
        by = self.bank_bytes().cpu().numpy()
        fx, fy, cx, cy = self.intrinsics
        frames = []
        for v in range(len(self)):
            rel = f"{split}/r_{v}"
            Image.fromarray(by[v] if self.has_alpha else np.ascontiguousarray(by[v, :, :, :3])).save(os.path.join(path, rel + ".png"))
            m = self.poses[v].double().cpu().numpy().copy()
            m[:3, 3] = (m[:3, 3] - np.array(offset, dtype=np.float64)) / scale
            frames.append({"file_path": rel, "transform_matrix": m.tolist()})
        with open(os.path.join(path, f"transforms_{split}.json"), "w") as f:
            json.dump({"h": self.H, "w": self.W, "fl_x": fx, "fl_y": fy, "cx": cx, "cy": cy, "frames": frames}, f)

    def save_colmap(self, path, points, errors=None, keypoints=None, names=None, scale=1.0, model="PINHOLE", folder="sparse/0",
                    depths=None, distortion=None):
        """Writes a COLMAP reconstruction (cameras.bin, images.bin, points3D.bin under `folder`, images/NAME.png) such that
        load_colmap(path, "trainval", scale=scale) of an already centred set (one that load_colmap produced, saved with the points, errors,
        keypoints and names of its Capture.colmap) gives this set back; any other set comes back re-centred by center_poses.  Mirrors
        save_nerf.  points [M,3] in this set's world (numbered from 1 in the file), errors [M] (default 1), keypoints: per view (xy [n,2] in
        pixels, index [n] into `points` or -1) -- default: every point projected into every view it lies in front of and inside of.  One
        camera (id 1) of `model` PINHOLE or SIMPLE_PINHOLE (needs fx = fy) at the stored size; a set with per-view intrinsics: one camera
        per distinct row, every image with the id of its row (load_colmap(..., per_view_intrinsics=True) reads it back).  depths: one 2-D array per view, of any
        size, written as depths/<stem of the view's name>.npy (what load_colmap(dense_depth=True) reads).
        distortion=(coefficients, model): the cameras are written as `model` SIMPLE_RADIAL (k; needs fx = fy), RADIAL (k1, k2; fx = fy),
        OPENCV (k1, k2, p1, p2) or OPENCV_FISHEYE (k1..k4) with those coefficients -- one list for the set, or one row per view -- i.e.
        the bank is declared to hold photographs taken through that lens (load_colmap(..., undistort=True) makes them pinhole); default
        keypoints are then the distorted projections.  It replaces `model`."""
        from PIL import Image
        points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
        M, V = len(points), len(self)
        ids = np.arange(1, M + 1, dtype=np.int64)
        errors = np.ones(M) if errors is None else np.asarray(errors, dtype=np.float64).reshape(M)
        names = [f"r_{v}.png" for v in range(V)] if names is None else list(names)
        # one camera per distinct row (ids from 1 in order of first appearance), every image the id of its row; a shared set: one camera, id 1
        rows = [self.intrinsics_of(v) for v in range(V)]
        lens = None
        if distortion is not None:
            coeff, model = distortion
            ncoef = {"SIMPLE_RADIAL": 1, "RADIAL": 2, "OPENCV": 4, "OPENCV_FISHEYE": 4}.get(model)
            coeff = np.asarray(coeff, dtype=np.float64)
            if ncoef is None or coeff.shape not in ((ncoef,), (V, ncoef)):
                raise ValueError("distortion must be (coefficients, model): SIMPLE_RADIAL [1], RADIAL [2], OPENCV [4] or OPENCV_FISHEYE [4] numbers, or [V, n] of them")
            coeff = np.broadcast_to(coeff, (V, ncoef))
            rows = [r + tuple(float(x) for x in c) for r, c in zip(rows, coeff)]
        cam_rows = list(dict.fromkeys(rows))
        cam_id = {r: n + 1 for n, r in enumerate(cam_rows)}
        if distortion is not None:
            mid = {name: i for i, (name, _) in COLMAP_MODELS.items()}[model]
            if model in ("SIMPLE_RADIAL", "RADIAL"):
                if any(r[0] != r[1] for r in cam_rows):
                    raise ValueError(f"{model} has one focal length: it needs fx == fy")
                cam_params = [(r[0], r[2], r[3]) + r[4:] for r in cam_rows]
            else:
                cam_params = cam_rows
            lens = [lens_row(model, cam_params[cam_id[r] - 1])[1:] for r in rows]            # per view (family, row [8])
        elif model == "PINHOLE":
            mid, cam_params = 1, [r for r in cam_rows]
        elif model == "SIMPLE_PINHOLE" and all(r[0] == r[1] for r in cam_rows):
            mid, cam_params = 0, [(r[0], r[2], r[3]) for r in cam_rows]
        else:
            raise ValueError("save_colmap writes PINHOLE, or SIMPLE_PINHOLE when fx == fy")
        # back to COLMAP's frame: undo the scale, then the convention change (its own inverse on the world side)
        poses = self.poses.double().cpu().numpy().copy()
        poses[:, :3, 3] /= scale
        poses, pw = _world_flip(poses, points / scale)         # its own inverse: sign changes and a swap, which commute
        if keypoints is None:
            keypoints = []
            for v in range(V):
                pc = (pw - poses[v, :3, 3]) @ poses[v, :3, :3]          # camera coordinates (x right, y down, z forward)
                fx, fy, cx, cy = rows[v][:4]
                with np.errstate(divide="ignore", invalid="ignore"):
                    if lens is None:
                        x, y = fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy
                    else:
                        x, y = lens_distort(*lens[v], pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2])
                        x, y = fx * x + cx, fy * y + cy
                m = (pc[:, 2] > 0) & (x >= 0) & (x < self.W) & (y >= 0) & (y < self.H)
                keypoints.append((np.stack([x[m], y[m]], -1), np.nonzero(m)[0]))
        root = os.path.join(path, *folder.split("/"))
        os.makedirs(root, exist_ok=True)
        os.makedirs(os.path.join(path, "images"), exist_ok=True)
        write_colmap_cameras(os.path.join(root, "cameras.bin"), mid, self.W, self.H, cam_params)
        qt, kp_ids = [], []
        for v in range(V):
            Rt = poses[v, :3, :3].T                                  # world-to-camera rotation
            qt.append(np.concatenate([rotmat_to_quat(Rt), -Rt @ poses[v, :3, 3]]))
            xy, idx = keypoints[v]
            xy, idx = np.asarray(xy, dtype=np.float64).reshape(-1, 2), np.asarray(idx, dtype=np.int64).reshape(-1)
            kp_ids.append((xy, np.where(idx >= 0, ids[np.clip(idx, 0, M - 1)], -1)))
        tracks = write_colmap_images(os.path.join(root, "images.bin"), qt, [cam_id[r] for r in rows], names, kp_ids)
        by = self.bank_bytes().cpu().numpy()
        for v in range(V):
            Image.fromarray(by[v] if self.has_alpha else np.ascontiguousarray(by[v, :, :, :3])).save(os.path.join(path, "images", names[v]))
        if depths is not None:
            if len(depths) != V or any(np.ndim(d) != 2 for d in depths):
                raise ValueError(f"depths must be one 2-D array per view ({V} views)")
            os.makedirs(os.path.join(path, "depths"), exist_ok=True)
            for v in range(V):
                np.save(os.path.join(path, "depths", os.path.splitext(names[v])[0] + ".npy"), np.asarray(depths[v]))
        write_colmap_points(os.path.join(root, "points3D.bin"), ids, pw, errors, tracks)

    def save_dtu(self, path, scale=1.0, offset=(0, 0, 0)):
        """Writes the set in the DTU layout (cameras_sphere.npz with world_mat_i = K_i [R_i | -R_i C_i] padded to 4 x 4 and an identity
        scale_mat_i, float64; image/NNN.png, mask/NNN.png) such that load_dtu(path, "all", scale, offset) gives it back: the bank byte
        for byte, rows and poses up to the rounding of the fp32 product and its decomposition.  A shared set writes its one K for every
        view.  Mirrors save_colmap; a set without alpha gets all-255 masks (and comes back with has_alpha)."""
        from PIL import Image
        for sub in ("image", "mask"):
            os.makedirs(os.path.join(path, sub), exist_ok=True)
        poses = self.poses.double().cpu().numpy().copy()
        poses[:, 2] *= -1                              # the three axis fixes of load_dtu, undone last to first
        poses = poses[:, [1, 0, 2, 3], :]
        poses[:, :3, 1:3] *= -1
        poses[:, :3, 3] = (poses[:, :3, 3] - np.array(offset, dtype=np.float64)) / scale
        by = self.bank_bytes().cpu().numpy()
        mats = {}
        for v in range(len(self)):
            fx, fy, cx, cy = self.intrinsics_of(v)
            K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float64)
            R, C = poses[v, :3, :3].T, poses[v, :3, 3]
            world = np.eye(4)
            world[:3, :3], world[:3, 3] = K @ R, -K @ R @ C
            mats[f"world_mat_{v}"], mats[f"scale_mat_{v}"] = world, np.eye(4)
            Image.fromarray(np.ascontiguousarray(by[v, :, :, :3])).save(os.path.join(path, "image", f"{v:03d}.png"))
            Image.fromarray(np.ascontiguousarray(by[v, :, :, 3])).save(os.path.join(path, "mask", f"{v:03d}.png"))
        np.savez(os.path.join(path, "cameras_sphere.npz"), **mats)
