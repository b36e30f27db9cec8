"""Test mode: cameras that are not in the set, and the frame sequences rendered from them.

The reference's `main.py --test` builds a trajectory of cameras without images (type='test': nerf/provider.py:168-184,
nerf/colmap_provider.py:346-402, nerf/dtu_provider.py:114-170), renders every frame (test_step, nerf/utils.py:865-889) and writes RGB and
normalised-depth frames or videos (Trainer.test, nerf/utils.py:953-1008).  Here:

  CameraPath                a set of cameras without images that offers the part of capture.Capture's interface the renderer factories of
                            metrics.py use (len, H, W, device, poses, intrinsics, intrinsics_of, mvps, cam_near_far, view): field_renderer,
                            mesh_renderer and asset_renderer take one where they take a Capture.
    CameraPath.between      the reference's default path: random key views, a sine-eased slerp / lerp between consecutive keys
    CameraPath.circle       camera_traj == 'circle': a small circle of look-at poses
  frame_pack                one rendered frame -> the uint8 RGB and depth bytes Trainer.test writes (n2m_frame_pack on the device; its torch
                            statement frame_pack_torch on CPU tensors)
  render_path               every frame of a path through a renderer into preallocated uint8 stacks
  save_frames               the stacks as {name}_{i:04d}_rgb.png / _depth.png (the reference's no-video file names) and, optionally, as animated
                            PNGs.  The reference writes mp4 through imageio.mimwrite; no mp4 encoder is assumed here, so video="apng" writes
                            {name}_rgb.apng / {name}_depth.apng with PIL instead, and the padding to even sizes of nerf/utils.py:1002-1003 --
                            an ffmpeg need -- is dropped.

The path arithmetic runs on the host in float64 numpy and is cast to fp32 once; nothing here imports scipy.
"""
import math
import os

import numpy as np
import torch

from .capture import Capture, proj_matrix, rays_from_pixels
from .colmap_model import quat_to_rotmat, rotmat_to_quat


def slerp_rotation(R0, R1, ratio):
    """The rotation a fraction `ratio` of the way from R0 to R1 along the shortest arc (what scipy's Slerp([0, 1], [R0, R1])(ratio) gives):
    unit quaternions, q1 negated when it lies in the other hemisphere, sin-weighted sum; float64.  Two keys closer than 1e-12 rad: R0."""
    q0, q1 = rotmat_to_quat(np.asarray(R0, dtype=np.float64)), rotmat_to_quat(np.asarray(R1, dtype=np.float64))
    c = float(np.dot(q0, q1))
    if c < 0:
        q1, c = -q1, -c
    s = float(np.linalg.norm(q1 - c * q0))            # sin of the angle between the quaternions, without the cancellation of sqrt(1 - c^2)
    omega = math.atan2(s, c)
    if omega < 1e-12:
        return quat_to_rotmat(q0)
    q = (math.sin((1 - ratio) * omega) * q0 + math.sin(ratio * omega) * q1) / math.sin(omega)
    return quat_to_rotmat(q / np.linalg.norm(q))


def ease(i, n_test):
    """nerf/colmap_provider.py:390: the sine ease of frame i of a segment, 0 at i = 0 and 1 at i = n_test."""
    return math.sin((i / n_test - 0.5) * math.pi) * 0.5 + 0.5


def between_poses(poses, keys, n_test):
    """fp32 [(K-1)(n_test+1),4,4]: for every consecutive pair of `keys` (rows of poses [V,4,4] fp32) the frames i = 0..n_test of
    nerf/colmap_provider.py:385-395 -- rotation slerp(ratio), translation (1 - ratio) t0 + ratio t1, ratio = ease(i).  Float64 from the fp32
    poses, cast once; the frames i = 0 and i = n_test are the key poses themselves, bit for bit (the reference emits their round trip through
    the slerp); a key shared by two segments therefore appears twice, as in the reference."""
    poses = np.asarray(poses, dtype=np.float32)
    n_test = int(n_test)
    if n_test < 1:
        raise ValueError("n_test must be at least 1")
    out = []
    for a, b in zip(keys[:-1], keys[1:]):
        p0, p1 = poses[int(a)].astype(np.float64), poses[int(b)].astype(np.float64)
        for i in range(n_test + 1):
            if i == 0 or i == n_test:
                out.append(poses[int(a if i == 0 else b)].copy())
                continue
            ratio = ease(i, n_test)
            pose = np.eye(4, dtype=np.float64)
            pose[:3, :3] = slerp_rotation(p0[:3, :3], p1[:3, :3], ratio)
            pose[:3, 3] = (1 - ratio) * p0[:3, 3] + ratio * p1[:3, 3]
            out.append(pose.astype(np.float32))
    return np.stack(out)


def circle_poses(n=100, radius=0.1, theta_deg=80):
    """fp32 [n,4,4]: nerf/colmap_provider.py:356-376 (the same in nerf/dtu_provider.py) -- centres on a circle at polar angle theta, columns
    (right, up, forward) with forward = normalize(centre), normalize(v) = v / (|v| + 1e-10); float64, cast once."""
    normalize = lambda v: v / (np.linalg.norm(v) + 1e-10)
    theta = np.deg2rad(theta_deg)
    out = []
    for i in range(int(n)):
        phi = np.deg2rad(i / n * 360)
        center = np.array([radius * np.sin(theta) * np.sin(phi), radius * np.sin(theta) * np.cos(phi), radius * np.cos(theta)])
        forward = normalize(center)
        right = normalize(np.cross(forward, np.array([0.0, 0.0, 1.0])))
        up = normalize(np.cross(right, forward))
        pose = np.eye(4)
        pose[:3, :3] = np.stack((right, up, forward), axis=-1)
        pose[:3, 3] = center
        out.append(pose.astype(np.float32))
    return np.stack(out)


class CameraPath:
    """F cameras of one size and ONE camera model without images.  poses [F,4,4] fp32 and mvps [F,4,4] on `device`; mvps are built as
    Capture builds them (proj_matrix(...) @ inverse(pose), per pose on the host)."""

    cam_near_far = None
    per_view_intrinsics = False

    def __init__(self, poses, H, W, intrinsics, device="cpu"):
        poses_cpu = torch.as_tensor(np.asarray(poses.detach().cpu() if torch.is_tensor(poses) else poses)).float().contiguous()
        if poses_cpu.dim() != 3 or poses_cpu.shape[1:] != (4, 4) or poses_cpu.shape[0] < 1:
            raise ValueError("poses must be [F,4,4] with F >= 1")
        intr = tuple(float(x) for x in intrinsics)
        if len(intr) != 4:
            raise ValueError("intrinsics must be (fx, fy, cx, cy)")
        self.H, self.W, self.intrinsics = int(H), int(W), intr
        self.poses = poses_cpu.to(device)
        self.device = self.poses.device
        proj = proj_matrix(self.H, self.W, *intr)
        self.mvps = torch.stack([proj @ torch.inverse(p) for p in poses_cpu]).to(self.device)

    def __len__(self):
        return int(self.poses.shape[0])

    def intrinsics_of(self, f):
        return self.intrinsics

    # ------------------------------------------------------------------------------------------------ constructors
    @classmethod
    def between(cls, capture, n_test=24, n_keys=5, seed=0, keys=None):
        """The reference's default test path (nerf/colmap_provider.py:383-397; nerf/provider.py:171-184 is the same with two keys) through
        views of `capture`: keys, or np.random.RandomState(seed).choice(V, min(n_keys, V), replace=False).  F = (K - 1)(n_test + 1).  The
        intrinsics are view 0's (colmap_provider.py:400), also for a per-view set."""
        V = len(capture)
        if V < 2:
            raise ValueError(f"a path between views needs at least 2 views, the set has {V}")
        if keys is None:
            keys = np.random.RandomState(seed).choice(V, min(int(n_keys), V), replace=False)
        keys = [int(k) for k in keys]
        if len(keys) < 2 or any(k < 0 or k >= V for k in keys):
            raise ValueError(f"a path needs at least 2 keys, each a view 0..{V - 1}; got {keys}")
        path = cls(between_poses(capture.poses.detach().cpu().numpy(), keys, n_test), capture.H, capture.W, capture.intrinsics_of(0), capture.device)
        path.keys, path.n_test = keys, int(n_test)
        return path

    @classmethod
    def circle(cls, capture_or_hw_intrinsics, n=100, radius=0.1, theta_deg=80, device=None):
        """camera_traj == 'circle'.  The camera comes from a Capture (its size, view 0's intrinsics, its device) or from a tuple
        (H, W, (fx, fy, cx, cy)) (then `device`, default the CPU)."""
        src = capture_or_hw_intrinsics
        if isinstance(src, (Capture, CameraPath)):
            H, W, intr, dev = src.H, src.W, src.intrinsics_of(0), src.device if device is None else device
        else:
            H, W, intr = src
            dev = "cpu" if device is None else device
        return cls(circle_poses(n, radius, theta_deg), H, W, intr, dev)

    # ------------------------------------------------------------------------------------------------------- access
    def view(self, f, stride=1, dirs_ssaa=0):
        """Capture.view without the image: (rays_o, rays_d [h*w,3], None, dirs [h*ssaa * w*ssaa, 3] | None).  On the GPU one kernel
        (n2m_path_view, the bits of n2m_capture_view); on the CPU the torch statement Capture.view takes."""
        s, a = int(stride), int(dirs_ssaa)
        h, w = self.H // s, self.W // s
        dev = self.device
        if dev.type == "cuda":
            from . import _lib as L
            e = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
            o, d = e(h * w, 3), e(h * w, 3)
            dirs = e(h * a * w * a, 3) if a >= 1 else None
            if h * w == 0:                                 # a stride above the size: nothing to launch
                return o, d, None, dirs
            with torch.cuda.device(dev):
                L.call("n2m_path_view", L.ptr(self.poses), len(self), int(f), self.H, self.W, s, *self.intrinsics, L.ptr(o), L.ptr(d), L.ptr(dirs),
                       max(a, 1), L.stream())
            return o, d, None, dirs
        jj, ii = torch.meshgrid(torch.arange(h, device=dev) * s, torch.arange(w, device=dev) * s, indexing="ij")
        jj, ii = jj.reshape(-1), ii.reshape(-1)
        o, d = rays_from_pixels(self.poses, int(f), ii, jj, self.intrinsics)
        dirs = None
        if a >= 1:
            n2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            unit = d / torch.clamp(n2, min=1e-20).double().sqrt().float().unsqueeze(-1)        # the correctly rounded fp32 root (see Capture.view)
            dirs = unit.view(h, 1, w, 1, 3).expand(h, a, w, a, 3).reshape(-1, 3).contiguous()
        return o, d, None, dirs


# ------------------------------------------------------------------------------------------------------ frames as bytes
def linear_to_srgb(x):
    """nerf/utils.py:45-46 linear_to_srgb."""
    return torch.where(x < 0.0031308, 12.92 * x, 1.055 * x ** 0.41666 - 0.055)


def frame_pack_torch(image, depth, linear=False):
    """The torch statement of n2m_frame_pack (nerf/utils.py:978-986): image [...,3] fp32, depth [...] fp32 -> (uint8, uint8) of the same
    shapes.  RGB: clamp to [0, 1] (a deviation: the reference lets a value above 1 wrap in astype(uint8)), under `linear` linear_to_srgb and
    the clamp again, then (x * 255) truncated.  Depth: ((d - min) / (max - min + 1e-6)) * 255 truncated, every operation in fp32."""
    x = image.float().clamp(0, 1)
    if linear:
        x = linear_to_srgb(x).clamp(0, 1)
    rgb = (x * 255).to(torch.uint8)
    d = depth.float()
    mn, mx = d.min(), d.max()
    return rgb, (((d - mn) / (mx - mn + 1e-6)) * 255).to(torch.uint8)


_PARTIALS = {}


def frame_pack(image, depth, linear=False, out=None):
    """One rendered frame as bytes: image [n,3] (or [H,W,3]) and depth [n] (or [H,W]) fp32, finite -> (rgb uint8, depth uint8) of the same
    shapes, written into `out` = (rgb_out, depth_out) when given (contiguous; slices of a stack).  On the GPU n2m_frame_pack (two launches,
    no host read); on the CPU frame_pack_torch."""
    n = depth.numel()
    if image.numel() != 3 * n:
        raise ValueError(f"image {tuple(image.shape)} and depth {tuple(depth.shape)} are not one frame")
    if not image.is_cuda:
        rgb, dep = frame_pack_torch(image, depth, linear)
        if out is not None:
            out[0].view(-1).copy_(rgb.reshape(-1))
            out[1].view(-1).copy_(dep.reshape(-1))
            return out
        return rgb, dep
    from . import _lib as L
    dev = image.device
    image, depth = image.detach().float().contiguous(), depth.detach().float().contiguous()
    if out is None:
        out = (torch.empty(image.shape, dtype=torch.uint8, device=dev), torch.empty(depth.shape, dtype=torch.uint8, device=dev))
    rgb, dep = out
    if rgb.dtype != torch.uint8 or dep.dtype != torch.uint8 or rgb.numel() != 3 * n or dep.numel() != n or not (rgb.is_contiguous() and dep.is_contiguous()) \
            or rgb.device != dev or dep.device != dev:
        raise ValueError("out must be contiguous uint8 tensors of 3 n and n elements on the frame's device")
    if n >= 1 << 32:
        raise ValueError("a frame holds fewer than 2^32 pixels")
    partials = _PARTIALS.get(dev)                      # uses on one stream are ordered; written by every call before it is read
    if partials is None:
        partials = _PARTIALS[dev] = torch.empty(L.FRAME_PACK_PARTIALS, 2, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.call("n2m_frame_pack", L.ptr(image), L.ptr(depth), n, int(bool(linear)), L.ptr(rgb), L.ptr(dep), L.ptr(partials), L.stream())
    return rgb, dep


@torch.no_grad()
def render_path(render, path, frames=None, linear=False):
    """Walks `frames` (default: all) of `path` through `render` -- metrics.field_renderer / mesh_renderer / asset_renderer built on the path, or
    any f -> {"image": [H*W,3], "depth": [H*W]} -- and packs every frame into preallocated stacks on the renderer's device:
    (rgb [F,H,W,3] uint8, depth [F,H,W] uint8).  linear: the renderer works in linear colour (--color_space linear)."""
    frames = list(range(len(path))) if frames is None else [int(f) for f in frames]
    H, W = path.H, path.W
    rgb = depth = None
    for k, f in enumerate(frames):
        res = render(f)
        image, dep = res["image"].detach().reshape(H * W, 3), res["depth"].detach().reshape(H * W)
        if rgb is None:
            rgb = torch.empty(len(frames), H, W, 3, dtype=torch.uint8, device=image.device)
            depth = torch.empty(len(frames), H, W, dtype=torch.uint8, device=image.device)
        frame_pack(image, dep, linear, out=(rgb[k], depth[k]))
    if rgb is None:
        dev = path.device
        return torch.empty(0, H, W, 3, dtype=torch.uint8, device=dev), torch.empty(0, H, W, dtype=torch.uint8, device=dev)
    return rgb, depth


def save_frames(rgb, depth, save_path, name, video=None):
    """rgb [F,H,W,3] uint8 and depth [F,H,W] uint8 -> {save_path}/{name}_{i:04d}_rgb.png and _depth.png (Trainer.test's no-video names,
    nerf/utils.py:992-993), through PIL.  video="apng" also writes {name}_rgb.apng and {name}_depth.apng (PIL's save_all, 24 frames a second
    like the reference's mp4): the stand-in for imageio.mimwrite, without its padding to even sizes.  Returns the list of files written."""
    from PIL import Image
    if video not in (None, "apng"):
        raise ValueError(f"video must be None or 'apng', not {video!r}")
    rgb, depth = np.ascontiguousarray(torch.as_tensor(rgb).cpu().numpy()), np.ascontiguousarray(torch.as_tensor(depth).cpu().numpy())
    if rgb.dtype != np.uint8 or depth.dtype != np.uint8 or rgb.ndim != 4 or rgb.shape[-1] != 3 or depth.shape != rgb.shape[:3]:
        raise ValueError("rgb must be uint8 [F,H,W,3] and depth uint8 [F,H,W]")
    os.makedirs(save_path, exist_ok=True)
    written = []
    for i in range(rgb.shape[0]):
        for arr, kind in ((rgb[i], "rgb"), (depth[i], "depth")):
            written.append(os.path.join(save_path, f"{name}_{i:04d}_{kind}.png"))
            Image.fromarray(arr).save(written[-1])
    if video == "apng" and rgb.shape[0] > 0:
        for stack, kind in ((rgb, "rgb"), (depth, "depth")):
            ims = [Image.fromarray(a) for a in stack]
            written.append(os.path.join(save_path, f"{name}_{kind}.apng"))
            ims[0].save(written[-1], format="PNG", save_all=True, append_images=ims[1:], duration=1000 / 24, loop=0)
    return written


def path_for(capture, opt=None, n_test=24, seed=0):
    """The path a front end renders: opt.camera_traj == "circle" -> CameraPath.circle, "" -> CameraPath.between."""
    traj = getattr(opt, "camera_traj", "") if opt is not None else ""
    if traj == "circle":
        return CameraPath.circle(capture)
    if traj != "":
        raise ValueError(f"camera_traj must be '' or 'circle', not {traj!r}")
    return CameraPath.between(capture, n_test=n_test, seed=seed)
