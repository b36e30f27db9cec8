"""A captured image set as a data source for both stages: cameras with real intrinsics and a uint8 image bank resident on the device.

The reference keeps its training images on the device as uint8 [N,H,W,3|4], divides by 255 when it gathers a batch and converts
sRGB -> linear under `--color_space linear` (nerf/provider.py:237,323-325; nerf/utils.py:640).  `Capture` holds the same data as ONE packed
RGBA8 word per pixel (R in the low byte; a 3-channel source stores alpha 255 and sets has_alpha = False) and decodes through a [2,256]
fp32 table built once per set with the reference's own torch expressions (row 0: R, G, B; row 1: alpha) -- what the kernels of
csrc/capture.hip gather is therefore bit for bit what the torch statement computes, without a device pow.

Every kernel has its torch statement here (batch_from_uniforms_u8, Capture.view, box_downscale); Python takes it when the tensors are on
the CPU, like synthetic.batch_from_uniforms, and the GPU tests compare the kernels against it.

One camera model per set (H, W, fx, fy, cx, cy), as in the reference's providers; H != W, fx != fy and an off-centre principal point
are allowed.  `mvps` is built FROM those intrinsics (proj_matrix), so the rasteriser of stage 1 and the rays of stage 0 see the same
camera; the reference's projection (nerf/provider.py:266-276) ignores cx, cy and fl_x, so off-centre its rays and its raster disagree.
"""
import json
import math
import os

import numpy as np
import torch

from . import synthetic

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
    """synthetic.rays_from_pixels (get_rays, nerf/utils.py:242-290) at intrinsics (fx, fy, cx, cy): pixel column pix_i, row pix_j."""
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


def batch_from_uniforms_u8(poses, bank, lut, u, aabb, min_near, H, W, intrinsics, out=None, counter=None, cam_near_far=None):
    """synthetic.batch_from_uniforms with the ground truth gathered from a packed uint8 bank [V,H*W] and decoded through `lut`.  On the GPU
    one kernel (n2m_batch_rays_u8); below it the torch statement of the same arithmetic, taken on the CPU."""
    dev = poses.device
    N, V = u.shape[0], poses.shape[0]
    fx, fy, cx, cy = (float(x) for x in intrinsics)
    if dev.type == "cuda":
        from . import _lib as L
        if out is None:
            f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
            out = (f(N, 3), f(N, 3), f(N, 4), f(N), f(N), f(N), f(N, 3))
        o, d, rgba, nears, fars, noises, bg = out
        L.call("n2m_batch_rays_u8", L.ptr(poses), L.ptr(u), V, N, H, W, fx, fy, cx, cy, L.ptr(bank), L.ptr(lut), L.ptr(aabb), float(min_near),
               L.ptr(o), L.ptr(d), L.ptr(rgba), L.ptr(nears), L.ptr(fars), L.ptr(noises), L.ptr(bg), L.ptr(counter), L.ptr(cam_near_far), L.stream())
        return o, d, rgba, nears, fars, noises, bg
    cam = (u[:, 0] * V).long().clamp(max=V - 1)
    pix = (u[:, 1] * (H * W)).long().clamp(max=H * W - 1)
    o, d = rays_from_pixels(poses, cam, pix % W, torch.div(pix, W, rounding_mode="floor"), (fx, fy, cx, cy))
    inv = 1.0 / d
    lo, hi = (aabb[:3] - o) * inv, (aabb[3:] - o) * inv
    tn, tf = torch.minimum(lo, hi).amax(-1), torch.maximum(lo, hi).amin(-1)
    miss = tn > tf
    big = torch.finfo(torch.float32).max
    nears = torch.where(miss, torch.full_like(tn, big), tn.clamp(min=min_near))
    fars = torch.where(miss, torch.full_like(tf, big), tf)
    if cam_near_far is not None:
        nears = torch.maximum(nears, cam_near_far[cam, 0])
        fars = torch.minimum(fars, cam_near_far[cam, 1])
    if counter is not None:
        counter.zero_()
    return o, d, decode_words(bank[cam, pix], lut), nears, fars, u[:, 2].contiguous(), u[:, 3:6].contiguous()


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


class Capture:
    """poses [V,4,4] fp32 (camera-to-world, OpenGL: the engines' convention), H, W, intrinsics (fx, fy, cx, cy), bank [V,H*W] packed RGBA8
    (int32 storage) on `device`, has_alpha, linear (opt.color_space == 'linear'), optional cam_near_far [V,2], mvps [V,4,4].  It can be handed
    to export_stage0 as its `dataset` (.mvps, .H, .W)."""

    def __init__(self, poses, bank, H, W, intrinsics, has_alpha=True, linear=False, cam_near_far=None, device=None):
        device = torch.device(device if device is not None else bank.device)
        self.device = device
        self.H, self.W = int(H), int(W)
        self.intrinsics = tuple(float(x) for x in intrinsics)
        poses_cpu = torch.as_tensor(poses).detach().float().cpu().contiguous()
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
        proj = proj_matrix(self.H, self.W, *self.intrinsics)
        self.mvps = torch.stack([proj @ torch.inverse(p) for p in poses_cpu]).to(device)      # per pose on the host, like synthetic.mvp_matrix

    # ------------------------------------------------------------------------------------------------ constructors
    @classmethod
    def from_arrays(cls, poses, images_uint8, intrinsics, linear=False, cam_near_far=None, downscale=1, device="cpu"):
        """poses [V,4,4], images uint8 [V,H,W,3|4] (numpy or torch), intrinsics (fx, fy, cx, cy) of the images as given; downscale=k takes
        the k x k integer block mean on `device` and divides the intrinsics by k."""
        images = torch.as_tensor(images_uint8)
        V, H, W, _ = images.shape
        bank, has_alpha = pack_rgba8(images)
        bank = bank.to(device)
        k = int(downscale)
        if k < 1:
            raise ValueError("downscale must be a positive integer")
        if k > 1:
            bank = box_downscale(bank, H, W, k)
            H, W, intrinsics = H // k, W // k, tuple(float(x) / k for x in intrinsics)
        return cls(poses, bank, H, W, intrinsics, has_alpha=has_alpha, linear=linear, cam_near_far=cam_near_far, device=device)

    @classmethod
    def load_nerf(cls, path, split="train", scale=0.33, offset=(0, 0, 0), downscale=1, linear=False, device="cpu"):
        """transforms_{split}.json (else transforms.json) by the rules of nerf/provider.py:150-263: H, W from h / w or the first image, focal
        from fl_x / fl_y else camera_angle_x / camera_angle_y, cx, cy default to W / 2, H / 2, `.png` appended to a file name without an
        extension, missing files skipped, poses through nerf_matrix_to_ngp.  Images are read with PIL."""
        from PIL import Image
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
            with Image.open(fp) as im:
                if im.mode not in ("RGB", "RGBA"):
                    im = im.convert("RGBA" if "A" in im.getbands() or "transparency" in im.info else "RGB")
                images.append(np.asarray(im, dtype=np.uint8))
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
    def synthetic(cls, poses, scene="lego", H=synthetic.LEGO_HW, W=synthetic.LEGO_HW, intrinsics=None, alpha=True, linear=False,
                  cam_near_far=None, device=None, chunk=1 << 20):
        """The box scene rendered through synthetic.render_gt at arbitrary intrinsics (default: the lego camera) and quantised with
        (x * 255 + 0.5).to(uint8); alpha=False composites on white and keeps three channels."""
        poses = torch.as_tensor(poses).float()
        dev = torch.device(device if device is not None else poses.device)
        if intrinsics is None:
            intrinsics = (synthetic.LEGO_FOCAL, synthetic.LEGO_FOCAL, W / 2, H / 2)
        intr = tuple(float(x) for x in intrinsics)
        pd, bx = poses.to(dev), synthetic.boxes(dev, scene)
        V = poses.shape[0]
        images = torch.empty(V, H * W, 4 if alpha else 3, dtype=torch.uint8, device=dev)
        pix = torch.arange(H * W, device=dev)
        for v in range(V):
            for s in range(0, H * W, chunk):
                p = pix[s:s + chunk]
                o, d = rays_from_pixels(pd, torch.full_like(p, v), p % W, torch.div(p, W, rounding_mode="floor"), intr)
                rgba = synthetic.render_gt(o, d, bx)
                if not alpha:
                    rgba = rgba[:, :3] * rgba[:, 3:] + (1 - rgba[:, 3:])
                images[v, s:s + chunk] = (rgba * 255 + 0.5).to(torch.uint8)
        return cls.from_arrays(poses, images.view(V, H, W, -1), intr, linear=linear, cam_near_far=cam_near_far, device=dev)

    # ------------------------------------------------------------------------------------------------------- access
    def check_device(self, device):
        """Raises when a driver on `device` is handed this set: the bank is gathered from where it lies, never copied per batch."""
        if torch.empty(0, device=device).device != self.device:
            raise ValueError(f"the capture lives on {self.device}, the driver on {device}")

    def __len__(self):
        return int(self.poses.shape[0])

    @property
    def nbytes(self):
        return self.bank.numel() * 4

    def bank_bytes(self):
        """uint8 view [V,H,W,4] of the bank (R, G, B, A)."""
        return self.bank.view(torch.uint8).view(len(self), self.H, self.W, 4)

    def decode(self, view=None):
        """The fp32 images the kernels gather from: [V,H*W,4], or [H*W,4] of one view."""
        return decode_words(self.bank if view is None else self.bank[view], self.lut)

    def view(self, v, stride=1, dirs_ssaa=0):
        """One whole view at pixel stride `stride` (h = H // stride, w = W // stride, pixel (j * stride, i * stride)): rays_o, rays_d [h*w,3],
        rgba [h*w,4], and with dirs_ssaa >= 1 the unit directions [h*ssaa * w*ssaa, 3] stage 1 shades with (safe_normalize of every pixel's
        direction, repeated ssaa x ssaa times) -- else None.  On the GPU one kernel (n2m_capture_view)."""
        s, a = int(stride), int(dirs_ssaa)
        h, w = self.H // s, self.W // s
        dev = self.device
        if dev.type == "cuda":
            from . import _lib as L
            f = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
            o, d, rgba = f(h * w, 3), f(h * w, 3), f(h * w, 4)
            dirs = f(h * a * w * a, 3) if a >= 1 else None
            L.call("n2m_capture_view", L.ptr(self.poses), len(self), int(v), self.H, self.W, s, *self.intrinsics, L.ptr(self.bank), L.ptr(self.lut),
                   L.ptr(o), L.ptr(d), L.ptr(rgba), L.ptr(dirs), max(a, 1), L.stream())
            return o, d, rgba, dirs
        jj, ii = torch.meshgrid(torch.arange(h, device=dev) * s, torch.arange(w, device=dev) * s, indexing="ij")
        jj, ii = jj.reshape(-1), ii.reshape(-1)
        o, d = rays_from_pixels(self.poses, int(v), ii, jj, self.intrinsics)
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
