"""Image metrics on the device, and the held-out evaluation built on them.

  ssim(pred, target)        SSIM (Wang et al. 2004) as an autograd Function over csrc/metrics.hip: 11 x 11 Gaussian window (sigma 1.5),
                            C1 = 0.01^2, C2 = 0.03^2, data range 1 -- the defaults of the structural_similarity_index_measure call in the
                            reference's commented-out SSIM meter (nerf/utils.py:351-465) -- over VALID windows only (no padded border: the
                            map of an [H, W, C] pair is [H - 10, W - 10, C]).  There is no host path: CPU tensors raise.
  ssim_patches(pred, target)  the same SSIM over a batch of square patches [B, P, P, C] (11 <= P <= 64), every patch on its own, in one launch
                            pair: the structural term of a stage-0 patch batch (trainer.Stage0Trainer, patch_size / lambda_patch_ssim).
  psnr(a, b)                asset.psnr, re-exported.
  evaluate_views(...)       per-view and mean PSNR / SSIM of a renderer against a capture's ground truth (the reference's eval_step
                            blends it on white, nerf/utils.py:794-811), with a renderer factory per stage's product: field_renderer (stage 0),
                            mesh_renderer (render_stage1), asset_renderer (the exported files, ExportedAsset.render).

LPIPS, the reference's other meter and its only structural training term, needs VGG weights and the `lpips` package; neither is part of
this repository, so it is not built.  `1 - ssim` is the structural term offered instead: of the whole frame in stage 1
(trainer.Stage1Trainer, lambda_ssim), of the batch's patches in stage 0 (trainer.Stage0Trainer, lambda_patch_ssim).
"""
import ctypes

import numpy as np
import torch

from . import _lib as L
from .asset import psnr  # noqa: F401  (re-export)

WINDOW, SIGMA = 11, 1.5


def gaussian_taps():
    """The window's 11 taps: float64 exp, normalised to sum 1 (the kernel is handed these rounded to fp32; no device exp decides anything)."""
    d = np.arange(WINDOW, dtype=np.float64) - (WINDOW - 1) / 2
    g = np.exp(-(d * d) / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


_TAPS = (ctypes.c_float * WINDOW)(*[float(np.float32(t)) for t in gaussian_taps()])


def _check_shape(H, W, C):
    if H < WINDOW or W < WINDOW:
        raise ValueError(f"ssim: H and W must be at least {WINDOW} (valid windows only), got {H} x {W}")
    if C not in (1, 3):
        raise ValueError(f"ssim: C must be 1 or 3, got {C}")


class _SSIM(torch.autograd.Function):
    """(mean, map | None) of fp32 contiguous device images x, y [H, W, C].  The three per-window derivative maps are written and saved only
    when x needs a gradient; the backward is one gather launch (n2m_ssim_backward), the same bits on every run."""

    @staticmethod
    def forward(ctx, x, y, want_map):
        H, W, C = x.shape
        dev = x.device
        need = ctx.needs_input_grad[0]
        smap = torch.empty(H - WINDOW + 1, W - WINDOW + 1, C, dtype=torch.float32, device=dev) if want_map else None
        dS = torch.empty(3, H - WINDOW + 1, W - WINDOW + 1, C, dtype=torch.float32, device=dev) if need else None
        partials = torch.empty(L.lib().n2m_ssim_partials(H, W), dtype=torch.float32, device=dev)
        out = torch.empty(1, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            L.call("n2m_ssim_forward", L.ptr(x), L.ptr(y), H, W, C, _TAPS, L.ptr(smap), L.ptr(dS), L.ptr(partials), L.ptr(out), L.stream())
        if need:
            ctx.save_for_backward(x, y, dS)
        if want_map:
            ctx.mark_non_differentiable(smap)
        return out.view(()), smap

    @staticmethod
    def backward(ctx, g, _gmap):
        x, y, dS = ctx.saved_tensors
        H, W, C = x.shape
        g = g.detach().to(torch.float32).reshape(1).contiguous()
        grad = torch.empty_like(x)
        with torch.cuda.device(x.device):
            L.call("n2m_ssim_backward", L.ptr(x), L.ptr(y), L.ptr(dS), H, W, C, _TAPS, L.ptr(g), L.ptr(grad), L.stream())
        return grad, None, None


def ssim(pred, target, return_map=False, hw=None):
    """Mean SSIM of `pred` against `target` (0-dim fp32 tensor on the device; differentiable in pred, not in target), and with return_map
    the per-window map [H - 10, W - 10, C] too.  Images are [H, W, C], or [H * W, C] with hw=(H, W); C is 1 or 3, H, W >= 11.
    Shapes the kernel refuses raise ValueError, CPU tensors RuntimeError (the package has no host path)."""
    if hw is not None:
        H, W = int(hw[0]), int(hw[1])
        if pred.dim() != 2 or pred.shape[0] != H * W:
            raise ValueError(f"ssim: hw={tuple(hw)} needs [H * W, C] images, got {tuple(pred.shape)}")
        pred, target = pred.reshape(H, W, pred.shape[-1]), target.reshape(H, W, target.shape[-1])
    if pred.dim() != 3 or pred.shape != target.shape:
        raise ValueError(f"ssim: images must be two [H, W, C] tensors of one shape, got {tuple(pred.shape)} and {tuple(target.shape)}")
    _check_shape(*pred.shape)
    if not (pred.is_cuda and target.is_cuda):
        raise RuntimeError("ssim: pred and target must be CUDA tensors (there is no host path)")
    mean, smap = _SSIM.apply(pred.float().contiguous(), target.detach().float().contiguous(), bool(return_map))
    return (mean, smap) if return_map else mean


PATCH_MIN, PATCH_MAX = WINDOW, 64


class _SSIMPatches(torch.autograd.Function):
    """(mean, per_patch [B]) of fp32 contiguous device patches x, y [B, P, P, C]: one launch pair for the whole batch
    (n2m_ssim_patches_forward), a workgroup per patch (or band of a patch).  The derivative maps [B, 3, P - 10, P - 10, C] are written and
    saved only when x needs a gradient; the backward is one gather launch (n2m_ssim_patches_backward).  Only the mean is differentiable."""

    @staticmethod
    def forward(ctx, x, y):
        B, P, _, C = x.shape
        dev = x.device
        need = ctx.needs_input_grad[0]
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        dS = f(B, 3, P - WINDOW + 1, P - WINDOW + 1, C) if need else None
        partials, per_patch, out = f(L.lib().n2m_ssim_patches_partials(B, P)), f(B), f(1)
        with torch.cuda.device(dev):
            L.call("n2m_ssim_patches_forward", L.ptr(x), L.ptr(y), B, P, C, _TAPS, L.ptr(dS), L.ptr(partials), L.ptr(per_patch), L.ptr(out),
                   L.stream())
        if need:
            ctx.save_for_backward(x, y, dS)
        ctx.mark_non_differentiable(per_patch)
        return out.view(()), per_patch

    @staticmethod
    def backward(ctx, g, _gpp):
        x, y, dS = ctx.saved_tensors
        B, P, _, C = x.shape
        g = g.detach().to(torch.float32).reshape(1).contiguous()
        grad = torch.empty_like(x)
        with torch.cuda.device(x.device):
            L.call("n2m_ssim_patches_backward", L.ptr(x), L.ptr(y), L.ptr(dS), B, P, C, _TAPS, L.ptr(g), L.ptr(grad), L.stream())
        return grad, None


def ssim_patches(pred, target, return_per_patch=False):
    """Mean SSIM over a batch of square patches, every patch on its own (a window never holds a pixel of another patch): the mean of S
    over all B (P - 10)^2 C windows as a 0-dim fp32 device tensor, differentiable in pred, not in target; with return_per_patch also the
    [B] per-patch means (not differentiable).  pred, target: [B, P, P, C], C 1 or 3, 11 <= P <= 64, B >= 1 -- the layout of a patch batch
    (capture.batch_from_uniforms_u8(patch_size=P)) viewed as [B, P, P, 3].  Shapes the kernel refuses raise ValueError, CPU tensors
    RuntimeError (there is no host path)."""
    if pred.dim() != 4 or pred.shape != target.shape or pred.shape[1] != pred.shape[2]:
        raise ValueError(f"ssim_patches: patches must be two [B, P, P, C] tensors of one shape, got {tuple(pred.shape)} and {tuple(target.shape)}")
    B, P, _, C = pred.shape
    if P < PATCH_MIN or P > PATCH_MAX:
        raise ValueError(f"ssim_patches: P must be {PATCH_MIN} .. {PATCH_MAX}, got {P}")
    if C not in (1, 3):
        raise ValueError(f"ssim_patches: C must be 1 or 3, got {C}")
    if B < 1:
        raise ValueError("ssim_patches: B must be at least 1")
    if not (pred.is_cuda and target.is_cuda):
        raise RuntimeError("ssim_patches: pred and target must be CUDA tensors (there is no host path)")
    mean, per_patch = _SSIMPatches.apply(pred.float().contiguous(), target.detach().float().contiguous())
    return (mean, per_patch) if return_per_patch else mean


# ------------------------------------------------------------------------------------------------ held-out evaluation
def ground_truth(capture, v, bg=1.0):
    """View v of the capture as the renderers are judged against it: [H * W, 3], blended on `bg` when the set has alpha."""
    rgba = capture.view(int(v))[2]
    if not capture.has_alpha:
        return rgba[:, :3].contiguous()
    return rgba[:, :3] * rgba[:, 3:] + bg * (1 - rgba[:, 3:])


@torch.no_grad()
def evaluate_views(render, capture, views=None, bg=1.0):
    """PSNR and SSIM of `render(v)["image"]` ([H * W, 3]) against the capture's view v for every v of `views` (default: all, in order):
    {"psnr": [...], "ssim": [...], "mean_psnr", "mean_ssim", "views": [...]}."""
    views = list(range(len(capture))) if views is None else [int(v) for v in views]
    H, W = capture.H, capture.W
    ps, ss = [], []
    for v in views:
        gt = ground_truth(capture, v, bg)
        img = render(v)["image"].detach().float().reshape(H * W, 3)
        ps.append(psnr(img, gt))
        ss.append(float(ssim(img, gt, hw=(H, W))))
    mean = lambda xs: float(np.mean(xs)) if xs else float("nan")
    return {"psnr": ps, "ssim": ss, "mean_psnr": mean(ps), "mean_ssim": mean(ss), "views": views}


def field_renderer(model, capture, bg=1.0):
    """Stage 0: the inference render of the field on the rays of capture.view(v)."""
    opt = model.opt

    def render(v):
        model.eval()
        rays_o, rays_d, _, _ = capture.view(int(v))
        cnf = capture.cam_near_far
        with torch.no_grad():
            return model.render(rays_o, rays_d, bg_color=bg, perturb=False, shading="full", dt_gamma=opt.dt_gamma, max_steps=opt.max_steps,
                                T_thresh=1e-4, cam_near_far=None if cnf is None else cnf[int(v):int(v) + 1])
    return render


def mesh_renderer(model, capture, bg=1.0):
    """Stage 1: render_stage1 of the model's mesh at the capture's cameras (the model's own ssaa)."""
    def render(v):
        model.eval()
        rays_o, rays_d, _, _ = capture.view(int(v))
        with torch.no_grad():
            return model.render_stage1(rays_o, rays_d, capture.mvps[int(v)], capture.H, capture.W, bg_color=bg)
    return render


def asset_renderer(asset, capture, ssaa=1, bg=1.0, filter="nearest"):
    """The shipped asset (asset.ExportedAsset) through the viewer's shader."""
    def render(v):
        rays_d = capture.view(int(v))[1]
        return asset.render(rays_d, capture.mvps[int(v)], capture.H, capture.W, bg_color=bg, filter=filter, ssaa=ssaa)
    return render
