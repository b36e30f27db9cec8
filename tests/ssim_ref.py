"""Reference model of the device SSIM (nerf2mesh_amd/metrics.py, csrc/metrics.hip), in torch on the CPU.

The definition (Wang et al. 2004): an 11 x 11 Gaussian window, sigma 1.5, VALID windows only (no padding: the map of an [H, W, C] pair is
[H - 10, W - 10, C]), C1 = 0.01^2, C2 = 0.03^2 (data range 1); per window and channel

    S = (2 mu_x mu_y + C1) (2 s_xy + C2) / ((mu_x^2 + mu_y^2 + C1) (s_x^2 + s_y^2 + C2))

with mu the Gaussian-weighted mean, s_x^2 = E[x^2] - mu_x^2, s_xy = E[xy] - mu_x mu_y; ssim = mean of S over windows and channels.

`ssim_model(x, y)` is the float64 model: conv2d with the 121-entry outer product of the float64 taps; its gradient is float64 autograd
(`ssim_model_grad`).  `dtype=torch.float32` is the same model with everything cast to fp32 (taps, window, images, every intermediate):
an independent restatement in the kernel's own precision -- the yardstick the GPU tests derive their tolerance from.
`ssim_loops` is the definition as a literal double loop over windows (test_ssim_ref_cpu.py holds the model to it).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

WIN, SIGMA = 11, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def taps64():
    """The 11 taps: exp(-d^2 / (2 sigma^2)) in float64, normalised to sum 1."""
    d = np.arange(WIN, dtype=np.float64) - (WIN - 1) / 2
    g = np.exp(-(d * d) / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def ssim_model(x, y, dtype=torch.float64):
    """x, y [H, W, C] -> (mean, map [H - 10, W - 10, C]) in `dtype`; differentiable in x."""
    x, y = x.to(dtype), y.to(dtype)
    H, W, C = x.shape
    t = torch.from_numpy(taps64()).to(dtype)            # float64 taps, rounded once when dtype is fp32 (what the kernel is handed)
    w2 = torch.outer(t, t).view(1, 1, WIN, WIN)

    def blur(img):                                       # [H, W, C] -> [C, 1, H, W] -> valid conv -> [H - 10, W - 10, C]
        return F.conv2d(img.permute(2, 0, 1).unsqueeze(1), w2).squeeze(1).permute(1, 2, 0)

    mx, my = blur(x), blur(y)
    sxx = blur(x * x) - mx * mx
    syy = blur(y * y) - my * my
    sxy = blur(x * y) - mx * my
    smap = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    return smap.mean(), smap


def ssim_model_grad(x, y, g=1.0, dtype=torch.float64):
    """d (g * mean) / dx by autograd in `dtype`: [H, W, C]."""
    xr = x.detach().to(dtype).clone().requires_grad_(True)
    mean, _ = ssim_model(xr, y.detach(), dtype)
    (gx,) = torch.autograd.grad(mean * torch.tensor(g, dtype=dtype), xr)
    return gx.contiguous()


def ssim_loops(x, y):
    """The definition, window by window, in Python floats (float64): (mean, map as a nested list [H - 10][W - 10][C])."""
    H, W, C = x.shape
    t = taps64()
    xs, ys = x.double().numpy(), y.double().numpy()
    out = np.zeros((H - WIN + 1, W - WIN + 1, C))
    for j in range(H - WIN + 1):
        for i in range(W - WIN + 1):
            for c in range(C):
                mx = my = exx = eyy = exy = 0.0
                for dj in range(WIN):
                    for di in range(WIN):
                        w = t[dj] * t[di]
                        a, b = float(xs[j + dj, i + di, c]), float(ys[j + dj, i + di, c])
                        mx += w * a
                        my += w * b
                        exx += w * a * a
                        eyy += w * b * b
                        exy += w * a * b
                sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
                out[j, i, c] = (2 * mx * my + C1) * (2 * sxy + C2) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    return float(out.mean()), out


# ------------------------------------------------------------------------------------------------ the GPU tests' case set
SHAPES = [(11, 11), (11, 43), (43, 11), (42, 75), (76, 43)]     # one window; one row / one column of windows; map extents 32 x 65 and 66 x 33
CHANNELS = [1, 3]
INPUTS = ["random", "same", "inverse", "const_vs_noise", "const_const"]


def make_pair(shape, C, kind, seed=0):
    """Seeded input pair (x, y) fp32 [H, W, C] in [0, 1]."""
    H, W = shape
    gen = torch.Generator().manual_seed(1000 * seed + 97 * H + 13 * W + C)
    x = torch.rand(H, W, C, generator=gen)
    n = torch.rand(H, W, C, generator=gen)
    if kind == "random":
        return x, n
    if kind == "same":
        return x, x.clone()
    if kind == "inverse":
        return x, 1 - x
    if kind == "const_vs_noise":
        return torch.full((H, W, C), 0.25), n
    if kind == "const_const":
        return torch.full((H, W, C), 0.3), torch.full((H, W, C), 0.7)
    raise ValueError(kind)


def forward_error(mean, smap, ref_mean, ref_map):
    """(|mean - ref|, max |map - ref|) as Python floats; everything compared in float64."""
    return (abs(float(mean) - float(ref_mean)), float((smap.double() - ref_map.double()).abs().max()))


def grad_error(grad, ref_grad, norm):
    """max |grad - ref| / norm: the error per image, normalised by the image's max |ref grad| (`grad_norm`)."""
    return float((grad.double() - ref_grad.double()).abs().max()) / norm


_CASES = {}


def case(shape, C, kind):
    """One case, computed once and shared: inputs, the float64 forward and gradient (g = 1), the normaliser, and the yardstick's own errors
    (fp32 model against float64 model, same error measures)."""
    key = (tuple(shape), C, kind)
    if key not in _CASES:
        x, y = make_pair(shape, C, kind)
        mean, smap = ssim_model(x, y)
        grad = ssim_model_grad(x, y)
        _CASES[key] = dict(x=x, y=y, mean=mean.detach(), map=smap.detach(), grad=grad)
        c = _CASES[key]
        # y = x is the maximum of S: the true gradient is identically zero and max |ref grad| is rounding noise.  That case is normalised
        # by the gradient scale of the SAME x against noise (the "random" case of the same shape and channel count).
        c["grad_norm"] = case(shape, C, "random")["grad_norm"] if kind == "same" else float(grad.abs().max())
        m32, s32 = ssim_model(x, y, torch.float32)
        g32 = ssim_model_grad(x, y, dtype=torch.float32)
        c["yard_mean"], c["yard_map"] = forward_error(m32.detach(), s32.detach(), c["mean"], c["map"])
        c["yard_grad"] = grad_error(g32, grad, c["grad_norm"])
    return _CASES[key]


def yardstick():
    """The largest yardstick error over the whole case set, per measure: {"mean", "map", "grad"}."""
    cs = [case(s, C, k) for s in SHAPES for C in CHANNELS for k in INPUTS]
    return {"mean": max(c["yard_mean"] for c in cs), "map": max(c["yard_map"] for c in cs), "grad": max(c["yard_grad"] for c in cs)}
