"""Shared by tests/test_undistort_cpu.py, tests/test_undistort_kernels_gpu.py and tests/test_undistort_engine_gpu.py: a float64 numpy model of
the lens models, the zoom rule and the resampler of DESIGN 4.26 (capture.undistort_bank / n2m_capture_undistort), written as plain loops over
pixels from COLMAP's published definitions -- independent of the vectorised code in nerf2mesh_amd/capture.py -- and the case list both test
files walk."""
import math

import numpy as np

# (name, COLMAP model, distortion coefficients in the model's own order, (fx, fy, cx, cy) at 24 rows x 33 columns)
H, W = 24, 33
CENTRED = (30.0, 30.0, W / 2, H / 2)
CASES = [
    ("pincushion", "SIMPLE_RADIAL", (0.1,), CENTRED),
    ("barrel", "SIMPLE_RADIAL", (-0.1,), CENTRED),
    ("radial2", "RADIAL", (0.12, -0.03), CENTRED),
    ("opencv", "OPENCV", (0.1, -0.02, 0.003, -0.002), CENTRED),
    ("fisheye", "OPENCV_FISHEYE", (0.05, 0.01, 0.0, 0.0), CENTRED),
    ("offcentre", "SIMPLE_RADIAL", (0.1,), (30.0, 30.0, W / 2 + 1.5, H / 2 - 1.5)),
    ("fx_ne_fy", "OPENCV", (0.1, -0.02, 0.003, -0.002), (31.0, 28.5, W / 2, H / 2)),
]


def colmap_params(model, intr, coeff):
    """The parameter vector cameras.bin holds for `model`."""
    fx, fy, cx, cy = intr
    if model in ("SIMPLE_RADIAL", "RADIAL"):
        assert fx == fy
        return (fx, cx, cy) + tuple(coeff)
    return (fx, fy, cx, cy) + tuple(coeff)


def distort(model, c, x, y):
    """COLMAP's forward model for one point, float64 scalars."""
    r2 = x * x + y * y
    if model == "SIMPLE_RADIAL":
        return x * (1 + c[0] * r2), y * (1 + c[0] * r2)
    if model == "RADIAL":
        f = 1 + c[0] * r2 + c[1] * r2 * r2
        return x * f, y * f
    if model == "OPENCV":
        k1, k2, p1, p2 = c
        f = 1 + k1 * r2 + k2 * r2 * r2
        return (x * f + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * f + 2 * p2 * x * y + p1 * (r2 + 2 * y * y))
    if model == "OPENCV_FISHEYE":
        r = math.sqrt(r2)
        if r < 1e-8:
            return x, y
        t = math.atan(r)
        td = t * (1 + c[0] * t ** 2 + c[1] * t ** 4 + c[2] * t ** 6 + c[3] * t ** 8)
        return x * td / r, y * td / r
    raise ValueError(model)


def sample_point(model, c, src, out, row, col):
    """(sx, sy): where in the source image (pixel-centre grid: sx = 0 is the centre of column 0) output pixel (row, col) samples."""
    x, y = (col + 0.5 - out[2]) / out[0], (row + 0.5 - out[3]) / out[1]
    xd, yd = distort(model, c, x, y)
    return src[0] * xd + src[2] - 0.5, src[1] * yd + src[3] - 0.5


def border(Hh, Ww):
    return [(j, i) for j in range(Hh) for i in range(Ww) if j in (0, Hh - 1) or i in (0, Ww - 1)]


def taps_inside(model, c, intr, Hh, Ww, s):
    out = (s * intr[0], s * intr[1], intr[2], intr[3])
    for j, i in border(Hh, Ww):
        sx, sy = sample_point(model, c, intr, out, j, i)
        if not (0 <= sx <= Ww - 1 and 0 <= sy <= Hh - 1):
            return False
    return True


def undistort_images(images, model, c, src, out):
    """images uint8 [V,H,W,C] -> (uint8 [V,H,W,C] rounded, float64 [V,H,W,C] before rounding): four-tap bilinear, taps clamped."""
    V, Hh, Ww, C = images.shape
    val = np.zeros((V, Hh, Ww, C))
    src_v = [src] * V if np.ndim(src) == 1 else src
    out_v = [out] * V if np.ndim(out) == 1 else out
    c_v = [c] * V if np.ndim(c) == 1 else c
    for v in range(V):
        im = images[v].astype(np.float64)
        for j in range(Hh):
            for i in range(Ww):
                sx, sy = sample_point(model, c_v[v], src_v[v], out_v[v], j, i)
                x0, y0 = math.floor(sx), math.floor(sy)
                tx, ty = sx - x0, sy - y0
                xa, xb = min(max(x0, 0), Ww - 1), min(max(x0 + 1, 0), Ww - 1)
                ya, yb = min(max(y0, 0), Hh - 1), min(max(y0 + 1, 0), Hh - 1)
                top = im[ya, xa] + (im[ya, xb] - im[ya, xa]) * tx
                bot = im[yb, xa] + (im[yb, xb] - im[yb, xa]) * tx
                val[v, j, i] = top + (bot - top) * ty
    return np.clip(np.floor(val + 0.5), 0, 255).astype(np.uint8), val


def undistort_depth(plane, model, c, src, out):
    """plane [H,W] -> [H,W]: the source texel that contains the sample point."""
    Hh, Ww = plane.shape
    res = np.zeros_like(plane)
    for j in range(Hh):
        for i in range(Ww):
            sx, sy = sample_point(model, c, src, out, j, i)
            res[j, i] = plane[min(max(math.floor(sy + 0.5), 0), Hh - 1), min(max(math.floor(sx + 0.5), 0), Ww - 1)]
    return res


def pattern(x, y, freq=1.0):
    """A smooth target in normalised coordinates, in [0, 255]: two low-frequency sinusoids."""
    return 127.5 + 63.0 * np.sin(freq * (5.0 * x + 1.0)) + 63.0 * np.sin(freq * (4.0 * y - 3.0 * x + 0.5))


def noise_images(V, Hh, Ww, C=4, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (V, Hh, Ww, C), dtype=np.uint8)


FREQS = (1.0, 1.3, 0.7, 1.9)               # one pattern per channel


def target(intr, Hh, Ww, freq_scale=1.0):
    """float64 [H,W,4]: the pattern seen by the pinhole camera `intr`, at the pixel centres."""
    jj, ii = np.meshgrid(np.arange(Hh) + 0.5, np.arange(Ww) + 0.5, indexing="ij")
    x, y = (ii - intr[2]) / intr[0], (jj - intr[3]) / intr[1]
    return np.stack([pattern(x, y, f * freq_scale) for f in FREQS], -1)


def photograph(inverse, intr, Hh, Ww, freq_scale=1.0):
    """uint8 [H,W,4]: the pattern photographed through the lens -- evaluated at the IDEAL coordinates of every distorted-image pixel centre,
    which `inverse(xd, yd) -> (x, y)` (the float64 host inverse under test elsewhere) supplies."""
    jj, ii = np.meshgrid(np.arange(Hh) + 0.5, np.arange(Ww) + 0.5, indexing="ij")
    x, y = inverse((ii - intr[2]) / intr[0], (jj - intr[3]) / intr[1])
    return np.clip(np.floor(np.stack([pattern(x, y, f * freq_scale) for f in FREQS], -1) + 0.5), 0, 255).astype(np.uint8)
