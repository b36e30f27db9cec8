"""Lens models and undistortion of captured sets (capture.Capture.load_colmap(undistort=True)).

COLMAP's camera models as its documentation defines them (https://colmap.github.io/cameras.html; parameter order as in cameras.bin, see
colmap_model.COLMAP_MODELS): normalised image coordinates (x, y) = ((u - cx) / fx, (v - cy) / fy), y DOWN, of the ideal pinhole projection
are mapped forward to the distorted (xd, yd) the sensor recorded; r2 = x^2 + y^2:
  SIMPLE_RADIAL (f, cx, cy, k)                    xd = x (1 + k r2)                                        yd likewise
  RADIAL        (f, cx, cy, k1, k2)               xd = x (1 + k1 r2 + k2 r2^2)
  OPENCV        (fx, fy, cx, cy, k1, k2, p1, p2)  xd = x (1 + k1 r2 + k2 r2^2) + 2 p1 x y + p2 (r2 + 2 x^2)
                                                  yd = y (1 + k1 r2 + k2 r2^2) + 2 p2 x y + p1 (r2 + 2 y^2)
  OPENCV_FISHEYE (fx, fy, cx, cy, k1, k2, k3, k4) theta = atan(r), thetad = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8),
                                                  xd = x thetad / r (x itself at r = 0)
The first three are ONE family here (LENS_BROWN, row = k1, k2, p1, p2 with the unused entries 0; the pinhole models are its all-zero row),
the fisheye polynomial the other (LENS_FISHEYE, row = k1, k2, k3, k4); a row has 8 entries, the last four reserved.  Float64 numpy on
the host (lens_distort, its inverse lens_undistort, the zoom rule); the fp32 statement of the device function of csrc/capture.hip is
lens_distort_f32, operation for operation.
"""
import ctypes

import numpy as np
import torch

LENS_BROWN, LENS_FISHEYE = 1, 2            # N2M_LENS_* of include/n2m_hip.h
LENS_MAX_ITER, LENS_STEP = 100, 1e-12      # the inverse: at most 100 Newton steps, converged when the step is below 1e-12 (normalised units)
ZOOM_MAX, ZOOM_TOL = 4.0, 1e-6


def as_f64(a):
    """A tensor (on any device) or anything numpy takes -> float64 numpy on the host."""
    return a.detach().double().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)


def lens_row(model, params):
    """COLMAP camera `model` (name) with its parameter vector -> ((fx, fy, cx, cy), family, row [8] float64).  FULL_OPENCV, FOV and the
    thin-prism / other fisheye models: ValueError."""
    p = [float(x) for x in params]
    row = np.zeros(8)
    if model in ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL"):
        f4 = (p[0], p[0], p[1], p[2])
        row[:len(p) - 3] = p[3:]
    elif model in ("PINHOLE", "OPENCV", "OPENCV_FISHEYE"):
        f4 = tuple(p[:4])
        row[:len(p) - 4] = p[4:]
    else:
        raise ValueError(f"unsupported COLMAP camera model: {model}")
    return f4, (LENS_FISHEYE if model == "OPENCV_FISHEYE" else LENS_BROWN), row


def lens_distort(family, row, x, y):
    """Forward map, float64: ideal normalised (x, y) -> distorted (xd, yd); arrays of one shape (or numbers), row [8] as lens_row."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    k = [float(a) for a in row]
    r2 = x * x + y * y
    if family == LENS_FISHEYE:
        r = np.sqrt(r2)
        th = np.arctan(r)
        t2 = th * th
        thd = th * (1 + k[0] * t2 + k[1] * t2 ** 2 + k[2] * t2 ** 3 + k[3] * t2 ** 4)
        with np.errstate(divide="ignore", invalid="ignore"):
            scale = np.where(r < 1e-8, 1.0, thd / r)
        return x * scale, y * scale
    if family != LENS_BROWN:
        raise ValueError(f"unknown lens family {family}")
    radial = k[0] * r2 + k[1] * r2 * r2
    return (x + x * radial + 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x),
            y + y * radial + 2 * k[3] * x * y + k[2] * (r2 + 2 * y * y))


def lens_undistort(family, row, xd, yd):
    """Inverse map, float64: distorted normalised (xd, yd) -> ideal (x, y), by Newton's method from (xd, yd) -- on the two coordinates with
    the analytic Jacobian for LENS_BROWN, on theta alone for LENS_FISHEYE (then r = tan theta).  Every point is iterated until the largest
    step of the array, in normalised units, is below LENS_STEP; more than LENS_MAX_ITER steps, or a step that is not finite: ValueError."""
    xd, yd = np.asarray(xd, dtype=np.float64), np.asarray(yd, dtype=np.float64)
    k = [float(a) for a in row]
    if family == LENS_FISHEYE:
        rd = np.sqrt(xd * xd + yd * yd)
        th = rd.copy()
        for _ in range(LENS_MAX_ITER):
            t2 = th * th
            g = th * (1 + k[0] * t2 + k[1] * t2 ** 2 + k[2] * t2 ** 3 + k[3] * t2 ** 4) - rd
            dg = 1 + 3 * k[0] * t2 + 5 * k[1] * t2 ** 2 + 7 * k[2] * t2 ** 3 + 9 * k[3] * t2 ** 4
            with np.errstate(all="ignore"):
                step = g / dg
                th = th - step
                size = np.abs(step) * (1 + np.tan(th) ** 2)            # the step of r = tan theta
            if not np.isfinite(size).all() or (np.abs(th) >= np.pi / 2).any():
                break
            if size.max(initial=0.0) < LENS_STEP:
                with np.errstate(divide="ignore", invalid="ignore"):
                    scale = np.where(rd < 1e-8, 1.0, np.tan(th) / rd)
                return xd * scale, yd * scale
        raise ValueError("lens_undistort: the fisheye inverse did not converge (a point beyond the model's field of view?)")
    if family != LENS_BROWN:
        raise ValueError(f"unknown lens family {family}")
    k1, k2, p1, p2 = k[:4]
    x, y = xd.copy(), yd.copy()
    for _ in range(LENS_MAX_ITER):
        xx, yy, xy = x * x, y * y, x * y
        r2 = xx + yy
        radial, dr = k1 * r2 + k2 * r2 * r2, k1 + 2 * k2 * r2            # radial and d radial / d r2
        fx_ = x + x * radial + 2 * p1 * xy + p2 * (r2 + 2 * xx) - xd
        fy_ = y + y * radial + 2 * p2 * xy + p1 * (r2 + 2 * yy) - yd
        a = 1 + radial + 2 * xx * dr + 2 * p1 * y + 6 * p2 * x
        b = 2 * xy * dr + 2 * p1 * x + 2 * p2 * y
        d = 1 + radial + 2 * yy * dr + 2 * p2 * x + 6 * p1 * y
        det = a * d - b * b
        with np.errstate(all="ignore"):
            sx, sy = (d * fx_ - b * fy_) / det, (a * fy_ - b * fx_) / det
        size = np.maximum(np.abs(sx), np.abs(sy))
        if not np.isfinite(size).all():
            break
        x, y = x - sx, y - sy
        if size.max(initial=0.0) < LENS_STEP:
            return x, y
    raise ValueError("lens_undistort: Newton's method did not converge (a point outside the range where the lens model is invertible?)")


def _border_pixels(H, W):
    """(rows, cols) of the 2 (H + W) - 4 border pixels of an H x W image (all of them for H or W below 3)."""
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    m = (jj == 0) | (jj == H - 1) | (ii == 0) | (ii == W - 1)
    return jj[m], ii[m]


def border_taps_inside(H, W, intrinsics, family, row, zoom):
    """True when, for the output camera (zoom fx, zoom fy, cx, cy), the bilinear sample point of every border pixel centre lies inside the
    hull of the source pixel centres, 0 <= sx <= W - 1 and 0 <= sy <= H - 1 -- then all four taps of every output pixel that carry weight
    are source pixels.  Float64."""
    fx, fy, cx, cy = (float(a) for a in intrinsics)
    jj, ii = _border_pixels(H, W)
    xd, yd = lens_distort(family, row, (ii + 0.5 - cx) / (zoom * fx), (jj + 0.5 - cy) / (zoom * fy))
    sx, sy = fx * xd + cx - 0.5, fy * yd + cy - 0.5
    return bool(((sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)).all())


def undistort_zoom(H, W, intrinsics, family, row, name="camera"):
    """The zoom s >= 1 of the output camera of an undistorted set (size, cx, cy kept; fx, fy multiplied by s): the smallest for which
    border_taps_inside holds, so no output pixel is blank.  1 when all coefficients are 0 or when it holds at 1 (barrel distortion);
    otherwise bisection on [1, ZOOM_MAX] until the bracket is below ZOOM_TOL, and its upper (holding) end is returned; ValueError naming
    the camera when it does not hold at ZOOM_MAX."""
    if not np.any(np.asarray(row, dtype=np.float64)) or border_taps_inside(H, W, intrinsics, family, row, 1.0):
        return 1.0
    if not border_taps_inside(H, W, intrinsics, family, row, ZOOM_MAX):
        raise ValueError(f"{name}: the lens distortion leaves blank pixels even at a zoom of {ZOOM_MAX:g}; the set cannot be undistorted at its own size")
    lo, hi = 1.0, ZOOM_MAX
    while hi - lo > ZOOM_TOL:
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if border_taps_inside(H, W, intrinsics, family, row, mid) else (mid, hi)
    return hi


def _f32(x):
    return torch.tensor(float(x), dtype=torch.float32)


def _atan_f32(r):
    """lens_atan of csrc/capture.hip, r >= 0 fp32: reduction by 1 / r and (t - 1) / (t + 1), Taylor series to z^17 by Horner, every step one
    fp32 rounding."""
    inv = r > 1
    t = torch.where(inv, torch.ones_like(r) / r, r)
    red = t > _f32(0.41421356237309503)
    z = torch.where(red, (t - 1) / (t + 1), t)
    z2 = z * z
    p = _f32(1 / 17).expand_as(z)
    for n, sign in ((15, -1), (13, 1), (11, -1), (9, 1), (7, -1), (5, 1), (3, -1)):
        p = p * z2 + _f32(1 / n) if sign > 0 else p * z2 - _f32(1 / n)
    p = p * z2 + 1
    a = p * z
    a = torch.where(red, a + _f32(0.78539816339744831), a)
    return torch.where(inv, _f32(1.5707963267948966) - a, a)


def lens_distort_f32(family, k, x, y):
    """The device function lens_distort of csrc/capture.hip as a torch statement: fp32 CPU tensors x, y; k [...,8] fp32, broadcast against
    them along its leading dimensions.  Each operation below is one fp32 rounding in the kernel's order."""
    k0, k1, k2, k3 = k[..., 0], k[..., 1], k[..., 2], k[..., 3]
    xx, yy = x * x, y * y
    r2 = xx + yy
    if family == LENS_FISHEYE:
        r = r2.double().sqrt().float()                  # the correctly rounded fp32 root (see Capture.view)
        th = _atan_f32(r)
        t2 = th * th
        t4 = t2 * t2
        t6, t8 = t4 * t2, t4 * t4
        thd = th * (1 + (((k0 * t2 + k1 * t4) + k2 * t6) + k3 * t8))
        scale = torch.where(r < _f32(1e-8), _f32(1.0), thd / r)
        return x * scale, y * scale
    r4, xy = r2 * r2, x * y
    radial = k0 * r2 + k1 * r4
    a, b = k2 * xy, k3 * xy
    return (x + ((x * radial + (a + a)) + k3 * (r2 + (xx + xx))),
            y + ((y * radial + (b + b)) + k2 * (r2 + (yy + yy))))


def undistort_source_f32(rows, cols, src_k, out_k, lens, family):
    """(u, v) fp32: where in the source image (continuous coordinates, pixel c covers [c, c + 1)) the centre of output pixel (rows, cols)
    comes from -- the first half of the undistort kernel.  rows, cols int tensors [..., P]; src_k, out_k [..., 1, 4] and lens [..., 1, 8]
    fp32 (or plain [4] / [8] rows)."""
    i, j = cols.float() + 0.5, rows.float() + 0.5
    x, y = (i - out_k[..., 2]) / out_k[..., 0], (j - out_k[..., 3]) / out_k[..., 1]
    xd, yd = lens_distort_f32(family, lens, x, y)
    return src_k[..., 0] * xd + src_k[..., 2], src_k[..., 1] * yd + src_k[..., 3]


def _lens_tables(V, src_intrinsics, out_intrinsics, lens):
    """The three parameter sets as fp32 CPU tensors [R,4], [R,4], [R,8] with R = V when any of them has a row per view, else 1."""
    t = [torch.as_tensor(as_f64(a)).to(torch.float32) for a in (src_intrinsics, out_intrinsics, lens)]
    for a, n, what in zip(t, (4, 4, 8), ("src_intrinsics", "out_intrinsics", "lens")):
        if tuple(a.shape) not in ((n,), (V, n)):
            raise ValueError(f"{what} must be [{n}] or [{V},{n}], not {tuple(a.shape)}")
    per_view = any(a.dim() == 2 for a in t)
    R = V if per_view else 1
    return [(a if a.dim() == 2 else a.unsqueeze(0).expand(R, -1)).contiguous() for a in t], per_view


def _undistort(src, H, W, src_intrinsics, out_intrinsics, lens, family, depth, out=None):
    V = src.shape[0]
    want = torch.float32 if depth else torch.int32
    if src.dim() != 2 or src.shape[1] != H * W or src.dtype != want:
        raise ValueError(f"the source must be {'fp32' if depth else 'int32 (pack_rgba8)'} [V, H*W] = [V, {H * W}]")
    if family not in (LENS_BROWN, LENS_FISHEYE):
        raise ValueError(f"unknown lens family {family}")
    (S, O, K), per_view = _lens_tables(V, src_intrinsics, out_intrinsics, lens)
    if src.is_cuda:
        from . import _lib as L
        src = src.contiguous()
        if out is None:
            out = torch.empty_like(src)
        S, O, K = S.to(src.device), O.to(src.device), K.to(src.device)
        desc = L.Undistort(src=L.ptr(src), dst=L.ptr(out), V=V, H=int(H), W=int(W), model=int(family), depth=int(bool(depth)), per_view=int(per_view),
                           src_intrinsics=L.ptr(S), out_intrinsics=L.ptr(O), lens=L.ptr(K))
        L.call("n2m_capture_undistort", ctypes.addressof(desc), L.stream())
        return out
    jj, ii = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    u, v = undistort_source_f32(jj.reshape(-1), ii.reshape(-1), S.unsqueeze(1), O.unsqueeze(1), K.unsqueeze(1), family)
    u, v = u.expand(V, H * W), v.expand(V, H * W)
    vv = torch.arange(V).unsqueeze(1)
    if depth:
        ix, iy = u.floor().clamp(0, W - 1).long(), v.floor().clamp(0, H - 1).long()
        val = src[vv, iy * W + ix]
    else:
        sx, sy = u - 0.5, v - 0.5
        fx0, fy0 = sx.floor(), sy.floor()
        tx, ty = (sx - fx0).unsqueeze(-1), (sy - fy0).unsqueeze(-1)
        ix, iy = fx0.clamp(-1, W).long(), fy0.clamp(-1, H).long()
        x0, x1, y0, y1 = ix.clamp(min=0, max=W - 1), (ix + 1).clamp(max=W - 1), iy.clamp(min=0, max=H - 1), (iy + 1).clamp(max=H - 1)
        by = src.contiguous().view(torch.uint8).view(V, H * W, 4)
        a, b, c, e = (by[vv, y * W + x].float() for y, x in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
        top, bot = a + (b - a) * tx, c + (e - c) * tx
        q = ((top + (bot - top) * ty) + 0.5).floor().clamp(0, 255).to(torch.uint8)
        val = q.contiguous().view(V, H * W * 4).view(torch.int32).view(V, H * W)
    return val if out is None else out.copy_(val)


def undistort_bank(bank, H, W, src_intrinsics, out_intrinsics, lens, family, out=None):
    """Packed words [V,H*W] of photographs taken through a lens -> the same views through the pinhole camera `out_intrinsics`, out of place:
    per output pixel centre the forward lens model (family, lens row) and the source camera give the sample point, four-tap bilinear per
    8-bit channel, floor(val + 0.5) clamped to [0, 255].  src_intrinsics / out_intrinsics (fx, fy, cx, cy) and lens [8] are single rows,
    or [V,4] / [V,8] with a row per view (any of them a table: all are taken per view).  On the GPU one kernel (n2m_capture_undistort);
    below it the torch statement of the same fp32 arithmetic, taken on the CPU: bit for bit."""
    return _undistort(bank, H, W, src_intrinsics, out_intrinsics, lens, family, False, out)


def undistort_depth(planes, H, W, src_intrinsics, out_intrinsics, lens, family, out=None):
    """fp32 planes [V,H*W] (rows of a dense-depth bank) through the same map, taking the NEAREST source texel -- the one that contains the
    sample point -- so that no output depth mixes two surfaces: every output value is a value of its source plane.  The zoom changes no
    value: a depth is measured along the ray, and the pose is unchanged.  The depth mode of n2m_capture_undistort / its torch statement."""
    return _undistort(planes, H, W, src_intrinsics, out_intrinsics, lens, family, True, out)
