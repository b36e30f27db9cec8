"""The exported asset's fragment shader in float64 numpy, written from its description (not from the kernel): per covered pixel of a
rasterised view

    face = rast[..., 3] - 1, cascade = the last one whose face_begin is <= face
    uv   = b0 vt[ft[face, 0]] + b1 vt[ft[face, 1]] + (1 - b0 - b1) vt[ft[face, 2]]
    nearest: texel (row clamp(floor(v Ht)), column clamp(floor(u Wt)));  linear: the four texels around (u Wt - .5, v Ht - .5), indices
             clamped at the border;  texel / 255
    d    = rays_d / sqrt(max(|rays_d|^2, 1e-20))
    spec = sigmoid(w1 relu(w0 [d, feat1 texel]))            (no bias; the direction comes first)
    full = clamp(feat0 texel + spec, 0, 1), diffuse = feat0 texel, specular = spec;  empty pixels are 0.
"""
import numpy as np


def sample(tex, u, v, filter):
    """tex [Ht,Wt,3] uint8, u / v [N] float64 -> ([N,3] float64 in [0,1], u Wt, v Ht)."""
    Ht, Wt = tex.shape[0], tex.shape[1]
    t = tex.astype(np.float64)
    x, y = u * Wt, v * Ht
    if filter == "nearest":
        col = np.clip(np.floor(x), 0, Wt - 1).astype(np.int64)
        row = np.clip(np.floor(y), 0, Ht - 1).astype(np.int64)
        out = t[row, col]
    elif filter == "linear":
        xs, ys = x - 0.5, y - 0.5
        x0, y0 = np.floor(xs), np.floor(ys)
        fx, fy = (xs - x0)[:, None], (ys - y0)[:, None]
        c0, c1 = np.clip(x0, 0, Wt - 1).astype(np.int64), np.clip(x0 + 1, 0, Wt - 1).astype(np.int64)
        r0, r1 = np.clip(y0, 0, Ht - 1).astype(np.int64), np.clip(y0 + 1, 0, Ht - 1).astype(np.int64)
        out = (1 - fx) * (1 - fy) * t[r0, c0] + fx * (1 - fy) * t[r0, c1] + (1 - fx) * fy * t[r1, c0] + fx * fy * t[r1, c1]
    else:
        raise ValueError(filter)
    return out / 255.0, x, y


def shade(rast, ft, vt, rays_d, feat0, feat1, face_begin, w0, w1, mode="full", filter="nearest"):
    """rast [H,W,4], ft [F,3] int, vt [T,2], rays_d [H W,3], feat0 / feat1: lists of uint8 [Ht,Wt,3], face_begin: list, w0 [32,6], w1 [3,32].
    Returns {"rgb" [H W,3] float64, "covered" [H W] bool, "cascade" [H W] int (-1 where empty), "x" / "y" [H W] float64: the texel-space
    coordinates u Wt and v Ht of the pixel's cascade (nan where empty)}."""
    rast = np.asarray(rast, np.float64).reshape(-1, 4)
    vt, rays_d = np.asarray(vt, np.float64), np.asarray(rays_d, np.float64).reshape(-1, 3)
    w0, w1 = np.asarray(w0, np.float64), np.asarray(w1, np.float64)
    ft = np.asarray(ft, np.int64)
    N = rast.shape[0]
    face = np.rint(rast[:, 3]).astype(np.int64) - 1
    covered = face >= 0
    cascade = np.full(N, -1, np.int64)
    for c, begin in enumerate(face_begin):
        cascade[covered & (face >= begin)] = c
    b0, b1 = rast[:, 0:1], rast[:, 1:2]
    fi = np.where(covered, face, 0)
    uv = b0 * vt[ft[fi, 0]] + b1 * vt[ft[fi, 1]] + (1 - b0 - b1) * vt[ft[fi, 2]]
    dif, sf = np.zeros((N, 3)), np.zeros((N, 3))
    x, y = np.full(N, np.nan), np.full(N, np.nan)
    for c in range(len(face_begin)):
        sel = cascade == c
        if sel.any():
            dif[sel], x[sel], y[sel] = sample(feat0[c], uv[sel, 0], uv[sel, 1], filter)
            sf[sel] = sample(feat1[c], uv[sel, 0], uv[sel, 1], filter)[0]
    d = rays_d / np.sqrt(np.maximum((rays_d * rays_d).sum(-1, keepdims=True), 1e-20))
    hidden = np.maximum(np.concatenate([d, sf], axis=1) @ w0.T, 0)
    spec = 1.0 / (1.0 + np.exp(-(hidden @ w1.T)))
    rgb = {"full": np.clip(dif + spec, 0, 1), "diffuse": dif, "specular": spec}[mode]
    return {"rgb": np.where(covered[:, None], rgb, 0.0), "covered": covered, "cascade": cascade, "x": x, "y": y}


def near_texel_boundary(x, y, tol=1e-4):
    """True where the texel-space coordinate lies within `tol` of an integer on either axis: there a float32 evaluation may
    legitimately land in the neighbouring texel."""
    return (np.abs(x - np.rint(x)) <= tol) | (np.abs(y - np.rint(y)) <= tol)
