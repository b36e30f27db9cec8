"""Float64 restatement of the stage-1 raster operators (include/n2m_raster.h), torch on the CPU -- TEST INFRASTRUCTURE ONLY.

Written from the header's semantics, not from the kernels, so that a formula mistake in raster.hip (or in the float32 C oracle, which
shares its author) shows up as a disagreement here:

  rasterize_truth   coverage of every pixel by brute force over faces x pixels (un-snapped perspective-correct barycentrics from
                    homogeneous edge functions; nearest z/w wins, ties -> lower id), with a per-pixel decision margin: the pixels where
                    the device's 1/256-px snapped, float32 decision may legitimately differ.
  uvz / interpolate / antialias
                    per-pixel (per pixel-pair) functions of the gathered corner values for an id image held fixed.  Autograd gives each
                    pixel's contribution c to every vertex; scatter-adding c gives the float64 gradient, and the same formulas run in
                    float32 give the per-element conditioning of the tolerance rule below.

Tolerance rule (one rule for every comparison in tests/test_raster_f64.py):

    |got - ref64| <= 4 * scatter(|c32 - c64|) + n_v * 2^-24 * scatter(|c64|) + 2^-30

  c64 / c32  the contributions of one term (a pixel, a pixel pair, an attribute channel) evaluated in float64 / float32.  |c32 - c64| is
             measured on the exact inputs and on JITTER_RUNS sets of inputs moved by one float32 ulp each, and the largest is kept: the
             rounding error of the float32 formula at that element, whatever order the kernel evaluates it in.
  n_v        the number of terms summed into that element: n_v * 2^-24 * sum |c| bounds the rounding of any summation order (the atomics).
             A per-pixel quantity has n_v = 1.
"""
import numpy as np
import torch

F64, F32 = torch.float64, torch.float32
U32 = 2.0 ** -24                     # unit roundoff of float32
JITTER_RUNS = 3
SNAP_PX = 1.0 / 256                  # the 1/256-px vertex snap (rounding to nearest) moves a vertex by <= sqrt(2) / 512 = 0.0028 px


# ------------------------------------------------------------------------------------------------ tolerance rule

class Scatter:
    """Terms c[m, :] summed into out[index[m], :] (out has n rows): the float64 sum and its tolerance."""

    def __init__(self, n, k):
        self.n, self.k = n, k
        self.ref = torch.zeros(n, k, dtype=F64)
        self.abs = torch.zeros(n, k, dtype=F64)
        self.cond = torch.zeros(n, k, dtype=F64)
        self.cnt = torch.zeros(n, k, dtype=F64)

    def add(self, index, c64, c32):
        index = torch.as_tensor(index, dtype=torch.long).reshape(-1)
        c64 = c64.detach().to(F64).reshape(len(index), self.k)
        dc = (c32.detach().to(F64).reshape(len(index), self.k) - c64).abs()
        self.ref.index_add_(0, index, c64)
        self.abs.index_add_(0, index, c64.abs())
        self.cond.index_add_(0, index, dc)
        self.cnt.index_add_(0, index, torch.ones_like(c64))
        return self

    def add_exact(self, index, c):
        """Terms the kernel reads exactly (an input copied through): no conditioning, but one term of the sum."""
        c = torch.as_tensor(c, dtype=F64).reshape(-1, self.k)
        return self.add(index, c, c)

    @property
    def tol(self):
        return 4.0 * self.cond + self.cnt * U32 * self.abs + 2.0 ** -30


def check(got, sc, what, mask=None):
    """assert |got - ref| <= tol elementwise (rows selected by `mask` if given); the message names the worst element."""
    got = torch.as_tensor(np.asarray(got)).to(F64).reshape(sc.n, sc.k)
    err, tol = (got - sc.ref).abs(), sc.tol
    if mask is not None:
        m = torch.as_tensor(np.asarray(mask)).reshape(-1).bool()
        err, tol = err[m], tol[m]
    bad = ~(err <= tol)
    if bool(bad.any()):
        r = (err / tol).nan_to_num(posinf=1e30)
        i = int(r.argmax())
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.numel()} elements outside the tolerance; worst ratio {float(r.max()):.3g} "
                             f"(err {float(err.reshape(-1)[i]):.3g}, tol {float(tol.reshape(-1)[i]):.3g})")
    return float((err / tol).max()) if err.numel() else 0.0


def _ulp_jitter(x, seed):
    """x (float32 values) moved by one float32 ulp up or down, element by element (fixed pattern)."""
    x = x.detach().to(F32)
    g = torch.Generator().manual_seed(seed)
    s = torch.randint(0, 2, x.shape, generator=g).bool()
    return torch.where(s, torch.nextafter(x, torch.full_like(x, float("inf"))), torch.nextafter(x, torch.full_like(x, float("-inf"))))


def contributions(fn, inputs, weights, seed=0):
    """Per-term contributions of sum(weights * fn(*inputs)) to each of `inputs` (autograd), in float64 and float32 (the float32 error
    measured on the exact inputs and on one-ulp-jittered inputs, the larger kept).  Returns [(c64, c32), ...] per input and
    the forward values (v64, v32)."""
    def run(dtype, jitter):
        xs = [(_ulp_jitter(x, jitter + i) if jitter else x).to(dtype).detach().requires_grad_(True) for i, x in enumerate(inputs)]
        v = fn(*xs)
        gs = torch.autograd.grad((v * weights.to(dtype)).sum(), xs, allow_unused=True)
        return v.detach().to(F64), [torch.zeros_like(x, dtype=F64) if g is None else g.detach().to(F64) for x, g in zip(xs, gs)]
    v64, g64 = run(F64, False)
    v32, g32 = run(F32, False)
    for j in range(JITTER_RUNS):
        vb, gb = run(F32, seed + 1000 * (j + 1))
        v32 = _worse(v32, vb, v64)
        g32 = [_worse(a, b, r) for a, b, r in zip(g32, gb, g64)]
    return list(zip(g64, g32)), (v64, v32)


def _worse(a, b, ref):
    """elementwise: whichever of two float32 evaluations lies farther from the float64 value."""
    return torch.where((a - ref).abs() >= (b - ref).abs(), a, b)


def f32_worst(fn, inputs, ref, seed):
    """fn(*inputs) in float32 on the exact inputs and on JITTER_RUNS one-ulp jitters of them: the evaluation farthest from `ref`."""
    out = fn(*[x.to(F32) for x in inputs]).to(F64)
    for j in range(JITTER_RUNS):
        out = _worse(out, fn(*[_ulp_jitter(x, seed + 1000 * (j + 1) + i) for i, x in enumerate(inputs)]).to(F64), ref)
    return out


# ------------------------------------------------------------------------------------------------ rasterize

def pixel_ndc(ix, iy, H, W, dtype=F64):
    """Pixel centres in NDC.  float32: the device's own rounding, ((float)ix + 0.5f) * (2.0f / W) - 1.0f."""
    ix, iy = torch.as_tensor(ix), torch.as_tensor(iy)
    if dtype == F32:
        sx, sy = torch.tensor(2.0 / W, dtype=F32), torch.tensor(2.0 / H, dtype=F32)
        return (ix.to(F32) + 0.5) * sx - 1.0, (iy.to(F32) + 0.5) * sy - 1.0
    return (ix.to(F64) + 0.5) * (2.0 / W) - 1.0, (iy.to(F64) + 0.5) * (2.0 / H) - 1.0


def _edge_fns(c, fx, fy):
    """c [..., 3, 4] clip corners, fx / fy broadcastable to [...]: homogeneous edge functions a [..., 3] (a_k opposite vertex k)."""
    px = c[..., 0] - fx[..., None] * c[..., 3]
    py = c[..., 1] - fy[..., None] * c[..., 3]
    a0 = px[..., 1] * py[..., 2] - py[..., 1] * px[..., 2]
    a1 = px[..., 2] * py[..., 0] - py[..., 2] * px[..., 0]
    a2 = px[..., 0] * py[..., 1] - py[..., 0] * px[..., 1]
    return torch.stack([a0, a1, a2], -1), px, py


def uvz(c, fx, fy):
    """(u, v, z/w) [..., 3] of corners c [..., 3, 4] at NDC (fx, fy): perspective-correct barycentrics of vertices 0 and 1 and the depth."""
    a, _, _ = _edge_fns(c, fx, fy)
    S = a.sum(-1)
    b = a * (1.0 / S)[..., None]
    z = (c[..., 2] * b).sum(-1)
    wp = (c[..., 3] * b).sum(-1)
    return torch.stack([b[..., 0], b[..., 1], z / wp], -1)


def fixed_path(pos, tri, H, W):
    """bool [F]: the faces whose coverage the header decides with 1/256-px fixed-point edge functions -- every w > 0 and every vertex
    within 2^20 px of the origin on screen; the others take the float homogeneous path."""
    c = torch.as_tensor(np.asarray(pos)).to(F64)[torch.as_tensor(np.asarray(tri)).long()]
    w = c[..., 3]
    sx = (c[..., 0] / w * 0.5 + 0.5) * W
    sy = (c[..., 1] / w * 0.5 + 0.5) * H
    return (w > 1e-12).all(-1) & (sx.abs() < 2.0 ** 20).all(-1) & (sy.abs() < 2.0 ** 20).all(-1)


def rasterize_truth(pos, tri, H, W, chunk=1 << 19):
    """Coverage truth.  Returns (ids [H, W] int64, -1 = empty; ambiguous [H, W] bool).

    A face covers a pixel when b0, b1, b2 >= 0, wp > 0 and z/w in [-1, 1] (float64, un-snapped); the nearest z/w wins, ties -> lower id.
    A pixel is ambiguous (its device id may legitimately differ) when a face that could own it -- the winner, or any face no farther than
    it -- has the pixel centre within the decision margin of one of its edges (SNAP_PX, or the float32 error of the homogeneous edge
    function on the float path), of wp = 0 or of z/w = +-1, or when two covering faces' depths lie within their float32 error."""
    pos = torch.as_tensor(np.asarray(pos)).to(F64)
    tri = torch.as_tensor(np.asarray(tri)).long()
    F = tri.shape[0]
    corners = pos[tri]                                                   # [F, 3, 4]
    c32 = corners.to(F32)
    w = corners[..., 3]
    allpos = (w > 1e-12).all(-1)
    fixed = fixed_path(pos, tri, H, W)
    # edge lines a_k = L_k . (fx, fy, 1): gradient in pixel units for the distance to the edge
    x, y = corners[..., 0], corners[..., 1]
    j, l = [1, 2, 0], [2, 0, 1]
    Lx = y[:, j] * w[:, l] - w[:, j] * y[:, l]
    Ly = w[:, j] * x[:, l] - x[:, j] * w[:, l]
    gnorm = torch.sqrt((2 * Lx / W) ** 2 + (2 * Ly / H) ** 2)              # [F, 3] |grad a_k| per pixel
    ids = torch.full((H * W,), -1, dtype=torch.long)
    amb = torch.zeros(H * W, dtype=torch.bool)
    pix = torch.arange(H * W)
    step = max(1, chunk // max(F, 1))
    for s in range(0, H * W, step):
        p = pix[s:s + step]
        ix, iy = p % W, p // W
        fx, fy = pixel_ndc(ix, iy, H, W)
        fx32, fy32 = pixel_ndc(ix, iy, H, W, F32)
        a, px, py = _edge_fns(corners[None], fx[:, None], fy[:, None])          # [P, F, 3]
        S = a.sum(-1)
        ok = S != 0
        Ss = torch.where(ok, S, torch.ones_like(S))
        b = a / Ss[..., None]
        wp = (corners[None, ..., 3] * b).sum(-1)
        zw = (corners[None, ..., 2] * b).sum(-1) / torch.where(wp != 0, wp, torch.ones_like(wp))
        cov = ok & (b >= 0).all(-1) & (wp > 0) & (zw >= -1) & (zw <= 1)
        # float32 depth of the same faces: the depth-tie gap
        a32, _, _ = _edge_fns(c32[None], fx32[:, None], fy32[:, None])
        S32 = a32.sum(-1)
        b32 = a32 / torch.where(S32 != 0, S32, torch.ones_like(S32))[..., None]
        wp32 = (c32[None, ..., 3] * b32).sum(-1)
        zw32 = ((c32[None, ..., 2] * b32).sum(-1) / torch.where(wp32 != 0, wp32, torch.ones_like(wp32))).to(F64)
        dz = (zw32 - zw).abs().nan_to_num(nan=1.0, posinf=1.0)
        # decision margin of each edge: SNAP_PX on the fixed path; on the float path the float32 error of a_k (two products of
        # |px| |py|, 8 ulp of each) in pixels
        dist = (a * torch.sign(Ss)[..., None]) / gnorm[None]              # signed distance, > 0 inside
        jj = torch.tensor(j); ll = torch.tensor(l)
        mag = (px[..., jj] * py[..., ll]).abs() + (py[..., jj] * px[..., ll]).abs()
        fl_margin = 8 * U32 * mag / gnorm[None]
        margin = torch.where(fixed[None, :, None], torch.full_like(dist, SNAP_PX), torch.maximum(fl_margin, torch.full_like(dist, SNAP_PX)))
        # near an edge of its own region: inside all edges to within the margin, and within the margin of at least one
        near_in = ok & (dist > -margin).all(-1) & ((dist.abs() <= margin).any(-1))
        near_in = near_in & (wp > 0) & (zw >= -1 - 4 * dz - 1e-7) & (zw <= 1 + 4 * dz + 1e-7)
        near_z = ok & cov & ((zw.abs() - 1).abs() <= 4 * dz + 1e-7)
        near_w = ok & (dist > -margin).all(-1) & (wp.abs() <= 1e-6 * w.abs().max(-1).values[None])
        big = torch.tensor(float("inf"), dtype=F64)
        zc = torch.where(cov, zw, big)
        zmin, win = zc.min(-1)                                           # first index among equal minima: lower id
        has = torch.isfinite(zmin)
        ids[p] = torch.where(has, win, torch.full_like(win, -1))
        zwin = torch.where(has, zmin, big)
        dzw = dz.gather(1, win[:, None])[:, 0]
        gap = 4 * (dz + dzw[:, None]) + 2.0 ** -30
        contender = (zw <= zwin[:, None] + gap) | ~has[:, None]
        a1 = ((near_in | near_z | near_w) & contender).any(-1)
        tie = (cov & (zw - zwin[:, None]).abs().le(gap)).sum(-1) > 1
        amb[p] = a1 | tie
    return ids.reshape(H, W), amb.reshape(H, W)


def covered_corners(pos, tri, ids):
    """For an id image (int [H, W], -1 empty): flat pixel indices of the covered pixels, their face ids and corners [N, 3, 4] (float64)."""
    pos = torch.as_tensor(np.asarray(pos)).to(F64)
    tri = torch.as_tensor(np.asarray(tri)).long()
    ids = torch.as_tensor(np.asarray(ids)).long().reshape(-1)
    p = torch.nonzero(ids >= 0)[:, 0]
    f = ids[p]
    return p, f, pos[tri[f]]


def rasterize_fields(pos, tri, ids, H, W, d_rast=None):
    """(u, v, z/w) of the faces in `ids` and -- with d_rast [H, W, 4] -- the gradient w.r.t. pos of sum(d_rast[..., :2] * (u, v)).
    Returns (Scatter of the per-pixel values [H*W, 3], Scatter of grad_pos [V, 4] or None)."""
    p, f, c = covered_corners(pos, tri, ids)
    V = np.asarray(pos).shape[0]
    fx, fy = pixel_ndc(p % W, p // W, H, W)
    fx32, fy32 = pixel_ndc(p % W, p // W, H, W, F32)
    vals = Scatter(H * W, 3)
    grads = None
    # forward values: float64 at exact pixel centres; float32 at the device's pixel centres
    v64 = uvz(c, fx, fy)
    v32 = f32_worst(lambda cc: uvz(cc, fx32, fy32), [c], v64, 11)
    v64 = torch.cat([v64[:, :2], v64[:, 2:].clamp(-1, 1)], 1)
    v32 = torch.cat([v32[:, :2], v32[:, 2:].clamp(-1, 1)], 1)
    vals.add(p, v64, v32)
    if d_rast is not None:
        g = torch.as_tensor(np.asarray(d_rast)).to(F64).reshape(-1, 4)[p, :2]
        tri_t = torch.as_tensor(np.asarray(tri)).long()

        def fn(cc):
            ffx, ffy = (fx, fy) if cc.dtype == F64 else (fx32, fy32)
            return uvz(cc, ffx, ffy)[:, :2]
        [(c64, c32)], _ = contributions(fn, [c], g)
        grads = Scatter(V * 4, 1)
        vid = tri_t[f]                                                   # [N, 3]
        idx = (vid[..., None] * 4 + torch.arange(4)).reshape(-1)
        grads.add(idx, c64.reshape(-1, 1), c32.reshape(-1, 1))
    return vals, grads


# ------------------------------------------------------------------------------------------------ interpolate

def interpolate_ref(attr, rast, tri, d_out=None):
    """out = u a_i0 + v a_i1 + (1 - u - v) a_i2 on the covered pixels of `rast` [H, W, 4] (the device's own (u, v) taken as exact inputs).
    Returns (Scatter out [H*W, A], Scatter grad_attr [V*A, 1] or None, Scatter grad_rast[..., :2] [H*W, 2] or None)."""
    attr = torch.as_tensor(np.asarray(attr)).to(F64)
    V, A = attr.shape
    rast = torch.as_tensor(np.asarray(rast)).to(F64).reshape(-1, 4)
    HW = rast.shape[0]
    ids = rast[:, 3].long() - 1
    p = torch.nonzero(ids >= 0)[:, 0]
    tri_t = torch.as_tensor(np.asarray(tri)).long()
    vid = tri_t[ids[p]]                                                  # [N, 3]
    uv = rast[p, :2]
    ca = attr[vid]                                                       # [N, 3, A]

    def terms(uv_, ca_):                                                 # [N, 3, A]: the three products of each channel
        b2 = 1.0 - uv_[:, 0] - uv_[:, 1]
        b = torch.stack([uv_[:, 0], uv_[:, 1], b2], 1)
        return b[..., None] * ca_
    t64 = terms(uv, ca)
    t32 = f32_worst(terms, [uv, ca], t64, 21)
    out = Scatter(HW, A)
    for k in range(3):
        out.add(p, t64[:, k], t32[:, k])
    if d_out is None:
        return out, None, None
    g = torch.as_tensor(np.asarray(d_out)).to(F64).reshape(HW, -1)[p, :A]
    # grad_attr: one term g * b_k per (pixel, corner, channel), summed by atomics into vertex vid[k]
    ga = Scatter(V * A, 1)
    idx = (vid[..., None] * A + torch.arange(A)).reshape(-1)
    gterm = lambda g_, uv_: (g_[:, None, :] * torch.stack([uv_[:, 0], uv_[:, 1], 1.0 - uv_[:, 0] - uv_[:, 1]], 1)[..., None])  # noqa: E731
    c64 = gterm(g, uv)
    ga.add(idx, c64.reshape(-1, 1), f32_worst(gterm, [g, uv], c64, 23).reshape(-1, 1))
    # grad_rast: per pixel, a sum over the channels of g (a_i0 - a_i2) and g (a_i1 - a_i2)
    gr = Scatter(HW, 2)
    rterm = lambda g_, ca_: torch.stack([g_ * (ca_[:, 0] - ca_[:, 2]), g_ * (ca_[:, 1] - ca_[:, 2])], -1)      # noqa: E731  [N, A, 2]
    r64 = rterm(g, ca)
    r32 = f32_worst(rterm, [g, ca], r64, 25)
    for a in range(A):
        gr.add(p, r64[:, a], r32[:, a])
    return out, ga, gr


# ------------------------------------------------------------------------------------------------ antialias

def opposite_table(tri, V):
    """other [F, 3] int64: for face f and its edge k (vertices k, k+1), the opposite vertex of the one other face on that edge, or -1
    when the edge is a silhouette by topology: a boundary edge (one face) or an edge with more than two faces (the header's rule)."""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    F = tri.shape[0]
    a, b, c = tri, np.roll(tri, -1, 1), np.roll(tri, -2, 1)
    lo, hi = np.minimum(a, b).ravel(), np.maximum(a, b).ravel()
    key = lo * (V + 1) + hi
    order = np.argsort(key, kind="stable")
    ks = key[order]
    start = np.r_[True, ks[1:] != ks[:-1]]
    grp = np.cumsum(start) - 1
    cnt = np.bincount(grp)[grp]
    other = np.full(3 * F, -1, np.int64)
    cs = c.ravel()[order]
    two = cnt == 2
    first = start & two
    i = np.nonzero(first)[0]
    other[order[i]] = cs[i + 1]
    other[order[i + 1]] = cs[i]
    valid = (a != b).ravel() & (tri >= 0).all(1).repeat(3)
    other[~valid] = -1
    return other.reshape(F, 3)


def _project(c, W, H):
    """clip [..., 4] -> pixel (X, Y): (x / w * 0.5 + 0.5) * W."""
    return (c[..., 0] / c[..., 3] * 0.5 + 0.5) * W, (c[..., 1] / c[..., 3] * 0.5 + 0.5) * H


def antialias_pairs(rast, pos, tri, other=None):
    """Every horizontal / vertical pixel pair with different ids, its nearer face, and that face's silhouette crossing in float64.
    Returns a dict of tensors over the pairs that the operator blends (found): P, O (flat pixel ids), f, va, vb (the crossing edge), d;
    and `amb` [all pairs] / `pairs_PO` [all pairs, 2]: the pairs whose decision lies within the float32 error of a threshold."""
    rast = torch.as_tensor(np.asarray(rast)).to(F64)
    H, W = rast.shape[0], rast.shape[1]
    pos = torch.as_tensor(np.asarray(pos)).to(F64)
    V = pos.shape[0]
    tri_t = torch.as_tensor(np.asarray(tri)).long()
    if other is None:
        other = opposite_table(tri_t.numpy(), V)
    other = torch.as_tensor(other)
    ids = rast[..., 3].long() - 1
    z = rast[..., 2]
    iy, ix = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    flat = iy * W + ix
    Ps, Qs = [flat[:, :-1].reshape(-1), flat[:-1, :].reshape(-1)], [flat[:, 1:].reshape(-1), flat[1:, :].reshape(-1)]
    p, q = torch.cat(Ps), torch.cat(Qs)
    idr, zr = ids.reshape(-1), z.reshape(-1)
    ta, tb = idr[p], idr[q]
    sel = ta != tb
    p, q, ta, tb = p[sel], q[sel], ta[sel], tb[sel]
    use_a = (tb < 0) | ((ta >= 0) & (zr[p] <= zr[q]))
    f = torch.where(use_a, ta, tb)
    P, O = torch.where(use_a, p, q), torch.where(use_a, q, p)
    n = len(f)
    vid = tri_t[f]                                                       # [n, 3]
    cw = pos[vid]                                                        # [n, 3, 4]
    okw = (cw[..., 3] > 1e-12).all(-1)
    X, Y = _project(cw, W, H)
    X = torch.where(okw[:, None], X, torch.zeros_like(X)); Y = torch.where(okw[:, None], Y, torch.zeros_like(Y))
    Px, Py = (P % W).to(F64) + 0.5, (P // W).to(F64) + 0.5
    Ox, Oy = (O % W).to(F64) + 0.5, (O // W).to(F64) + 0.5
    M = torch.maximum(torch.maximum(X.abs().amax(1), Y.abs().amax(1)), torch.tensor(float(max(W, H)), dtype=F64))
    ecoord = 4 * U32 * M                                                 # float32 error of a projected coordinate
    best = torch.full((n,), 2.0, dtype=F64)
    bestk = torch.full((n,), -1, dtype=torch.long)
    amb = torch.zeros(n, dtype=torch.bool)
    dlist, dtol = [], []
    for k in range(3):
        a, b, c = k, (k + 1) % 3, (k + 2) % 3
        ex, ey = X[:, b] - X[:, a], Y[:, b] - Y[:, a]
        el = torch.sqrt(ex * ex + ey * ey)
        els = torch.where(el > 0, el, torch.ones_like(el))
        sc = ex * (Y[:, c] - Y[:, a]) - ey * (X[:, c] - X[:, a])
        sgn = torch.sign(sc)
        eP = ex * (Py - Y[:, a]) - ey * (Px - X[:, a])
        eO = ex * (Oy - Y[:, a]) - ey * (Ox - X[:, a])

        def dtol_of(qx, qy, vertex):   # float32 error of the distance of point q to the edge line, pixels (x 8)
            r = torch.sqrt((qx - X[:, a]) ** 2 + (qy - Y[:, a]) ** 2)
            return 8 * ((2 if vertex else 1) * ecoord + r * 2 * ecoord / els + 2 * U32 * r)
        sP, sO, sC = eP * sgn / els, eO * sgn / els, sc.abs() / els
        tP, tO, tC = dtol_of(Px, Py, False), dtol_of(Ox, Oy, False), dtol_of(X[:, c], Y[:, c], True)
        den = eP - eO
        d = eP / torch.where(den != 0, den, torch.ones_like(den))
        qx, qy = Px + d * (Ox - Px), Py + d * (Oy - Py)
        tt = ((qx - X[:, a]) * ex + (qy - Y[:, a]) * ey) / torch.where(el > 0, el * el, torch.ones_like(el))
        tq = dtol_of(qx, qy, False)
        sd = (sP - sO).abs()
        td = (tP + tO) / torch.where(sd > 0, sd, torch.ones_like(sd))
        # silhouette by topology and screen side
        oth = other[f, k]
        has_o = oth >= 0
        qv = pos[oth.clamp(min=0)]
        o_ok = has_o & (qv[:, 3] > 1e-12)
        QX, QY = _project(qv, W, H)
        sQ = (ex * (QY - Y[:, a]) - ey * (QX - X[:, a])) * sgn / els
        tQ = dtol_of(QX, QY, True)
        sQ = torch.where(o_ok, sQ, torch.ones_like(sQ)); tQ = torch.where(o_ok, tQ, torch.zeros_like(tQ))
        # each condition: (holds in float64, within its float32 error of the threshold)
        conds = [
            (sC > 0, sC <= tC),                                          # sc != 0, and its sign
            (sP >= 0, sP.abs() <= tP),                                   # P inside
            (sO < 0, sO.abs() <= tO),                                    # O outside
            ((tt >= 0) & (tt <= 1), ((tt * el).abs() <= tq) | (((tt - 1) * el).abs() <= tq)),
            (sQ > 0, sQ.abs() <= tQ),                                    # silhouette: the neighbour's vertex on the same side
        ]
        holds = okw.clone()
        maybe = okw.clone()
        for h, m in conds:
            holds &= h & ~m
            maybe &= h | m
        near = maybe & ~holds                                            # the edge's qualification is not decided in float32
        amb |= near
        dlist.append(torch.where(holds | near, d, torch.full_like(d, 2.0)))
        dtol.append(torch.where(holds | near, td, torch.zeros_like(td)))
        take = holds & (d < best)
        best = torch.where(take, d, best)
        bestk = torch.where(take, torch.full_like(bestk, k), bestk)
    D, T = torch.stack(dlist, 1), torch.stack(dtol, 1)
    found = bestk >= 0
    tb_ = T.gather(1, bestk.clamp(min=0)[:, None])[:, 0]
    # two competing d within their error, or the best d within its error of 0.5
    for k in range(3):
        other_d = (D[:, k] < 1.5) & (bestk != k)
        amb |= found & other_d & ((D[:, k] - best).abs() <= T[:, k] + tb_)
    amb |= found & ((best - 0.5).abs() <= tb_)
    k = bestk.clamp(min=0)
    va = vid.gather(1, k[:, None])[:, 0]
    vb = vid.gather(1, ((k + 1) % 3)[:, None])[:, 0]
    return {"P": P[found], "O": O[found], "f": f[found], "va": va[found], "vb": vb[found], "d": best[found], "amb_found": amb[found],
            "amb": amb, "pairs_PO": torch.stack([P, O], 1), "n_pairs": n}


def _pair_d(ab, Pxy, Oxy, W, H):
    """d of the crossing of edge (A, B) (clip corners ab [n, 2, 4]) with the segment P -> O, in the dtype of ab."""
    X, Y = _project(ab, W, H)
    ex, ey = X[:, 1] - X[:, 0], Y[:, 1] - Y[:, 0]
    eP = ex * (Pxy[:, 1] - Y[:, 0]) - ey * (Pxy[:, 0] - X[:, 0])
    eO = ex * (Oxy[:, 1] - Y[:, 0]) - ey * (Oxy[:, 0] - X[:, 0])
    return eP / (eP - eO)


def antialias_ref(color, rast, pos, tri, d_out=None, boost=1.0, other=None):
    """Forward (Scatter [H*W, C]) and, with d_out, grad_color (Scatter [H*W, C]) and grad_pos (Scatter [V*4, 1]) of the antialias operator;
    plus the pair record of antialias_pairs (its `amb` marks the pairs the comparison must leave out)."""
    color = torch.as_tensor(np.asarray(color)).to(F64)
    H, W, C = color.shape
    pos_t = torch.as_tensor(np.asarray(pos)).to(F64)
    V = pos_t.shape[0]
    pr = antialias_pairs(rast, pos, tri, other)
    P, O, d64 = pr["P"], pr["O"], pr["d"]
    n = len(P)
    col = color.reshape(-1, C)
    ab = torch.stack([pos_t[pr["va"]], pos_t[pr["vb"]]], 1)               # [n, 2, 4]
    Pxy = torch.stack([(P % W).to(F64) + 0.5, (P // W).to(F64) + 0.5], 1)
    Oxy = torch.stack([(O % W).to(F64) + 0.5, (O // W).to(F64) + 0.5], 1)
    near = d64 < 0.5
    dst, src = torch.where(near, P, O), torch.where(near, O, P)

    def blend(ab_, cs, cd):                                              # [n, C]: the term added to out[dst]
        d = _pair_d(ab_, Pxy.to(ab_.dtype), Oxy.to(ab_.dtype), W, H)
        return (0.5 - d).abs()[:, None] * (cs - cd)
    out = Scatter(H * W, C).add_exact(torch.arange(H * W), col)
    ones = torch.ones(n, C, dtype=F64)
    _, (t64, t32) = contributions(blend, [ab, col[src], col[dst]], ones, seed=31)
    out.add(dst, t64, t32)
    if d_out is None:
        return out, None, None, pr
    g = torch.as_tensor(np.asarray(d_out)).to(F64).reshape(-1, C)
    gd = g[dst]
    [(cab64, cab32), (cs64, cs32), (cd64, cd32)], _ = contributions(blend, [ab, col[src], col[dst]], gd, seed=41)
    gc = Scatter(H * W, C).add_exact(torch.arange(H * W), g)
    gc.add(src, cs64, cs32)
    gc.add(dst, cd64, cd32)
    gp = Scatter(V * 4, 1)
    vv = torch.stack([pr["va"], pr["vb"]], 1)
    idx = (vv[..., None] * 4 + torch.arange(4)).reshape(-1)
    gp.add(idx, boost * cab64.reshape(-1, 1), boost * cab32.reshape(-1, 1))
    return out, gc, gp, pr


def ambiguous_pixels(pr, HW):
    """bool [HW]: pixels that an ambiguous pair touches."""
    m = torch.zeros(HW, dtype=torch.bool)
    po = pr["pairs_PO"][pr["amb"]]
    m[po.reshape(-1)] = True
    return m
