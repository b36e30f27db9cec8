"""Shared by tests/test_composite_loss_ref_cpu.py and tests/test_composite_loss_modes_gpu.py: a float64 model of n2m_composite_loss_train
(include/n2m_hip.h: compositing, the loss head with its optional entropy and depth terms, the backward scan), the inputs that put its edges
under test, the fp32 yardstick (the CPU oracle's forward -> the loss head in fp32 CPU torch -> the CPU oracle's backward) and the per-ray
error both are measured with.  numpy and CPU torch only.

Modes: "density" (alpha = 1 - exp(-sigma dt)), "alpha" (the SDF recipe: `sigmas` are the alphas, backward scale 1 / (1 - alpha)), "entropy"
(density + the entropy regulariser), "depth" (density + the sparse-depth term).

T_THRESH is 1e-3 here, not the recipes' 1e-4: alpha mode's placed stops use alpha = 0.9999 (the largest alpha these inputs hold), and a stop
on a ray's FIRST sample then leaves T = 1e-4 -- on the threshold itself at 1e-4, a factor of 10 below it at 1e-3.  Exact alpha == 1 is out of
scope: 1 / (1 - alpha) is inf there, un-guarded in the kernel as in the reference (raymarching.cu:671); the drivers clip alpha before it."""
import functools

import numpy as np
import torch

MODES = ("density", "alpha", "entropy", "depth")
T_THRESH = 1e-3
SCALE = 128.0                                    # the seed gradient (*grad_loss)
LAM_RGB, LAM_MASK, LAM_ENT, LAM_DEPTH = 1.0, 0.1, 0.05, 0.1        # (the recipe's lambda_entropy 1e-3 would hide in the rgb term's fp32 noise)
H_LO = float(np.float32(1e-5))                   # the entropy clamp, the fp32 numbers the kernel and fp32 torch clamp to
H_HI = float(np.float32(1.0) - np.float32(1e-5))

EDGE_COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129)                 # once dense (the longer ones stop), once thin (none stops); + LONG
LONG = 193                                       # no stop, T > 0.3 at its end: three 64-sample chunks carry gradients
PLACED = ((90, 0), (64, 63), (129, 63), (129, 64), (193, 127))     # (samples, index of the stop): first sample; a ray's last sample; last lane of a
#                                                                    chunk with two chunks behind it; first lane of a later chunk; last lane of one
CUT = 3                                          # the last ray's range overruns M by this many samples
CUT_COUNT = 101                                  # (long enough for its H(1e-5) samples to show in the entropy loss)


def _entropy(p):
    p = np.clip(p, H_LO, H_HI)
    return -p * np.log2(p) - (1 - p) * np.log2(1 - p)


def _entropy_grad(x):
    """d H(clamp(x)) / dx; the clamp passes the gradient on [H_LO, H_HI] inclusive (torch.clamp's backward)."""
    x = np.asarray(x, np.float64)
    inside = (x >= H_LO) & (x <= H_HI)
    xs = np.where(inside, x, 0.5)
    return np.where(inside, np.log2((1 - xs) / xs), 0.0)


def _suffix(x):
    """sum over j > i of x_j, along axis 0."""
    return np.cumsum(x[::-1], 0)[::-1] - x


def _lams(mode):
    return (LAM_ENT if mode == "entropy" else 0.0), (LAM_DEPTH if mode == "depth" else 0.0)


def model(case, mode, lam_rgb=LAM_RGB, lam_mask=LAM_MASK, bg="tensor"):
    """Float64 on the fp32 inputs.  bg: "tensor" (case["bg"]) or a float (uniform background).  Returns a dict of numpy arrays: loss, gs [M],
    gr [M,3], ws [N], image [N,3], depth [N], live [N], S [M] (the scale of gs: the sum of the absolute values of its terms, the suffix sums
    written as sums over j > i so that nothing cancels), T_after (list per ray), w [M], gs_explicit / gr_explicit (the backward written out;
    in entropy mode gs IS gs_explicit: the kernel and the reference apply grad_weights[i] to sample i's whole suffix term, raymarching.cu:676,
    which is not the derivative of the entropy of the later samples' weights -- autograd would be another function)."""
    assert mode in MODES
    lam_ent, lam_depth = _lams(mode)
    N, M, rays = case["N"], case["M"], case["rays"]
    sig = torch.from_numpy(case["sig"]).double().requires_grad_()
    rgb = torch.from_numpy(case["rgb"]).double().requires_grad_()
    ts = torch.from_numpy(case["ts"]).double()
    gt, gtd, dw = (torch.from_numpy(case[k]).double() for k in ("gt", "gtd", "dw"))
    bgt = torch.from_numpy(case["bg"]).double() if bg == "tensor" else torch.full((N, 3), float(bg), dtype=torch.float64)
    zero = torch.zeros((), dtype=torch.float64)
    image, wsum, depth, live, T_all, alphas = [], [], [], [], [], []
    w_all = np.zeros(M)
    for n in range(N):
        a, c = int(rays[n, 0]), int(rays[n, 1])
        if c == 0 or a + c > M:          # empty, or cut off by M: nothing composited, no gradient
            image.append(torch.zeros(3, dtype=torch.float64)); wsum.append(zero); depth.append(zero); live.append(0)
            T_all.append(np.zeros(0)); alphas.append(np.zeros(0))
            continue
        alpha = sig[a:a + c] if mode == "alpha" else 1 - torch.exp(-sig[a:a + c] * ts[a:a + c, 1])
        T_after = torch.cumprod(1 - alpha, 0)
        T_before = torch.cat([torch.ones(1, dtype=torch.float64), T_after[:-1]])
        below = torch.nonzero(T_after.detach() < T_THRESH)
        k = c if len(below) == 0 else int(below[0]) + 1          # the sample the stop falls on keeps its weight
        w = (alpha * T_before)[:k]
        image.append((w.unsqueeze(-1) * rgb[a:a + k]).sum(0)); wsum.append(w.sum()); depth.append((w * ts[a:a + k, 0]).sum()); live.append(k)
        T_all.append(T_after.detach().numpy()); alphas.append(alpha.detach().numpy())
        w_all[a:a + k] = w.detach().numpy()
    image, wsum, depth = torch.stack(image), torch.stack(wsum), torch.stack(depth)
    pred = image + (1 - wsum).unsqueeze(-1) * bgt
    mask = gt[:, 3:]
    target = gt[:, :3] * mask + bgt * (1 - mask)
    m = (gtd > 0).double()
    per_ray = lam_rgb * ((pred - target) ** 2).mean(-1) + lam_mask * (wsum - mask.squeeze(1)) ** 2 + lam_depth * dw * (depth * m - gtd * m) ** 2
    graph = per_ray.mean()
    (graph * SCALE).backward()
    ws_np, im_np, dp_np = wsum.detach().numpy(), image.detach().numpy(), depth.detach().numpy()
    loss = graph.item()
    if lam_ent:
        loss += lam_ent * (_entropy(w_all).mean() + _entropy(ws_np).mean())          # the mean over ALL M samples: zeros count as H(1e-5)
    # ---- the backward written out
    g = SCALE / N
    e = (pred - target).detach().numpy()
    gi_all = g * lam_rgb * 2 * e / 3
    gws_all = g * (lam_mask * 2 * (ws_np - case["gt"][:, 3].astype(np.float64)) + lam_ent * _entropy_grad(ws_np)) - (gi_all * bgt.numpy()).sum(-1)
    gd_all = g * lam_depth * case["dw"].astype(np.float64) * 2 * (dp_np - case["gtd"]) * (case["gtd"] > 0)
    gs_x, gr_x, S = np.zeros(M), np.zeros((M, 3)), np.zeros(M)
    rgb_np, ts_np = case["rgb"].astype(np.float64), case["ts"].astype(np.float64)
    for n in range(N):
        a, k = int(rays[n, 0]), live[n]
        if k == 0:
            continue
        w, T, col, t, dt = w_all[a:a + k], T_all[n][:k], rgb_np[a:a + k], ts_np[a:a + k, 0], ts_np[a:a + k, 1]
        gscl = 1 / (1 - alphas[n][:k]) if mode == "alpha" else dt
        gw = SCALE * lam_ent / M * _entropy_grad(w)               # grad_weights[i]
        gi, gws, gd = gi_all[n], gws_all[n], gd_all[n]
        wc = w[:, None] * col
        gs_x[a:a + k] = gscl * ((gi * (T[:, None] * col - _suffix(wc))).sum(-1) + (gws + gw) * (T - _suffix(w)) + gd * (T * t - _suffix(w * t)))
        S[a:a + k] = np.abs(gscl) * ((np.abs(gi) * (np.abs(T[:, None] * col) + _suffix(np.abs(wc)))).sum(-1)
                                     + np.abs(gws + gw) * (np.abs(T) + _suffix(np.abs(w))) + np.abs(gd) * (np.abs(T * t) + _suffix(np.abs(w * t))))
        gr_x[a:a + k] = gi[None] * w[:, None]
    ent = mode == "entropy"
    return dict(loss=loss, gs=gs_x if ent else sig.grad.numpy(), gr=gr_x if ent else rgb.grad.numpy(), ws=ws_np, image=im_np, depth=dp_np,
                live=np.array(live, np.int32), S=S, T_after=T_all, w=w_all, gs_explicit=gs_x, gr_explicit=gr_x)


def oracle_chain(case, mode, oracle, lam_rgb=LAM_RGB, lam_mask=LAM_MASK, bg="tensor"):
    """The fp32 yardstick: the oracle's serial forward, the loss head as fp32 CPU torch states it (tests/test_depth_loss_gpu._chain, + the
    entropy term of nerf/utils.py:728-733), the oracle's serial backward with grad_weights / grad_depth filled in where the mode has them."""
    lam_ent, lam_depth = _lams(mode)
    N, M, alpha_mode = case["N"], case["M"], mode == "alpha"
    w, ws, depth, im = oracle.composite_rays_train_forward(case["sig"], case["rgb"], case["ts"], case["rays"], T_THRESH, alpha_mode)
    tw, tws, td, tim = (torch.from_numpy(x.copy()).requires_grad_() for x in (w, ws, depth, im))
    gt, gtd, dw = (torch.from_numpy(case[k]) for k in ("gt", "gtd", "dw"))
    bgt = torch.from_numpy(case["bg"]) if bg == "tensor" else float(bg)
    pred = tim + (1 - tws).unsqueeze(-1) * bgt
    mask = gt[:, 3:]
    target = gt[:, :3] * mask + bgt * (1 - mask)
    loss = lam_rgb * ((pred - target) ** 2).mean(-1) + lam_mask * (tws - mask.squeeze(1)) ** 2
    if mode == "depth":
        m = (gtd > 0).float()
        loss = loss + lam_depth * dw * (td * m - gtd * m) ** 2
    loss = loss.mean()
    if mode == "entropy":
        ent = lambda p: (-p * torch.log2(p) - (1 - p) * torch.log2(1 - p)).mean()
        loss = loss + lam_ent * (ent(tw.clamp(1e-5, 1 - 1e-5)) + ent(tws.clamp(1e-5, 1 - 1e-5)))
    loss.backward(gradient=torch.tensor(SCALE))
    grad = lambda t: np.zeros(tuple(t.shape), np.float32) if t.grad is None else t.grad.numpy()
    gs, gr = oracle.composite_rays_train_backward(grad(tw), grad(tws), grad(td), grad(tim), case["sig"], case["rgb"], case["ts"], case["rays"],
                                                  ws, depth, im, T_THRESH, alpha_mode)
    live = np.zeros(N, np.int32)
    for n, (a, c) in enumerate(case["rays"].tolist()):
        nz = np.flatnonzero(w[a:min(a + c, M)])          # every alpha here is > 0: the weights end where the ray stopped
        live[n] = int(nz[-1]) + 1 if nz.size else 0
    return dict(loss=loss.item(), gs=gs, gr=gr, ws=ws, image=im, depth=depth, live=live, w=w)


def ray_errors(case, ref, gs, gr):
    """(e_gs, e_gr): the largest per-ray normalised error, max over rays of  max_{i in ray} |g_i - ref_i| / scale(ray)  with scale = the ray's
    largest S_i for grad_sigmas and the ray's sum of |ref| for grad_rgbs.  A ray whose scale is 0 must hold exact zeros (else inf)."""
    gs, gr = np.asarray(gs, np.float64), np.asarray(gr, np.float64)
    out = [0.0, 0.0]
    for a, c in case["rays"].tolist():
        if c == 0 or a + c > case["M"]:
            continue
        sl = slice(a, a + c)
        for q, (got, want, den) in enumerate(((gs[sl], ref["gs"][sl], ref["S"][sl].max()), (gr[sl], ref["gr"][sl], np.abs(ref["gr"][sl]).sum()))):
            err = np.abs(got - want).max() / den if den > 0 else (np.inf if got.any() else 0.0)
            out[q] = max(out[q], float(err))
    return tuple(out)


def loss_error(got, ref):
    return abs(float(got) - ref["loss"]) / abs(ref["loss"])


def check_conditions(case, mode, ref):
    """What the comparisons rest on, asserted on the float64 model: no stop decision near the threshold (fp32 and float64 stop at the same
    sample), every placed stop where it was placed, the long ray alive to its end, a non-zero scale on every live sample, and in entropy mode
    no weight near an end of the clamp (where H' jumps between 0 and +-16.6)."""
    for n, T in enumerate(ref["T_after"]):
        assert not ((T > T_THRESH / 2) & (T < T_THRESH * 2)).any(), (n, T)
    for n, idx in case["placed"]:
        assert ref["live"][n] == idx + 1 and idx + 1 <= case["rays"][n, 1], (n, idx, ref["live"][n])
    n = case["long"]
    assert case["rays"][n, 1] == LONG and ref["live"][n] == LONG and ref["T_after"][n][-1] > 0.3
    assert ref["live"][-1] == 0 and case["rays"][-1, 0] + case["rays"][-1, 1] == case["M"] + CUT
    for n, (a, c) in enumerate(case["rays"].tolist()):
        k = int(ref["live"][n])
        assert k == 0 or ref["S"][a:a + k].min() > 0, n
        if mode == "alpha" and k:
            assert case["sig"][a:a + c].max() <= 0.9999
        if mode == "entropy":
            for x in list(ref["w"][a:a + k]) + [ref["ws"][n]]:
                assert abs(x / H_LO - 1) > 1e-4 and abs(x - H_HI) > 2e-6, (n, x)      # fp32 sums of <= 193 terms: some 1e-7 of their value
    if mode != "alpha":          # the opaque samples leave 1 - alpha = 2^-18 to within fp32's rounding of sigma dt (see edge_case)
        i = np.array(case["opaque"])
        keep = np.exp(-case["sig"][i].astype(np.float64) * case["ts"][i, 1].astype(np.float64))
        assert (np.abs(keep * 2.0 ** 18 - 1) < 2e-6).all() and (-np.log(keep) >= 12).all()


@functools.lru_cache(maxsize=None)
def edge_case(mode, seed=0):
    """About 40 rays: EDGE_COUNTS with dense samples (alpha up to 0.25: the longer ones stop where their random transmittance first nears the
    threshold) and again with thin ones (no stop), the LONG ray, the PLACED stops (alpha <= 0.005 before the stop, one opaque sample on it:
    sigma dt = 12.48, or alpha = 0.9999 in alpha mode; dense samples behind it, which only a missed stop would see), a dozen random counts in [2, 100], shuffled; the LAST ray's range overruns M by CUT samples.  A third
    of the rays have gt alpha = 0, another third no keypoint depth.  The result is cached and shared: treat it as read-only."""
    assert mode in MODES
    rng = np.random.default_rng(seed)
    kinds = ([("dense", c, None) for c in EDGE_COUNTS] + [("thin", c, None) for c in EDGE_COUNTS] + [("long", LONG, None)]
             + [("placed", c, s) for c, s in PLACED] + [("dense", int(c), None) for c in rng.integers(2, 101, 12)])
    kinds = [kinds[i] for i in rng.permutation(len(kinds))] + [("dense", CUT_COUNT, None)]
    N = len(kinds)
    counts = np.array([k[1] for k in kinds])
    offs = np.concatenate([[0], np.cumsum(counts)])
    M = int(offs[-1]) - CUT
    rays = np.stack([offs[:-1], counts], -1).astype(np.int32)
    alpha, dt, tmid = np.zeros(offs[-1]), np.zeros(offs[-1]), np.zeros(offs[-1])
    opaque = []
    for n, (kind, c, stop) in enumerate(kinds):
        sl = slice(int(offs[n]), int(offs[n]) + c)
        dt[sl] = rng.random(c) * 0.02 + 0.005
        a = rng.random(c) * 0.25 + 1e-3
        if kind == "thin":
            a *= 0.2
        elif kind == "long":
            a = rng.random(c) * 0.01 + 1e-4
        elif kind == "placed":
            a[:stop] = rng.random(stop) * 0.0049 + 1e-5
            a[stop] = 0.9999
            dt[sl.start + stop] = 0.025
            opaque.append(sl.start + stop)
        alpha[sl] = a
        tmid[sl] = 0.3 + rng.random() + np.cumsum(dt[sl])
    sig = alpha if mode == "alpha" else -np.log1p(-alpha) / dt
    sig, dt = sig[:M].astype(np.float32), dt[:M].astype(np.float32)
    if mode != "alpha":
        # sigma dt = 18 ln 2 = 12.48, so that 1 - alpha = 2^-18.  fp32 holds alpha = 1 - exp(-sigma dt) next to 1 on a grid of 2^-24; at any other
        # sigma dt >= 12 the rounding of alpha alone puts ~1% on 1 - alpha and so on T -- in every fp32 form of this recurrence, the reference's
        # included -- and on the ray stopped at its first sample that is the whole gradient.  2^-18 lies on the grid.
        sig[opaque] = (18 * np.log(2.0) / dt[opaque].astype(np.float64)).astype(np.float32)
    # a stop the random data puts within a factor of 2 of the threshold is moved off it: that sample is made to end at T_thresh / 8
    for n in range(N - 1):
        a, c = int(offs[n]), int(counts[n])
        s64, d64 = sig[a:a + c].astype(np.float64), dt[a:a + c].astype(np.float64)
        T = np.cumprod(1 - (s64 if mode == "alpha" else 1 - np.exp(-s64 * d64)))
        near = np.flatnonzero(T < 2 * T_THRESH)
        if near.size and T[near[0]] > T_THRESH / 2:
            i = int(near[0])
            keep = T_THRESH / 8 / (T[i - 1] if i else 1.0)          # the 1 - alpha that sample needs
            sig[a + i] = 1 - keep if mode == "alpha" else -np.log(keep) / d64[i]
    ts = np.stack([tmid[:M], dt], -1).astype(np.float32)
    gt = rng.random((N, 4)).astype(np.float32)
    gt[::3, 3] = 0.0
    gtd = (0.4 + rng.random(N) * 1.5).astype(np.float32)
    gtd[1::3] = 0.0
    case = dict(mode=mode, N=N, M=M, rays=rays, sig=sig, ts=ts, rgb=rng.random((M, 3)).astype(np.float32), gt=gt,
                bg=rng.random((N, 3)).astype(np.float32), gtd=gtd, dw=(2.0 - rng.random(N) * 1.9).astype(np.float32),
                placed=[(n, k[2]) for n, k in enumerate(kinds) if k[0] == "placed"], opaque=opaque, long=[k[0] for k in kinds].index("long"))
    assert 35 <= N <= 60 and M < 6000 and len(case["placed"]) == len(PLACED)
    case["ref"] = model(case, mode)
    check_conditions(case, mode, case["ref"])
    return case


BIG_N = 16 * 1024 + 17                           # 1026 workgroups of 16 rays: the last workgroup's loop over the partials takes a second trip


@functools.lru_cache(maxsize=None)
def big_case(seed=0):
    """BIG_N rays of 0..3 samples (density mode, no stops: T >= 0.4), tiling [0, M).  Cached and shared: read-only."""
    rng = np.random.default_rng(seed)
    N = BIG_N
    counts = rng.integers(0, 4, N)
    offs = np.concatenate([[0], np.cumsum(counts)])
    M = int(offs[-1])
    dt = rng.random(M) * 0.02 + 0.005
    ts = np.stack([1.0 + rng.random(M), dt], -1).astype(np.float32)
    gt = rng.random((N, 4)).astype(np.float32)
    gt[::3, 3] = 0.0
    case = dict(N=N, M=M, rays=np.stack([offs[:-1], counts], -1).astype(np.int32), sig=(rng.random(M) * 12 + 0.01).astype(np.float32), ts=ts,
                rgb=rng.random((M, 3)).astype(np.float32), gt=gt, bg=rng.random((N, 3)).astype(np.float32))
    assert (N + 15) // 16 == 1026
    return case


def big_loss(case, dtype):
    """The loss of big_case, vectorised over rays in `dtype` (float64: the reference; float32: what plain fp32 arithmetic makes of it)."""
    t = lambda k: torch.from_numpy(case[k]).to(dtype)
    sig, ts, rgb, gt, bg = t("sig"), t("ts"), t("rgb"), t("gt"), t("bg")
    rays = torch.from_numpy(case["rays"]).long()
    lane = torch.arange(3)
    valid = lane[None] < rays[:, 1:]
    idx = torch.where(valid, rays[:, :1] + lane[None], torch.zeros((), dtype=torch.long))
    alpha = torch.where(valid, 1 - torch.exp(-sig[idx] * ts[idx, 1]), torch.zeros((), dtype=dtype))
    T_after = torch.cumprod(1 - alpha, 1)
    assert T_after.min() > 2 * T_THRESH
    w = alpha * torch.cat([torch.ones(case["N"], 1, dtype=dtype), T_after[:, :-1]], 1)
    ws, image = w.sum(1), (w.unsqueeze(-1) * rgb[idx]).sum(1)
    pred = image + (1 - ws).unsqueeze(-1) * bg
    mask = gt[:, 3:]
    target = gt[:, :3] * mask + bg * (1 - mask)
    return (LAM_RGB * ((pred - target) ** 2).mean(-1) + LAM_MASK * (ws - mask.squeeze(1)) ** 2).mean().item()
