"""Reference statements of the distortion loss on the ray weights (losses.distortion_loss, csrc/distortion.hip) -- a helper, not a
test.

model_f64:        the float64 O(n^2) DEFINITION, ray by ray: sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 d_i with the double sum written out
                  as an [n, n] array; the gradient is torch.autograd's of that same expression.  No prefix sums anywhere: an independent
                  statement of what the kernels compute in O(n).
restatement_f32:  the O(n) form in float32 with a SEQUENTIAL running sum per ray -- the yardstick: what plain fp32 arithmetic of the kernels'
                  formulas costs against the float64 model.  A kernel is allowed 4 x the largest error this shows over the same cases (the
                  factor covers the wave scan associating its sums as a tree; the rule of tests/test_ssim_gpu.py).
make_case:        packed (weights, ts, rays, nears, fars) from a list of per-ray sample counts.
"""
import functools

import numpy as np
import torch

SPACES = ("linear", "disparity")
KINDS = ("random", "peaked", "two_peaks", "early_stop", "zeros")
COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 0, 1024, 3, 0)       # both sides of every 64-sample chunk boundary, empty rays inside and at the end,
                                                               # the longest ray the marcher emits; 12 rays = three workgroups of four waves
SEEDS = (1.0, 1024.0)                                          # the gradient that arrives at loss_ray: 1, and a loss scale's size
DT_GAMMA, DT_MIN = 1.0 / 256, 2 * 3 ** 0.5 / 1024              # the marcher's step rule: dt = clamp(t * dt_gamma, dt_min, .)


def _weights(n, kind, rng):
    if n == 0:
        return np.zeros(0)
    if kind == "zeros":
        return np.zeros(n)
    if kind in ("random", "early_stop"):                       # alphas uniform -> front-to-back weights (opacity spread over the ray's length)
        alpha = rng.random(n) * min(1.0, 8.0 / n)
        w = alpha * np.concatenate([[1.0], np.cumprod(1 - alpha)[:-1]])
        if kind == "early_stop" and n >= 2:                    # exact zeros behind the sample the early stop fell on (T < T_thresh)
            w[n // 2:] = 0.0
        return w
    floor = rng.random(n) + 0.1
    if kind == "peaked":                                       # one sample carries 0.99, the others share 0.01
        k = int(rng.integers(n))
        w = 0.01 * floor / max(floor.sum() - floor[k], 1e-30)
        w[k] = 0.99
        return w
    if kind == "two_peaks":                                    # what the loss exists for: two separated surfaces, 0.45 each, 0.1 of haze
        a, b = n // 4, (3 * n) // 4
        rest = floor.copy()
        rest[[a, b]] = 0.0
        w = 0.1 * rest / max(rest.sum(), 1e-30)
        w[a] += 0.45
        w[b] += 0.45
        return w
    raise ValueError(kind)


def make_case(counts, kind, seed=0, gap=0):
    """Packed rays as march_rays_train + composite_rays_train leave them.  ts: t starts at the ray's near, dt follows the marcher's dt_gamma
    rule (geometric growth above dt_min), random stretches of empty space are skipped between samples; t is the value AFTER the step.
    far lies behind the last sample.  gap > 0: that many rows no ray owns in front of every ray (ranges that do not tile [0, M))."""
    rng = np.random.default_rng(seed)
    ws, tss, rays, nears, fars = [], [], [], [], []
    off = 0
    for n in counts:
        near = 0.2 + 0.6 * rng.random()
        t, rows = near, []
        for _ in range(n):
            if rng.random() < 0.15:
                t += max(t * DT_GAMMA, DT_MIN) * (1 + 7 * rng.random())
            dt = max(t * DT_GAMMA, DT_MIN)
            t += dt
            rows.append((t, dt))
        far = t * (1 + 0.5 * rng.random()) + 0.1
        off += gap if n else 0
        rays.append((off, n))
        off += n
        if gap and n:
            ws.append(np.full(gap, 0.25))                      # the rows in the gap hold values that must not be read
            tss.append(np.tile([[near + 1.0, 0.5]], (gap, 1)))
        ws.append(_weights(n, kind, rng))
        tss.append(np.array(rows).reshape(n, 2))
        nears.append(near)
        fars.append(far)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return (f(np.concatenate(ws)), f(np.concatenate(tss, 0)), torch.tensor(rays, dtype=torch.int32), f(np.array(nears)), f(np.array(fars)))


def _owned(rays, nears, fars, M):
    """(ray, offset, count) of the rays the term is formed over: samples, all inside [0, M), far > near."""
    for r, (off, cnt) in enumerate(rays.tolist()):
        if cnt > 0 and off >= 0 and off + cnt <= M and float(fars[r]) > float(nears[r]):
            yield r, off, cnt


def model_f64(weights, ts, rays, nears, fars, space="linear", grad_ray=None):
    """(loss_ray [N], mean, grad_weights [M]) in float64: the O(n^2) definition and autograd's gradient of sum_r grad_ray[r] * loss_ray[r]
    (grad_ray = None: ones)."""
    assert space in SPACES
    weights, ts, nears, fars = (t.detach().cpu().double() for t in (weights, ts, nears, fars))
    rays = rays.detach().cpu()
    w_all = weights.clone().requires_grad_(True)
    g = (lambda x: 1.0 / x) if space == "disparity" else (lambda x: x)
    N = rays.shape[0]
    loss_ray = [torch.zeros((), dtype=torch.float64) for _ in range(N)]
    for r, off, cnt in _owned(rays, nears, fars, weights.shape[0]):
        w, t, dt = w_all[off:off + cnt], ts[off:off + cnt, 0], ts[off:off + cnt, 1]
        gn, gf = g(nears[r]), g(fars[r])
        lo, hi = (g(t - dt) - gn) / (gf - gn), (g(t) - gn) / (gf - gn)
        m, d = (lo + hi) / 2, (hi - lo).abs()
        pair = w[:, None] * w[None, :] * (m[:, None] - m[None, :]).abs()
        loss_ray[r] = pair.sum() + (w * w * d).sum() / 3
    loss_ray = torch.stack(loss_ray)
    seed = torch.ones(N, dtype=torch.float64) if grad_ray is None else torch.as_tensor(grad_ray).detach().cpu().double().expand(N)
    (loss_ray * seed).sum().backward()
    return loss_ray.detach(), loss_ray.detach().mean(), w_all.grad.detach()


def restatement_f32(weights, ts, rays, nears, fars, space="linear", grad_ray=None):
    """(loss_ray [N], grad_weights [M]) as float32 arrays: the O(n) form, every operation rounded to float32, the running sums taken
    sequentially in sample order."""
    assert space in SPACES
    f = np.float32
    w_all, ts, nears, fars = (t.detach().cpu().float().numpy() for t in (weights, ts, nears, fars))
    N, M = rays.shape[0], w_all.shape[0]
    seed = np.ones(N, f) if grad_ray is None else np.broadcast_to(np.asarray(grad_ray, f), (N,))
    g = (lambda x: f(1) / x) if space == "disparity" else (lambda x: x)
    loss_ray, grad = np.zeros(N, f), np.zeros(M, f)
    for r, off, cnt in _owned(rays, nears, fars, M):
        w, t, dt = w_all[off:off + cnt], ts[off:off + cnt, 0], ts[off:off + cnt, 1]
        gn = g(nears[r])
        den = g(fars[r]) - gn
        lo, hi = (g(t - dt) - gn) / den, (g(t) - gn) / den
        m, d = (lo + hi) * f(0.5), np.abs(hi - lo)
        W, S, acc = f(0), f(0), f(0)
        W_lt, S_lt = np.empty(cnt, f), np.empty(cnt, f)
        for i in range(cnt):
            W_lt[i], S_lt[i] = W, S
            acc = acc + (f(2) * w[i] * (m[i] * W - S) + (w[i] * w[i] * d[i]) / f(3))
            W = W + w[i]
            S = S + w[i] * m[i]
        W_gt, S_gt = W - W_lt - w, S - S_lt - w * m
        loss_ray[r] = acc
        grad[off:off + cnt] = seed[r] * (f(2) * (m * (W_lt - W_gt) - S_lt + S_gt) + (f(2) * w * d) / f(3))
        assert acc.dtype == f and grad.dtype == f and m.dtype == f
    return loss_ray, grad


def loss_error(loss_ray, ref_loss_ray):
    """Largest absolute error of the per-ray loss (L_ray <= 1 + 1/3 whenever the weights of a ray sum to at most 1)."""
    return float((torch.as_tensor(loss_ray).double() - ref_loss_ray).abs().max())


def grad_error(grad, ref_grad, rays):
    """Largest over the rays of max |grad - ref| / max |ref| over the ray's samples.  A ray whose reference gradient is exactly zero
    everywhere (all its weights are zero: every term of dL/dw_i carries a weight) has no scale to divide by; there the gradient must be
    exactly zero as well, which is asserted here, and the ray adds nothing to the measure."""
    grad, worst = torch.as_tensor(grad).double(), 0.0
    for off, cnt in rays.tolist():
        if cnt == 0:
            continue
        ref, got = ref_grad[off:off + cnt], grad[off:off + cnt]
        top = float(ref.abs().max())
        if top == 0.0:
            assert float(got.abs().max()) == 0.0, "a ray of zero weights has a non-zero gradient"
            continue
        worst = max(worst, float((got - ref).abs().max()) / top)
    return worst


@functools.lru_cache(maxsize=None)
def case(kind, gap=0):
    return make_case(COUNTS, kind, seed=KINDS.index(kind) + 1, gap=gap)


@functools.lru_cache(maxsize=None)
def reference(kind, space, seed=1.0):
    """model_f64 of case(kind), computed once and shared (treat as read-only)."""
    return model_f64(*case(kind), space=space, grad_ray=seed)


@functools.lru_cache(maxsize=None)
def yardstick():
    """The fp32 restatement's largest errors against the float64 model over the whole case set (every kind, both spaces, both seeds):
    {"loss": absolute, "grad": relative per ray, "per_kind": {kind: (loss, grad)}}."""
    per_kind = {}
    for kind in KINDS:
        el = eg = 0.0
        for space in SPACES:
            for seed in SEEDS:
                ref_loss, _, ref_grad = reference(kind, space, seed)
                loss_ray, grad = restatement_f32(*case(kind), space=space, grad_ray=seed)
                el = max(el, loss_error(loss_ray, ref_loss))
                eg = max(eg, grad_error(grad, ref_grad, case(kind)[2]))
        per_kind[kind] = (el, eg)
    return {"loss": max(v[0] for v in per_kind.values()), "grad": max(v[1] for v in per_kind.values()), "per_kind": per_kind}
