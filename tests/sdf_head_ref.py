"""A float64 model of the SDF head kernels (n2m_sdf_offsets / n2m_sdf_alpha_forward / n2m_sdf_alpha_backward, csrc/step_helpers.hip), per sample,
and the inputs ("cases") that the CPU and GPU tests of those kernels share.  No GPU is needed: tests/test_sdf_head_ref_cpu.py pins the model to
the project's torch statement and to finite differences, tests/test_sdf_head_gpu.py compares the kernels with it.

The model is written from the header comment of the kernels and from the torch statement in nerf2mesh_amd/{renderer,network}.py:
    normal = 0.5 (s+ - s-) / eps                      cos = safe_normalize(dir) . safe_normalize(normal)
    iter_cos = -(relu(0.5 - 0.5 cos) (1 - car) + relu(-cos) car)        inv_s = clip(exp(10 variance), 1e-6, 1e6)
    p = sigmoid((sdf - iter_cos dt / 2) inv_s)        q = sigmoid((sdf + iter_cos dt / 2) inv_s)
    alpha = clip((p - q + 1e-5) / (p + 1e-5), 0, 1)   eikonal summand (|normal| - 1)^2
The float32 inputs, eps and car are promoted exactly; everything after that is float64.  The backward is float64 autograd through that forward,
never a re-typed derivative."""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24                     # unit roundoff of float32
LAMBDA_EIK, SEED = 0.1, 64.0       # the eikonal weight and the loss-scale seed of every case

VARS, CARS, EPSS = (-0.3, 0.0, 0.35, 0.6), (0.0, 0.3, 1.0), (3e-2, 2e-3)
M_POP, M_LOOP = 4099, 65793        # the populations' size; 65793 samples = 258 partials, so the one-workgroup sum takes its stride loop
SIZES = (1, 63, 64, 65, 255, 256, 257, 4099)


def f32(x):
    """The value a C `float` parameter takes."""
    return float(np.float32(x))


def _t64(x):
    return (x.detach().cpu() if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))).to(torch.float64)


# ------------------------------------------------------------------------------------------------ offsets
def offsets(xyz, eps, bound):
    """pts[M,6,3], pts01[M,6,3] in float32, the kernel's own expression (add, clamp, (p + bound) / (2 bound)): comparable bit for bit.
    Copy k = 2 axis + (minus ? 1 : 0)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    eps, bound = np.float32(eps), np.float32(bound)
    off = np.zeros((6, 3), np.float32)
    for axis in range(3):
        off[2 * axis, axis] = eps
        off[2 * axis + 1, axis] = -eps
    pts = np.minimum(np.maximum(xyz[:, None, :] + off[None], -bound), bound).astype(np.float32)
    pts01 = ((pts + bound) / (np.float32(2.0) * bound)).astype(np.float32)
    return pts, pts01


# ------------------------------------------------------------------------------------------------ forward / backward
def _safe_normalize(x):
    return x / torch.sqrt(torch.clamp((x * x).sum(-1, keepdim=True), min=1e-20))


def _forward(sdf, s6, dirs, dt, var, eps, car):
    """The statement on torch tensors of one dtype; `var` is a scalar or a per-sample [M] tensor."""
    normal = torch.stack([0.5 * (s6[:, 0] - s6[:, 1]) / eps, 0.5 * (s6[:, 2] - s6[:, 3]) / eps, 0.5 * (s6[:, 4] - s6[:, 5]) / eps], dim=-1)
    cos = (_safe_normalize(dirs) * _safe_normalize(normal)).sum(-1)
    iter_cos = -(torch.relu(0.5 - 0.5 * cos) * (1.0 - car) + torch.relu(-cos) * car)
    inv_s = torch.exp(var * 10.0).clip(1e-6, 1e6)
    p = torch.sigmoid((sdf - iter_cos * dt * 0.5) * inv_s)
    q = torch.sigmoid((sdf + iter_cos * dt * 0.5) * inv_s)
    alpha = ((p - q + 1e-5) / (p + 1e-5)).clip(0, 1)
    nn = (normal * normal).sum(-1)
    eik_term = (torch.linalg.norm(normal, ord=2, dim=-1) - 1.0) ** 2          # (norm, not sqrt(nn): a zero vector has a zero gradient)
    return dict(alpha=alpha, normal=normal, eik_term=eik_term, cos=cos, p=p, nn=nn)


def _inputs64(sdf, s6, dirs, ts, var):
    sdf, s6, dirs, ts = _t64(sdf).reshape(-1), _t64(s6).reshape(-1, 6), _t64(dirs).reshape(-1, 3), _t64(ts).reshape(-1, 2)
    return sdf, s6, dirs, ts[:, 1], torch.tensor(float(np.float32(var)), dtype=torch.float64)


def alpha_forward(sdf, s6, dirs, ts, var, eps, car):
    """alpha[M], normal[M,3], eik_term[M] as float64 numpy arrays."""
    sdf, s6, dirs, dt, var = _inputs64(sdf, s6, dirs, ts, var)
    with torch.no_grad():
        f = _forward(sdf, s6, dirs, dt, var, f32(eps), f32(car))
    return f["alpha"].numpy(), f["normal"].numpy(), f["eik_term"].numpy()


def alpha_backward(d_alpha, sdf, s6, dirs, ts, var, eps, car, seed, eik_coef):
    """d_sdf[M], d_s6[M,6], d_var_term[M] (float64 numpy) of   sum(d_alpha alpha) + lambda mean((|n| - 1)^2) seed,   eik_coef = lambda 2 / M,
    by autograd.  d_var_term is the per-sample summand of d_variance: the variance enters as one copy per sample."""
    sdf, s6, dirs, dt, var = _inputs64(sdf, s6, dirs, ts, var)
    sdf, s6 = sdf.clone().requires_grad_(), s6.clone().requires_grad_()
    var_m = var.repeat(sdf.shape[0]).requires_grad_()
    f = _forward(sdf, s6, dirs, dt, var_m, f32(eps), f32(car))
    loss = (f["alpha"] * _t64(d_alpha).reshape(-1)).sum()
    if eik_coef != 0.0:
        loss = loss + 0.5 * f32(eik_coef) * f32(seed) * f["eik_term"].sum()
    if sdf.shape[0] == 0:
        return np.zeros(0), np.zeros((0, 6)), np.zeros(0)
    g_sdf, g_s6, g_var = torch.autograd.grad(loss, [sdf, s6, var_m])
    return g_sdf.numpy(), g_s6.numpy(), g_var.numpy()


def condition(sdf, s6, dirs, ts, var, eps, car):
    """bool[M]: the samples where float32 cannot be expected to agree with the model, from the model alone -- a cosine at a ReLU kink
    (|cos| < 1e-4) or at the pole of the normalisation's projection (1 - |cos| < 1e-4), a saturating sigmoid (1 - p < 1e-3: 1 - p then keeps
    fewer than 14 of float32's 24 bits), and |normal|^2 within a factor 4 of safe_normalize's clamp at 1e-20."""
    sdf, s6, dirs, dt, var = _inputs64(sdf, s6, dirs, ts, var)
    with torch.no_grad():
        f = _forward(sdf, s6, dirs, dt, var, f32(eps), f32(car))
    c, p, nn = f["cos"].abs(), f["p"], f["nn"]
    return ((c < 1e-4) | (1.0 - c < 1e-4) | (1.0 - p < 1e-3) | ((nn > 0.25e-20) & (nn < 4e-20))).numpy()


# ------------------------------------------------------------------------------------------------ error measures
def normalised_error(got, ref, median):
    """|got - ref| / (|ref| + median) per element; where that denominator is 0 the element must be exact (0 -> 0, else inf)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err, den = np.abs(got - ref), np.abs(ref) + median
    out = np.where(err == 0.0, 0.0, np.inf)
    np.divide(err, den, out=out, where=(den > 0) & (err > 0))
    return out


def var_sum_depth(nb):
    """Additions a summand of d_variance goes through: 6 wave levels + 2 for the four waves, the stride loop of the one-workgroup sum
    (ceil(nb / 256)) and that workgroup's own 6 + 2."""
    return 6 + 2 + (nb + 255) // 256 + 8


# ------------------------------------------------------------------------------------------------ cases
# A case is everything one call of the three kernels takes, as float32 CPU tensors and floats.  The grid cases are the random populations
# (one per variance x cos_anneal_ratio x eps); the others are directed at one branch each, built so that float32 and float64 take it alike.
class _Gen:
    """numpy's PCG64 stream as float32 torch tensors: torch's own CPU randn takes a host-specific vector path and is not the same everywhere."""
    def __init__(self, seed):
        self.g = np.random.Generator(np.random.PCG64(seed))

    def randn(self, *shape):
        return torch.from_numpy(self.g.standard_normal(shape).astype(np.float32))

    def rand(self, *shape):
        return torch.from_numpy(self.g.random(shape).astype(np.float32))


def _population(M, var, eps, gen):
    inv_s = min(max(math.exp(10.0 * var), 1e-6), 1e6)
    sdf = gen.randn(M) * np.float32(1.5 / inv_s)
    s6 = sdf.unsqueeze(1) + gen.randn(M, 6) * np.float32(1.2 * eps)
    dirs = gen.randn(M, 3) * 2.0
    ts = gen.rand(M, 2) * np.float32(0.01) + np.float32(0.002)
    d_alpha = gen.randn(M)
    return dict(sdf=sdf, s6=s6, dirs=dirs, ts=ts, d_alpha=d_alpha)


def grid_name(var, car, eps):
    return f"grid[var={var},car={car},eps={eps}]"


GRID = [(v, c, e) for v in VARS for c in CARS for e in EPSS]
STANDARD = grid_name(0.35, 0.3, 3e-2)          # the configuration the size sweep, the NULL outputs and the found_inf checks run on
DIRECTED = ("loop", "no_eikonal", "axis", "flat", "tiny_normal", "zero_dirs", "clip_high", "clip_low")
CASES = tuple(grid_name(*g) for g in GRID) + DIRECTED


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of case `name` (shared, do not modify): sdf[M], s6[M,6], dirs[M,3], ts[M,2], d_alpha[M], var, car, eps, seed, eik_coef, M."""
    gen = _Gen(1000 + CASES.index(name))
    var, car, eps, lam = 0.35, 0.3, 3e-2, LAMBDA_EIK
    if name.startswith("grid["):
        var, car, eps = GRID[CASES.index(name)]
        c = _population(M_POP, var, eps, gen)
    elif name == "loop":
        c = _population(M_LOOP, var, eps, gen)
    elif name == "no_eikonal":                   # eik_coef == 0 (and, on the device, seed = NULL)
        c, lam = _population(M_POP, var, eps, gen), 0.0
    elif name == "axis":
        # dirs = 2 e_z and a normal along z or x: cos is exactly +1, -1 or 0 in both precisions (sqrt(fl(x^2)) == |x|).  One sample in
        # eight has cos = +1, one cos = -1, six cos = 0: more than half of the d_sdf6 entries are then non-zero, and so is their median.
        M = 192
        c = _population(M, var, eps, gen)
        third = (torch.arange(M) % 8).clamp(max=2)                                    # 0: cos = +1, 1: cos = -1, 2: cos = 0
        c["dirs"] = torch.zeros(M, 3)
        c["dirs"][:, 2] = 2.0
        mag = (gen.rand(M) + 0.5) * np.float32(2.0 * eps)                           # s+ - s-: |normal| in [0.5, 1.5]
        s6 = c["sdf"].unsqueeze(1).repeat(1, 6)
        s6[third == 0, 4] += mag[third == 0]
        s6[third == 1, 5] += mag[third == 1]
        s6[third == 2, 0] += mag[third == 2]
        c["s6"] = s6
    elif name == "flat":                         # s6 == sdf in all six: zero normal, safe_normalize divides by 1e-10, no eikonal gradient
        c = _population(96, var, eps, gen)
        c["s6"] = c["sdf"].unsqueeze(1).repeat(1, 6)
    elif name == "tiny_normal":
        # |normal| in [1e-17, 1e-11]: |normal|^2 is a normal float32 below 1e-20, so the clamped branch runs with a non-zero normal and the
        # eikonal term is active.  The sdf values themselves are tiny so that their differences are representable.  Every third sample has
        # d_alpha = 0: its d_sdf6 is the eikonal part alone (of order 1, where the other rows' alpha part is ~1e9).  Those rows are judged on
        # their own, by relative error per element (TINY_EIKONAL_RELATIVE): under the case's median they would pass whatever their value.
        M = 128
        c = _population(M, var, eps, gen)
        mag = torch.from_numpy((10.0 ** (-17.0 + 6.0 * gen.g.random((M, 1)))).astype(np.float32))
        c["s6"] = (gen.randn(M, 6).double() * mag.double() * eps).to(torch.float32)
        c["sdf"] = c["s6"].mean(1)
        c["d_alpha"][::3] = 0.0
    elif name == "zero_dirs":                    # dirs = 0 for every other sample: the clamp of safe_normalize gives cos = 0
        c = _population(128, var, eps, gen)
        c["dirs"][::2] = 0.0
    elif name in ("clip_high", "clip_low"):
        # inv_s clips to 1e6 / 1e-6: d_variance is exactly 0.  At 1e6 a quarter of the samples keeps the population's dt (both sigmoids
        # saturate to 0 or 1), the rest gets dt ~ 1e-6 so that the gradients of the case are ordinary numbers.
        var = 1.5 if name == "clip_high" else -1.5
        M = 256
        c = _population(M, 0.0, eps, gen)
        if name == "clip_high":
            c["sdf"] = c["sdf"] * 1e-6
            c["s6"] = c["sdf"].unsqueeze(1) + gen.randn(M, 6) * np.float32(1.2 * eps)
            c["ts"][torch.arange(M) % 4 != 0] *= 1e-3
        else:
            c["sdf"] = c["sdf"] * 100.0
            c["s6"] = c["sdf"].unsqueeze(1) + gen.randn(M, 6) * np.float32(1.2 * eps)
    else:
        raise KeyError(name)
    M = c["sdf"].shape[0]
    c = {k: v.to(torch.float32).contiguous() for k, v in c.items()}
    c.update(name=name, M=M, var=var, car=car, eps=eps, seed=SEED, eik_coef=lam * 2.0 / M)
    return c


def uses_condition(name):
    """The random populations leave out what `condition` marks (at most 1 %); a directed case is compared whole."""
    return name.startswith("grid[") or name in ("loop", "no_eikonal")


@functools.lru_cache(maxsize=None)
def model(name):
    """The float64 model of case `name`, computed once: forward, backward, the ordinary samples and the medians the errors are normalised by."""
    c = case(name)
    a = (c["sdf"], c["s6"], c["dirs"], c["ts"], c["var"], c["eps"], c["car"])
    alpha, normal, eik_term = alpha_forward(*a)
    d_sdf, d_s6, d_var_term = alpha_backward(c["d_alpha"], *a, c["seed"], c["eik_coef"])
    ordinary = ~condition(*a) if uses_condition(name) else np.ones(c["M"], bool)
    med = lambda x: float(np.median(np.abs(x[ordinary]))) if ordinary.any() else 0.0
    return dict(alpha=alpha, normal=normal, eik_term=eik_term, d_sdf=d_sdf, d_s6=d_s6, d_var_term=d_var_term, ordinary=ordinary,
                med_d_sdf=med(d_sdf), med_d_s6=med(d_s6), med_d_var=med(d_var_term))


def errors(name, alpha, d_sdf, d_s6, d_var_term=None, rows=None):
    """The four figures a float32 evaluation of case `name` is judged by, over the ordinary samples (of the first `rows`): max absolute error
    of alpha; max normalised error of d_sdf, d_sdf6 and (when given) the d_variance summands -- those over all samples, since a sum can leave none out."""
    m = model(name)
    sl = slice(0, c_rows(name, rows))
    o = m["ordinary"][sl]
    e_alpha = np.abs(np.asarray(alpha, np.float64) - m["alpha"][sl])[o]
    e_sdf = normalised_error(d_sdf, m["d_sdf"][sl], m["med_d_sdf"])[o]
    e_s6 = normalised_error(d_s6, m["d_s6"][sl], m["med_d_s6"])[o]
    out = [float(e_alpha.max(initial=0.0)), float(e_sdf.max(initial=0.0)), float(e_s6.max(initial=0.0))]
    if d_var_term is not None:
        out.append(float(normalised_error(d_var_term, m["d_var_term"][sl], m["med_d_var"]).max(initial=0.0)))      # ALL samples: they are summed
    return tuple(out)


def c_rows(name, rows):
    return case(name)["M"] if rows is None else rows


# ------------------------------------------------------------------------------------------------ yardsticks
# What float32 itself costs on each case: the project's torch statement evaluated in float32 on the CPU (exp and sigmoid correctly rounded, so
# that the figures are the same on every host) against the model above, as
# (alpha: max absolute error; d_sdf, d_sdf6, d_variance summand: max normalised error |got - ref| / (|ref| + median |ref|)).  The kernels are
# allowed KERNEL_FACTOR times these: the device's expf and division may differ from the host's by a few ulp at each of about four chained steps.
# tests/test_sdf_head_ref_cpu.py::test_recorded_yardsticks_are_what_float32_gives recomputes every row and asserts measured <= recorded <=
# 2 measured.  A row above 1e-3 is kept but says little about the kernel (at var = -0.3 alpha is dominated by its 1e-5 guards).
KERNEL_FACTOR = 4.0
YARDSTICK = {
    "grid[var=-0.3,car=0.0,eps=0.03]": (9.8e-07, 0.0054, 7.7e-07, 0.013),
    "grid[var=-0.3,car=0.0,eps=0.002]": (6.6e-07, 0.0049, 9.8e-07, 0.0085),
    "grid[var=-0.3,car=0.3,eps=0.03]": (6.7e-07, 0.0058, 1.2e-06, 0.014),
    "grid[var=-0.3,car=0.3,eps=0.002]": (8.6e-07, 0.0058, 1.1e-06, 0.012),
    "grid[var=-0.3,car=1.0,eps=0.03]": (8.3e-07, 0.0067, 7.5e-07, 0.016),
    "grid[var=-0.3,car=1.0,eps=0.002]": (6.2e-07, 0.0085, 1.5e-06, 0.02),
    "grid[var=0.0,car=0.0,eps=0.03]": (6.8e-07, 0.00063, 1.6e-06, 0.00069),
    "grid[var=0.0,car=0.0,eps=0.002]": (5.6e-07, 0.00074, 2.2e-06, 0.0013),
    "grid[var=0.0,car=0.3,eps=0.03]": (5.3e-07, 0.00086, 2.3e-06, 0.0016),
    "grid[var=0.0,car=0.3,eps=0.002]": (7e-07, 0.00074, 3.5e-06, 0.001),
    "grid[var=0.0,car=1.0,eps=0.03]": (5.1e-07, 0.0035, 2.8e-06, 0.0031),
    "grid[var=0.0,car=1.0,eps=0.002]": (5.8e-07, 0.0027, 2.2e-06, 0.0038),
    "grid[var=0.35,car=0.0,eps=0.03]": (1e-06, 3.7e-05, 6.2e-06, 5.5e-05),
    "grid[var=0.35,car=0.0,eps=0.002]": (9.5e-07, 5e-05, 4.4e-06, 4.7e-05),
    "grid[var=0.35,car=0.3,eps=0.03]": (6.8e-07, 6.9e-05, 9e-06, 0.00013),
    "grid[var=0.35,car=0.3,eps=0.002]": (6.4e-07, 4.1e-05, 4.5e-06, 3.4e-05),
    "grid[var=0.35,car=1.0,eps=0.03]": (1e-06, 0.0018, 2.8e-05, 0.0012),
    "grid[var=0.35,car=1.0,eps=0.002]": (5.8e-07, 0.00094, 1.3e-05, 0.0011),
    "grid[var=0.6,car=0.0,eps=0.03]": (4.6e-07, 4.3e-06, 7.4e-06, 4e-06),
    "grid[var=0.6,car=0.0,eps=0.002]": (5.7e-07, 5e-06, 5.7e-06, 3.6e-06),
    "grid[var=0.6,car=0.3,eps=0.03]": (4.8e-07, 7.1e-06, 6.4e-06, 4.3e-06),
    "grid[var=0.6,car=0.3,eps=0.002]": (5.4e-07, 7.7e-06, 5.2e-06, 8.3e-06),
    "grid[var=0.6,car=1.0,eps=0.03]": (3.9e-07, 0.00083, 2.2e-05, 0.00073),
    "grid[var=0.6,car=1.0,eps=0.002]": (5.5e-07, 0.00019, 1.9e-05, 0.00019),
    "loop": (9.9e-07, 7.6e-05, 9.2e-06, 7.8e-05),
    "no_eikonal": (8.5e-07, 5e-05, 4.8e-06, 4.3e-05),
    "axis": (4.5e-07, 2.7e-05, 1.4e-06, 1.5e-05),
    "flat": (5e-07, 4.2e-05, 4.3e-07, 1e-05),
    "tiny_normal": (8.3e-08, 1e-05, 3.1e-07, 3.8e-07),
    "zero_dirs": (3.4e-07, 3.1e-05, 1e-06, 2.2e-05),
    "clip_high": (1.9e-05, 2.5e-05, 7.2e-05, 0),
    "clip_low": (1.7e-07, 0.0058, 1e-06, 0),
}
# the flat case's d_sdf6 by plain relative error per element |got - ref| / |ref| (its values are ~1e10 times an ordinary gradient); recomputed by
# tests/test_sdf_head_ref_cpu.py::test_recorded_flat_yardstick_is_what_float32_gives
FLAT_RELATIVE = 9.2e-07
# the d_alpha == 0 rows of the tiny_normal case, whose d_sdf6 is the clamped branch's eikonal gradient alone: plain relative error per element;
# recomputed by tests/test_sdf_head_ref_cpu.py::test_recorded_tiny_eikonal_yardstick_is_what_float32_gives
TINY_EIKONAL_RELATIVE = 2e-07


def tiny_eikonal_relative(d_s6):
    """Largest relative error per element of d_sdf6 over the d_alpha == 0 rows of the tiny_normal case."""
    rows = (case("tiny_normal")["d_alpha"] == 0).numpy()
    ref = model("tiny_normal")["d_s6"][rows]
    return float((np.abs(np.asarray(d_s6, np.float64)[rows] - ref) / np.abs(ref)).max())
