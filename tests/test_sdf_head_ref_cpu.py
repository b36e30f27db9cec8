"""The float64 model of the SDF head (tests/sdf_head_ref.py) on the CPU: against the project's torch statement, against central differences and
closed forms, and the float32 yardsticks and exclusion shares that tests/test_sdf_head_gpu.py relies on."""
import functools
import json
import os
import subprocess
import sys
import types
from unittest import mock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sdf_head_ref as R


class _Exp32(torch.autograd.Function):
    """float32 exp, correctly rounded (through float64); backward g y in float32, as torch's."""
    @staticmethod
    def forward(ctx, x):
        y = torch_exp(x.double()).to(x.dtype)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0]


class _Sigmoid32(torch.autograd.Function):
    """float32 sigmoid, correctly rounded (through float64); backward g y (1 - y) in float32, as torch's."""
    @staticmethod
    def forward(ctx, x):
        y = torch_sigmoid(x.double()).to(x.dtype)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        y = ctx.saved_tensors[0]
        return g * ((1.0 - y) * y)


class _Sqrt32(torch.autograd.Function):
    """float32 sqrt, correctly rounded (the float64 root of a float32 rounds to it without a double-rounding error); backward g / (2 y)."""
    @staticmethod
    def forward(ctx, x):
        y = torch_sqrt(x.double()).to(x.dtype)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        return g / (2.0 * ctx.saved_tensors[0])


torch_exp, torch_sigmoid, torch_sqrt = torch.exp, torch.sigmoid, torch.sqrt


def project_statement(c, dtype, grads=True):
    if dtype == torch.float32:
        # The host decides the last bit of torch's float32 exp, sigmoid and sqrt (the same input gave different roots on two CPUs, seen), and
        # with it the largest error among thousands of samples, by a factor of up to 10.  The yardstick must be one number everywhere: these
        # three functions are evaluated correctly rounded; +, -, *, / are IEEE operations and the same on every host.
        with mock.patch.object(torch, "exp", _Exp32.apply), mock.patch.object(torch, "sigmoid", _Sigmoid32.apply), \
                mock.patch.object(torch, "sqrt", _Sqrt32.apply):
            return _project_statement(c, dtype, grads)
    return _project_statement(c, dtype, grads)


def _project_statement(c, dtype, grads):
    """The SDF branch as the project states it in torch (renderer.render / NeRFRenderer._sdf_to_alpha / network.normal, the eikonal term of
    trainer.py), in `dtype`, with the variance as one copy per sample.  Returns numpy arrays: alpha, normal, eik_term[, d_sdf, d_s6, d_var_term]."""
    from nerf2mesh_amd.renderer import NeRFRenderer, safe_normalize
    eps, car = R.f32(c["eps"]), R.f32(c["car"])
    sdf, s6 = c["sdf"].to(dtype).clone().requires_grad_(grads), c["s6"].to(dtype).clone().requires_grad_(grads)
    dirs, dt = c["dirs"].to(dtype), c["ts"][:, 1].to(dtype)
    var = torch.full((c["M"],), R.f32(c["var"]), dtype=dtype).requires_grad_(grads)
    normal = torch.stack([0.5 * (s6[:, 0] - s6[:, 1]) / eps, 0.5 * (s6[:, 2] - s6[:, 3]) / eps, 0.5 * (s6[:, 4] - s6[:, 5]) / eps], dim=-1)
    true_cos = (safe_normalize(dirs) * safe_normalize(normal)).sum(-1)
    iter_cos = -(F.relu(-true_cos * 0.5 + 0.5) * (1.0 - car) + F.relu(-true_cos) * car)
    alpha = NeRFRenderer._sdf_to_alpha(types.SimpleNamespace(variance=var), sdf, iter_cos, dt)
    eik_term = (torch.linalg.norm(normal, ord=2, dim=-1) - 1) ** 2
    out = [alpha, normal, eik_term]
    if grads:
        lam = c["eik_coef"] * c["M"] / 2.0
        loss = (alpha * c["d_alpha"].to(dtype)).sum() + lam * eik_term.mean() * c["seed"]
        out += list(torch.autograd.grad(loss, [sdf, s6, var]))
    return [t.detach().double().numpy() for t in out]


def args(c):
    return c["sdf"], c["s6"], c["dirs"], c["ts"], c["var"], c["eps"], c["car"]


@pytest.mark.parametrize("name", R.CASES)
def test_model_forward_equals_the_torch_statement_in_float64(name):
    c = R.case(name)
    alpha, normal, eik = R.alpha_forward(*args(c))
    want = project_statement(c, torch.float64, grads=False)
    for got, ref in zip((alpha, normal, eik), want):
        assert got.shape == ref.shape and np.all(np.abs(got - ref) <= 1e-12 * np.maximum(1.0, np.abs(ref))), name


def test_model_backward_against_central_differences():
    """Autograd of the model against central differences of its own float64 forward on 200 ordinary samples (away from the kinks by much
    more than a step).  Samples are independent, so one coordinate (sdf, one of the six copies, the variance) of ALL samples moves at once.
    Step: h = 1e-6 of the coordinate's scale (1 / inv_s for the sdf, eps for a copy, 1 / 10 for the variance).  Tolerance, per value:
      * truncation: D(h) = f' + h^2 f''' / 6 + O(h^4), so D(2h) - D(h) = 3 (h^2 f''' / 6): three times the second-order error of D(h),
        measured from the model itself;
      * rounding: alpha is a quotient of a difference of two sigmoids of order 1, so whatever its own size each evaluation carries an
        absolute error of a few 2^-53: (|d_alpha| + |l|) 2^-52 * 8 say, divided by 2h; and x + h, x - h are rounded
        themselves, so the step actually taken is 2h (1 +- 2^-52 |x| / h).
    The per-sample loss l = d_alpha alpha + (eik_coef / 2) seed (|n| - 1)^2 is what alpha_backward differentiates."""
    c = R.case(R.STANDARD)
    sdf, s6, dirs, dt, var = R._inputs64(*args(c)[:5])
    eps, car = R.f32(c["eps"]), R.f32(c["car"])
    f0 = R._forward(sdf, s6, dirs, dt, var, eps, car)
    n_len = f0["nn"].sqrt()
    ok = (f0["alpha"] > 1e-3) & (f0["alpha"] < 1 - 1e-3) & (f0["cos"].abs() > 1e-3) & (f0["cos"].abs() < 1 - 1e-3) & (n_len > 0.05)
    pick = torch.nonzero(ok).reshape(-1)[:200]
    assert pick.numel() == 200
    d_alpha = c["d_alpha"].double()

    def loss(sdf_, s6_, var_):
        f = R._forward(sdf_, s6_, dirs, dt, var_, eps, car)
        return (d_alpha * f["alpha"] + 0.5 * R.f32(c["eik_coef"]) * c["seed"] * f["eik_term"])[pick]

    var_m = var.repeat(c["M"])
    g_sdf, g_s6, g_var = R.alpha_backward(c["d_alpha"], *args(c), c["seed"], c["eik_coef"])
    inv_s = float(torch.exp(var * 10.0))
    coords = [("sdf", 1.0 / inv_s, g_sdf, sdf)] + [(k, eps, g_s6[:, k], s6[:, k]) for k in range(6)] + [("var", 0.1, g_var, var_m)]
    l0 = loss(sdf, s6, var_m).abs() + d_alpha[pick].abs()
    for key, scale, grad, x in coords:
        def diff(h):
            def at(sign):
                if key == "sdf":
                    return loss(sdf + sign * h, s6, var_m)
                if key == "var":
                    return loss(sdf, s6, var_m + sign * h)
                s = s6.clone()
                s[:, key] += sign * h
                return loss(sdf, s, var_m)
            return (at(+1.0) - at(-1.0)) / (2.0 * h)
        h = 1e-6 * scale
        d1, d2 = diff(h), diff(2.0 * h)
        tol = (d2 - d1).abs() + 8.0 * 2.0 ** -52 * l0 / (2.0 * h) + 2.0 ** -52 * x[pick].abs() / h * d1.abs()
        err = (d1 - torch.from_numpy(grad)[pick]).abs()
        assert bool((err <= tol).all()), (key, float((err / tol).max()))
        # ... and the bound is a sharp one: a gradient off by 1e-6 of its size would not pass
        assert float((tol / (d1.abs() + 1e-300)).median()) < 1e-6, key


def closed_dtc(c, idx):
    """d loss / d cos of samples with cos == 0 exactly, typed out in float64 numpy: iter_cos = -(1 - car) / 2, only the relu(0.5 - 0.5 cos)
    branch passes a gradient."""
    sdf, dt, g = (c[k].double().numpy()[idx] for k in ("sdf", "ts", "d_alpha"))
    dt, car = dt[:, 1], R.f32(c["car"])
    s = min(max(np.exp(10.0 * R.f32(c["var"])), 1e-6), 1e6)
    h = -0.5 * (1.0 - car) * dt * 0.5
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    p, q = sig((sdf - h) * s), sig((sdf + h) * s)
    du, dv = g * q / (p + 1e-5) ** 2 * p * (1 - p), -g / (p + 1e-5) * q * (1 - q)
    dic = s * (dv - du) * dt * 0.5
    return 0.5 * (1.0 - car) * dic


def test_model_closed_forms_of_the_directed_cases():
    # flat samples: normal = 0, no eikonal gradient, d_sdf6 = +-0.5 dtc dir^ / 1e-10 / eps
    c, m = R.case("flat"), R.model("flat")
    assert not m["normal"].any() and np.all(m["eik_term"] == 1.0)
    d = c["dirs"].double().numpy()
    dh = d / np.sqrt((d * d).sum(-1, keepdims=True))
    want = 0.5 * closed_dtc(c, slice(None))[:, None] * dh / 1e-10 / R.f32(c["eps"])
    for a in range(3):
        np.testing.assert_allclose(m["d_s6"][:, 2 * a], want[:, a], rtol=1e-9)
        np.testing.assert_allclose(m["d_s6"][:, 2 * a + 1], -want[:, a], rtol=1e-9)
    # axis-aligned samples
    c, m = R.case("axis"), R.model("axis")
    kind = np.minimum(np.arange(c["M"]) % 8, 2)
    n = m["normal"]
    n_len = np.sqrt((n * n).sum(-1))
    eik = 0.5 * (R.f32(c["eik_coef"]) * c["seed"] * (n_len - 1.0) / n_len)[:, None] * n / R.f32(c["eps"])     # the + copies' eikonal part
    s = np.exp(10.0 * R.f32(c["var"]))
    p = 1.0 / (1.0 + np.exp(-c["sdf"].double().numpy() * s))
    plus = kind == 0                    # cos = +1: iter_cos = 0, p == q, alpha = 1e-5 / (p + 1e-5), d_sdf6 is the eikonal part alone
    np.testing.assert_allclose(m["alpha"][plus], 1e-5 / (p[plus] + 1e-5), rtol=1e-12)
    np.testing.assert_allclose(m["d_s6"][plus][:, 0::2], eik[plus], rtol=1e-9, atol=1e-18)
    np.testing.assert_allclose(m["d_s6"][plus][:, 1::2], -eik[plus], rtol=1e-9, atol=1e-18)
    minus = kind == 1                   # cos = -1: the gradient of the cosine is along the normal and the normalisation projects it out
    np.testing.assert_allclose(m["d_s6"][minus][:, 0::2], eik[minus], rtol=1e-9, atol=1e-12)
    zero = kind == 2                    # cos = 0: relu(-cos) passes nothing; the normal is along x, the cosine's gradient along z
    want = eik[zero].copy()
    want[:, 2] += 0.5 * closed_dtc(c, zero) * 1.0 / n_len[zero] / R.f32(c["eps"])
    np.testing.assert_allclose(m["d_s6"][zero][:, 0::2], want, rtol=1e-9, atol=1e-18)
    # the clipped variances: no gradient to the variance, none of it NaN
    for name in ("clip_high", "clip_low"):
        m = R.model(name)
        assert not m["d_var_term"].any() and all(np.isfinite(m[k]).all() for k in ("alpha", "d_sdf", "d_s6"))
    # the quarter that keeps the population's dt: nearly all of it has both sigmoids saturated, alpha is the clip's 0, 1e-5 / (1 + 1e-5) or 1
    assert np.isin(np.round(R.model("clip_high")["alpha"][0::4] * 1e5), (0.0, 1.0, 1e5)).mean() > 0.9
    # the tiny normals sit in the clamped branch, with an active eikonal term
    n = R.model("tiny_normal")["normal"]
    nn32 = (n.astype(np.float32) ** 2).sum(-1)
    assert np.all(nn32 < 0.25e-20) and np.all(nn32 > 1e-36) and np.all(np.sqrt((n * n).sum(-1)) > 1e-18)
    # ... whose gradient stands alone in the d_alpha == 0 rows: 0.5 eik_coef seed (|n| - 1) n^ / eps, of order 1, and the whole of those rows
    c, m = R.case("tiny_normal"), R.model("tiny_normal")
    rows = (c["d_alpha"] == 0).numpy()
    assert rows.sum() == 43 and np.array_equal(np.flatnonzero(rows), np.arange(0, 128, 3))
    n_len = np.sqrt((n * n).sum(-1, keepdims=True))
    want = 0.5 * R.f32(c["eik_coef"]) * c["seed"] * (n_len - 1.0) * (n / n_len) / R.f32(c["eps"])
    np.testing.assert_allclose(m["d_s6"][rows][:, 0::2], want[rows], rtol=1e-9)
    np.testing.assert_allclose(m["d_s6"][rows][:, 1::2], -want[rows], rtol=1e-9)
    assert np.abs(m["d_s6"][rows]).min() > 0 and np.abs(m["d_s6"][rows]).max() < 10 and m["med_d_s6"] > 1e6
    # without the eikonal term those rows would be zero: a relative check of them sees the term, the case's median does not
    a = (c["sdf"], c["s6"], c["dirs"], c["ts"], c["var"], c["eps"], c["car"])
    without = R.alpha_backward(c["d_alpha"], *a, c["seed"], 0.0)[1]
    assert not without[rows].any() and R.tiny_eikonal_relative(without) == 1.0


def test_offsets_model():
    xyz = np.array([[0.25, -0.5, 0.75], [1.0, -1.0, 0.99], [1.5, -2.0, 0.0]], np.float32)
    pts, pts01 = R.offsets(xyz, 3e-2, 1.0)
    assert pts.dtype == np.float32 and pts.shape == (3, 6, 3) and pts01.shape == (3, 6, 3)
    assert pts[0, 0, 0] == np.float32(0.25) + np.float32(3e-2) and pts[0, 3, 1] == np.float32(-0.5) - np.float32(3e-2)
    assert np.array_equal(pts[0, 4, :2], xyz[0, :2]) and pts[1, 0, 0] == 1.0 and pts[1, 3, 1] == -1.0 and pts[2, 1, 0] == 1.0
    assert pts01.min() == 0.0 and pts01.max() == 1.0 and pts01[2, 0, 2] == np.float32(0.5)


@pytest.mark.parametrize("name", [n for n in R.CASES if R.uses_condition(n)])
def test_condition_leaves_out_at_most_one_percent(name):
    """The cap on what the GPU tests may leave out of a random population."""
    m = R.model(name)
    share = 1.0 - m["ordinary"].mean()
    print(f"{name}: excluded {share:.4%}")
    assert share <= 0.01


def measure_yardstick(name):
    c = R.case(name)
    alpha, _, _, d_sdf, d_s6, d_var = project_statement(c, torch.float32)
    return R.errors(name, alpha, d_sdf, d_s6, d_var)


def measure_flat_relative():
    m = R.model("flat")
    d_s6 = project_statement(R.case("flat"), torch.float32)[4]
    return float((np.abs(d_s6 - m["d_s6"]) / np.abs(m["d_s6"])).max())


def measure_tiny_eikonal_relative():
    return R.tiny_eikonal_relative(project_statement(R.case("tiny_normal"), torch.float32)[4])


@functools.lru_cache(maxsize=None)
def measured():
    """Every yardstick, measured once in a child process whose torch uses its plain CPU kernels, not the ones picked for the host's vector
    unit: a precaution on top of the correctly rounded functions of project_statement, so that the order of the short sums does not depend on
    the host either.  The figures have to be the same everywhere: a few nearly singular samples decide a population's largest error."""
    env = dict(os.environ, ATEN_CPU_CAPABILITY="default", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, check=True, capture_output=True, text=True, timeout=300).stdout
    return json.loads(out.strip().splitlines()[-1])


@pytest.mark.parametrize("name", R.CASES)
def test_recorded_yardsticks_are_what_float32_gives(name):
    """The float32 torch statement against the float64 model on the case's own inputs: measured <= recorded <= 2 measured, for each of
    alpha (absolute), d_sdf, d_sdf6 and the d_variance summands (normalised by |ref| + median |ref|)."""
    got_all, recorded = measured()[name], R.YARDSTICK[name]
    print(f"{name}: measured {got_all}, recorded {recorded}")
    for got, rec in zip(got_all, recorded):
        assert got <= rec <= 2.0 * got, (name, got_all, recorded)


def test_recorded_flat_yardstick_is_what_float32_gives():
    got = measured()["flat_relative"]
    print(f"flat: measured relative {got}, recorded {R.FLAT_RELATIVE}")
    assert got <= R.FLAT_RELATIVE <= 2.0 * got


def test_recorded_tiny_eikonal_yardstick_is_what_float32_gives():
    got = measured()["tiny_eikonal_relative"]
    print(f"tiny_normal, eikonal rows: measured relative {got}, recorded {R.TINY_EIKONAL_RELATIVE}")
    assert got <= R.TINY_EIKONAL_RELATIVE <= 2.0 * got


def test_the_configurations_that_count_have_sharp_bounds():
    """The kernel's d_sdf6 bound (KERNEL_FACTOR times the yardstick) is below 1e-4 at least where var is 0.35 or 0.6 and car is 0 or 0.3."""
    for var in (0.35, 0.6):
        for car in (0.0, 0.3):
            for eps in R.EPSS:
                assert R.KERNEL_FACTOR * R.YARDSTICK[R.grid_name(var, car, eps)][2] < 1e-4


if __name__ == "__main__":          # the child process of measured(): one JSON line
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    figures = {name: measure_yardstick(name) for name in R.CASES}
    figures["flat_relative"] = measure_flat_relative()
    figures["tiny_eikonal_relative"] = measure_tiny_eikonal_relative()
    print(json.dumps(figures))
