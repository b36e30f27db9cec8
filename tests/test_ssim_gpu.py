"""GPU: the SSIM kernels (n2m_ssim_forward / n2m_ssim_backward, csrc/metrics.hip) through metrics.ssim against the float64 model of
tests/ssim_ref.py.

Case set (tests/ssim_ref.py): shapes 11 x 11 (one window), 11 x 43 and 43 x 11 (one row / one column of windows), 42 x 75 and 76 x 43 (maps of
32 x 65 and 66 x 33: one and two past the 32 x 16 tile and its multiples), each for C = 1 and 3, each with five seeded input pairs: uniform
noise against noise, y = x, y = 1 - x, a constant image against noise, two constant images.

Error measures: |mean - ref|, max |map - ref|, and for the gradient max |grad - ref| / max |ref grad| per image (y = x, whose true gradient
is identically zero, is normalised by the gradient scale of the same x against noise; the gradient seeded with g is compared with g x the
reference).  Tolerance: the yardstick -- the same model evaluated in fp32 -- is measured against the float64 model with the same measures,
and the kernel is held to 4 x the LARGEST yardstick error over the whole case set (the factor covers a different summation order in a
121-term sum).  Measured, yardstick (this is computed, not stored: the test derives its bound on every run):
    mean 1.02e-04, map 1.02e-04 (both from the two-constant-images case, where s_x^2 = E[x^2] - mu_x^2 cancels to rounding noise against
    C2 = 9e-4; 1.0e-05 without that kind), gradient 6.6e-04 (same case; 3.3e-05 without it)
and the kernels on an MI355X, largest over the case set: mean 4.19e-05, map 4.19e-05, gradient 2.58e-04 (the same case; without it
    mean 4.8e-07, map 2.5e-06, gradient 2.1e-05) -- in every input kind but y = x closer to float64 than the fp32 model is.  DESIGN.md 4.25
    has the table per input kind."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ssim_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu

FACTOR = 4.0
SEEDS = [1.0, 1024.0]          # 1024: a loss-scale-sized upstream gradient


@pytest.fixture(scope="module")
def bound():
    y = R.yardstick()
    print(f"yardstick (fp32 model against float64 model), largest over the case set: mean {y['mean']:.3g}, map {y['map']:.3g}, "
          f"gradient {y['grad']:.3g}")
    assert y["mean"] > 0 and y["map"] > 0 and y["grad"] > 0
    return {k: FACTOR * v for k, v in y.items()}


def _run(c, g):
    from nerf2mesh_amd.metrics import ssim
    x = c["x"].cuda().requires_grad_()
    mean, smap = ssim(x, c["y"].cuda(), return_map=True)
    (mean * g).backward()
    return mean.detach().clone(), smap.clone(), x.grad.clone()


@pytest.mark.parametrize("C", R.CHANNELS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_forward_and_backward_against_the_float64_model(bound, shape, C):
    """Mean, per-window map and gradient (g = 1 and g = 1024) of every input kind within 4 x the yardstick's largest error."""
    import torch
    worst = {"mean": 0.0, "map": 0.0, "grad": 0.0}
    for kind in R.INPUTS:
        c = R.case(shape, C, kind)
        for g in SEEDS:
            mean, smap, grad = _run(c, g)
            assert tuple(smap.shape) == (shape[0] - 10, shape[1] - 10, C) and grad.shape == c["x"].shape
            e_mean, e_map = R.forward_error(mean.cpu(), smap.cpu(), c["mean"], c["map"])
            e_grad = R.grad_error(grad.cpu() / g, c["grad"], c["grad_norm"])
            print(f"{shape[0]}x{shape[1]}x{C} {kind:15s} g={g:6g}: ssim {float(mean):+.6f}  |mean err| {e_mean:.3g} (yardstick {c['yard_mean']:.3g})  "
                  f"map {e_map:.3g} ({c['yard_map']:.3g})  gradient {e_grad:.3g} ({c['yard_grad']:.3g})")
            worst = {"mean": max(worst["mean"], e_mean), "map": max(worst["map"], e_map), "grad": max(worst["grad"], e_grad)}
            assert bool(torch.isfinite(grad).all())
            assert e_mean <= bound["mean"], (kind, g, e_mean, bound["mean"])
            assert e_map <= bound["map"], (kind, g, e_map, bound["map"])
            assert e_grad <= bound["grad"], (kind, g, e_grad, bound["grad"])
    print(f"{shape[0]}x{shape[1]}x{C} worst: mean {worst['mean']:.3g}  map {worst['map']:.3g}  gradient {worst['grad']:.3g}")


@pytest.mark.parametrize("C", R.CHANNELS)
def test_two_calls_give_identical_bits(C):
    """Mean, map and gradient of two calls on one input are the same bits (fixed-order reduction, gather backward: no float atomics)."""
    import torch
    c = R.case((76, 43), C, "random")
    a, b = _run(c, 1024.0), _run(c, 1024.0)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_flat_images_and_no_grad_path():
    """[H * W, C] with hw=(H, W) is the same call; without a gradient request nothing is saved and the value is the same bits."""
    import torch
    from nerf2mesh_amd.metrics import ssim
    c = R.case((42, 75), 3, "random")
    x, y = c["x"].cuda(), c["y"].cuda()
    a = ssim(x, y)
    b = ssim(x.view(-1, 3), y.view(-1, 3), hw=(42, 75))
    assert a.shape == () and a.dtype == torch.float32 and torch.equal(a, b) and not a.requires_grad
    xr = x.clone().requires_grad_()
    d = ssim(xr, y)
    assert d.requires_grad and torch.equal(d.detach(), a)
    m, smap = ssim(x, y, return_map=True)
    assert torch.equal(m, a) and not smap.requires_grad
    # the mean is the mean of the map it wrote (another summation order: a few ulp of a value of order 1e-2 .. 1)
    assert abs(float(m) - float(smap.double().mean())) <= 4 * 2.0 ** -24


def test_refused_shapes_and_host_tensors():
    """Refused on the host, before any launch: H or W below 11, C outside {1, 3}, mismatched shapes (ValueError); CPU tensors (RuntimeError)."""
    import torch
    from nerf2mesh_amd import _lib as L
    from nerf2mesh_amd.metrics import ssim
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(ValueError, match="at least 11"):
        ssim(z(10, 11, 3), z(10, 11, 3))
    with pytest.raises(ValueError, match="at least 11"):
        ssim(z(11, 10, 1), z(11, 10, 1))
    with pytest.raises(ValueError, match="C must be 1 or 3"):
        ssim(z(11, 11, 2), z(11, 11, 2))
    with pytest.raises(ValueError, match="one shape"):
        ssim(z(11, 11, 3), z(11, 12, 3))
    with pytest.raises(ValueError, match="hw="):
        ssim(z(120, 3), z(120, 3), hw=(11, 11))
    with pytest.raises(RuntimeError, match="CUDA tensors"):
        ssim(torch.zeros(11, 11, 3), torch.zeros(11, 11, 3))
    with pytest.raises(RuntimeError, match="CUDA tensors"):
        ssim(z(11, 11, 3), torch.zeros(11, 11, 3))
    # the ABI refuses the same on its own (N2M_EINVAL / N2M_ENULL through N2M_REQUIRE), also before any launch
    from nerf2mesh_amd.metrics import _TAPS
    with pytest.raises(RuntimeError, match=r"failed \(-1\).*at least 11"):
        L.call("n2m_ssim_forward", 16, 16, 10, 11, 3, _TAPS, None, None, 16, 16, None)
    with pytest.raises(RuntimeError, match=r"failed \(-1\).*C must be 1 or 3"):
        L.call("n2m_ssim_backward", 16, 16, 16, 11, 11, 2, _TAPS, 16, 16, None)
    with pytest.raises(RuntimeError, match=r"failed \(-2\).*NULL"):
        L.call("n2m_ssim_forward", 16, None, 11, 11, 3, _TAPS, None, None, 16, 16, None)
    with pytest.raises(RuntimeError, match=r"failed \(-2\).*NULL"):
        L.call("n2m_ssim_backward", 16, 16, None, 11, 11, 3, _TAPS, 16, 16, None)
