"""GPU: the batched patch SSIM (n2m_ssim_patches_forward / n2m_ssim_patches_backward, csrc/metrics.hip) through metrics.ssim_patches
against the float64 model of tests/ssim_ref.py applied per patch.

Case set: P in {11, 16, 27, 32, 33, 64} -- one window; the common sizes; both sides of the kernel's tier boundaries (P <= 16, P <= 32,
above: banded) --, C in {1, 3}, B in {1, 3, 17}, the five input kinds of ssim_ref.INPUTS (a different seed per patch), gradient seeds 1
and 1024.  The model sees the B patches as B * C channels of one P x P image: channels never mix in it, so that IS the model per patch,
in one call per (P, C, kind); the reference for a smaller B is its first B patches.

Measures and bound are those of tests/test_ssim_gpu.py: |mean - ref| for every per-patch mean and for the global mean,
max |grad - ref| / max |ref grad| per patch (y = x normalised by the same x against noise), each held to 4 x the largest error of
ssim_ref.yardstick() -- the fp32 model against the float64 model, computed on every run.  The arithmetic per window is the frame
kernel's 121-term fmaf sum and a mean over more windows only averages, which is why the frame rule carries over.  Measured on MI355X:
DESIGN.md 4.27 has the table per input kind."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ssim_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu

FACTOR = 4.0
SIZES = [11, 16, 27, 32, 33, 64]
BATCHES = [1, 3, 17]
SEEDS = [1.0, 1024.0]
BMAX = max(BATCHES)


@pytest.fixture(scope="module")
def bound():
    y = R.yardstick()
    print(f"yardstick (fp32 model against float64 model), largest over its case set: mean {y['mean']:.3g}, gradient {y['grad']:.3g}")
    assert y["mean"] > 0 and y["grad"] > 0
    return {k: FACTOR * v for k, v in y.items()}


_REF = {}


def reference(P, C, kind):
    """BMAX patches of one kind with their float64 per-patch means and per-patch gradients of the patch's OWN mean, computed once."""
    import torch
    key = (P, C, kind)
    if key not in _REF:
        pairs = [R.make_pair((P, P), C, kind, seed=b) for b in range(BMAX)]
        x, y = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])               # [B, P, P, C]
        as_channels = lambda t: t.permute(1, 2, 0, 3).reshape(P, P, BMAX * C)
        xr = as_channels(x).double().requires_grad_(True)
        _, smap = R.ssim_model(xr, as_channels(y))
        means = smap.view(P - 10, P - 10, BMAX, C).mean(dim=(0, 1, 3))                               # [B]
        (grad,) = torch.autograd.grad(means.sum(), xr)
        grad = grad.view(P, P, BMAX, C).permute(2, 0, 1, 3).contiguous()                             # [B, P, P, C]: d mean_b / d x_b
        norm = reference(P, C, "random")["norm"] if kind == "same" else grad.abs().amax(dim=(1, 2, 3))
        _REF[key] = dict(x=x, y=y, means=means.detach(), grad=grad, norm=norm)
    return _REF[key]


def _run(x, y, g):
    from nerf2mesh_amd.metrics import ssim_patches
    xg = x.cuda().requires_grad_()
    mean, pp = ssim_patches(xg, y.cuda(), return_per_patch=True)
    (mean * g).backward()
    return mean.detach().clone(), pp.clone(), xg.grad.clone()


@pytest.mark.parametrize("C", R.CHANNELS)
@pytest.mark.parametrize("P", SIZES)
def test_forward_and_backward_against_the_float64_model_per_patch(bound, P, C):
    import torch
    for kind in R.INPUTS:
        ref = reference(P, C, kind)
        worst = {"patch": 0.0, "mean": 0.0, "grad": 0.0}
        for B in BATCHES:
            want_mean = float(ref["means"][:B].mean())
            for g in SEEDS:
                mean, pp, grad = _run(ref["x"][:B], ref["y"][:B], g)
                assert mean.shape == () and pp.shape == (B,) and grad.shape == (B, P, P, C) and not pp.requires_grad
                assert bool(torch.isfinite(grad).all())
                e_patch = float((pp.cpu().double() - ref["means"][:B]).abs().max())
                e_mean = abs(float(mean) - want_mean)
                per = (grad.cpu().double() * (B / g) - ref["grad"][:B]).abs().amax(dim=(1, 2, 3)) / ref["norm"][:B]
                e_grad = float(per.max())
                worst = {"patch": max(worst["patch"], e_patch), "mean": max(worst["mean"], e_mean), "grad": max(worst["grad"], e_grad)}
                assert e_patch <= bound["mean"], (kind, B, g, e_patch, bound["mean"])
                assert e_mean <= bound["mean"], (kind, B, g, e_mean, bound["mean"])
                assert e_grad <= bound["grad"], (kind, B, g, e_grad, bound["grad"])
        print(f"P={P} C={C} {kind:15s} worst over B, g: per-patch mean {worst['patch']:.3g}  global mean {worst['mean']:.3g}  "
              f"gradient {worst['grad']:.3g}   (bounds {bound['mean']:.3g}, {bound['grad']:.3g})")


@pytest.mark.parametrize("P", [16, 64])
def test_a_patch_does_not_see_the_other_patches(P):
    """Changing patch 1 of x and y leaves per_patch[b] and the gradient rows of patch b the same bits for b = 0, 2."""
    import torch
    ref = reference(P, 3, "random")
    x, y = ref["x"][:3].clone(), ref["y"][:3].clone()
    mean_a, pp_a, grad_a = _run(x, y, 1024.0)
    other = reference(P, 3, "inverse")
    x[1], y[1] = other["x"][5], other["y"][5]
    mean_b, pp_b, grad_b = _run(x, y, 1024.0)
    for b in (0, 2):
        assert torch.equal(pp_a[b], pp_b[b]) and torch.equal(grad_a[b], grad_b[b]), b
    assert not torch.equal(pp_a[1], pp_b[1]) and not torch.equal(grad_a[1], grad_b[1]) and not torch.equal(mean_a, mean_b)


@pytest.mark.parametrize("P,B", [(16, 17), (27, 3), (64, 3)])
def test_two_calls_give_identical_bits(P, B):
    import torch
    ref = reference(P, 3, "random")
    a, b = _run(ref["x"][:B], ref["y"][:B], 1024.0), _run(ref["x"][:B], ref["y"][:B], 1024.0)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_one_patch_agrees_with_the_frame_kernel(bound):
    """B = 1, P = H = W = 32: the frame entry point on the same image, within twice the bound (each is within the bound of the model)."""
    from nerf2mesh_amd.metrics import ssim
    ref = reference(32, 3, "random")
    mean, pp, grad = _run(ref["x"][:1], ref["y"][:1], 1.0)
    xf = ref["x"][0].cuda().requires_grad_()
    frame = ssim(xf, ref["y"][0].cuda())
    frame.backward()
    frame = frame.detach()
    assert abs(float(mean) - float(frame)) <= 2 * bound["mean"] and abs(float(pp[0]) - float(frame)) <= 2 * bound["mean"]
    e = float((grad[0] - xf.grad).abs().max()) / float(ref["norm"][0])
    print(f"patch kernel {float(mean):.8f}, frame kernel {float(frame):.8f}; gradient difference / max |ref grad| {e:.3g}")
    assert e <= 2 * bound["grad"]


def test_no_grad_path_and_views():
    """Without a gradient request no derivative maps are written and the mean is the same bits; a non-contiguous view is accepted."""
    import torch
    from nerf2mesh_amd.metrics import ssim_patches
    ref = reference(27, 3, "random")
    x, y = ref["x"][:3].cuda(), ref["y"][:3].cuda()
    a = ssim_patches(x, y)
    assert a.shape == () and a.dtype == torch.float32 and not a.requires_grad
    d, pp = ssim_patches(x.clone().requires_grad_(), y, return_per_patch=True)
    assert d.requires_grad and torch.equal(d.detach(), a) and not pp.requires_grad
    flat = x.reshape(3 * 27 * 27, 3)                                                     # the layout of a patch batch's image [N, 3]
    assert torch.equal(ssim_patches(flat.view(3, 27, 27, 3), y), a)
    wide = torch.zeros(3, 27, 27, 4, device="cuda")
    wide[..., :3] = x
    assert torch.equal(ssim_patches(wide[..., :3], y), a)
    # the global mean is the mean of the per-patch means (equal window counts), up to the rounding of another summation order
    assert abs(float(a) - float(pp.double().mean())) <= 4 * 2.0 ** -24


def test_refused_shapes_and_host_tensors():
    import torch
    from nerf2mesh_amd import _lib as L
    from nerf2mesh_amd.metrics import _TAPS, ssim_patches
    z = lambda *s: torch.zeros(*s, device="cuda")
    for P in (10, 65):
        with pytest.raises(ValueError, match="P must be 11 .. 64"):
            ssim_patches(z(2, P, P, 3), z(2, P, P, 3))
    with pytest.raises(ValueError, match="C must be 1 or 3"):
        ssim_patches(z(2, 16, 16, 2), z(2, 16, 16, 2))
    with pytest.raises(ValueError, match="B must be at least 1"):
        ssim_patches(z(0, 16, 16, 3), z(0, 16, 16, 3))
    with pytest.raises(ValueError, match="one shape"):
        ssim_patches(z(2, 16, 16, 3), z(3, 16, 16, 3))
    with pytest.raises(ValueError, match="one shape"):
        ssim_patches(z(2, 16, 17, 3), z(2, 16, 17, 3))
    with pytest.raises(RuntimeError, match="CUDA tensors"):
        ssim_patches(torch.zeros(2, 16, 16, 3), torch.zeros(2, 16, 16, 3))
    with pytest.raises(RuntimeError, match="CUDA tensors"):
        ssim_patches(z(2, 16, 16, 3), torch.zeros(2, 16, 16, 3))
    # the ABI refuses the same on its own, before any launch (16: a stand-in for a device pointer)
    with pytest.raises(RuntimeError, match=r"failed \(-1\).*P must be 11 .. 64"):
        L.call("n2m_ssim_patches_forward", 16, 16, 2, 10, 3, _TAPS, None, 16, 16, 16, None)
    with pytest.raises(RuntimeError, match=r"failed \(-1\).*B must be"):
        L.call("n2m_ssim_patches_backward", 16, 16, 16, 0, 16, 3, _TAPS, 16, 16, None)
    with pytest.raises(RuntimeError, match=r"failed \(-2\).*NULL"):
        L.call("n2m_ssim_patches_forward", 16, 16, 2, 16, 3, _TAPS, None, 16, None, 16, None)
