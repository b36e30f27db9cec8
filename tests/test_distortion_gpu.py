"""GPU: n2m_distortion_forward / _backward through losses.distortion_loss against the float64 O(n^2) definition of tests/distortion_ref.py.

Cases: per-ray sample counts 1, 2, 63, 64, 65, 127, 128, 129, 0, 1024, 3, 0 (both sides of every 64-sample chunk boundary, empty rays inside
and at the end, the longest ray the marcher emits, three workgroups of four waves with the last one partly filled), every weight kind, both
spaces, and the incoming gradients 1 and 1024 (a loss scale's size).

Bound (the rule of tests/test_ssim_gpu.py): 4 x the largest error the fp32 O(n) restatement with SEQUENTIAL running sums shows
against the float64 model over the same case set, computed on every run -- absolute for the per-ray loss (L_ray <= 1 + 1/3), max |grad - ref| /
max |ref grad| per ray for the gradient.  The factor 4 covers the wave scan associating its sums as a tree.  The mean over the 12 rays is
allowed the per-ray bound (the mean of errors is at most their largest) plus the rounding of one fp32 sum of 12 values <= 4/3 and its
division: 13 * 2^-24 * 4/3."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import distortion_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bound():
    y = R.yardstick()
    b = {"loss": 4.0 * y["loss"], "grad": 4.0 * y["grad"]}
    print(f"yardstick: fp32 sequential restatement vs float64 model: loss {y['loss']:.3g} (absolute), gradient {y['grad']:.3g} (relative per ray); "
          f"per kind {y['per_kind']}; bounds {b}")
    assert b["loss"] > 0 and b["grad"] > 0
    return b


def _run(case, space, seed=1.0, tiled=True):
    """(mean, loss_ray, grad_weights) of the device path, on the host."""
    import torch
    from nerf2mesh_amd.losses import distortion_loss
    weights, ts, rays, nears, fars = (t.cuda() for t in case)
    w = weights.clone().requires_grad_(True)
    mean, loss_ray = distortion_loss(w, ts, rays, nears, fars, space=space, rays_tile_samples=tiled, return_per_ray=True)
    (loss_ray * seed).sum().backward()
    torch.cuda.synchronize()
    return mean.detach().cpu(), loss_ray.detach().cpu(), w.grad.cpu()


@pytest.mark.parametrize("seed", R.SEEDS)
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("space", R.SPACES)
def test_kernels_against_the_float64_model(bound, space, kind, seed):
    import torch
    ref_loss, ref_mean, ref_grad = R.reference(kind, space, seed)
    mean, loss_ray, grad = _run(R.case(kind), space, seed)
    el, eg, em = R.loss_error(loss_ray, ref_loss), R.grad_error(grad, ref_grad, R.case(kind)[2]), abs(float(mean) - float(ref_mean))
    print(f"{kind} / {space} / seed {seed:g}: loss error {el:.3g} (bound {bound['loss']:.3g}), gradient error {eg:.3g} (bound {bound['grad']:.3g}), "
          f"mean {float(mean):.7g} vs {float(ref_mean):.7g} (error {em:.3g})")
    assert loss_ray.dtype == torch.float32 and loss_ray.shape == (len(R.COUNTS),) and grad.shape == R.case(kind)[0].shape
    assert bool(torch.isfinite(loss_ray).all()) and bool(torch.isfinite(grad).all())
    assert float(loss_ray[8]) == 0 and float(loss_ray[11]) == 0                      # the rays without samples are written, with zeros
    assert el <= bound["loss"]
    assert eg <= bound["grad"]
    assert em <= bound["loss"] + 13 * 2.0 ** -24 * 4 / 3
    if kind == "zeros":
        assert float(loss_ray.abs().max()) == 0 and float(grad.abs().max()) == 0


def test_mean_backward_is_the_per_ray_gradient_over_n(bound):
    """The mean output's gradient: grad_ray = 1 / N for every ray (a power of two would make it exact; N = 12 is not, so the same bound)."""
    import torch
    from nerf2mesh_amd.losses import distortion_loss
    weights, ts, rays, nears, fars = (t.cuda() for t in R.case("two_peaks"))
    w = weights.clone().requires_grad_(True)
    distortion_loss(w, ts, rays, nears, fars, rays_tile_samples=True).backward()
    ref_grad = R.reference("two_peaks", "linear")[2] / len(R.COUNTS)
    assert R.grad_error(w.grad.cpu(), ref_grad, R.case("two_peaks")[2]) <= bound["grad"] + 2.0 ** -23


@pytest.mark.parametrize("space", R.SPACES)
def test_two_calls_give_identical_bits(space):
    import torch
    a, b = _run(R.case("random"), space, 1024.0), _run(R.case("random"), space, 1024.0)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("space", R.SPACES)
def test_untiled_ranges(space):
    """Five rows no ray owns in front of every ray: with rays_tile_samples=False their gradient is exactly zero, and the owned rows hold
    the bits of the tiled call."""
    import torch
    tiled, gapped = R.case("two_peaks"), R.case("two_peaks", gap=5)
    mean_t, loss_t, grad_t = _run(tiled, space, 1024.0, tiled=True)
    mean_g, loss_g, grad_g = _run(gapped, space, 1024.0, tiled=False)
    owned = torch.zeros(gapped[0].shape[0], dtype=torch.bool)
    for off, cnt in gapped[2].tolist():
        owned[off:off + cnt] = True
    assert int((~owned).sum()) == 5 * sum(1 for c in R.COUNTS if c)
    assert float(grad_g[~owned].abs().max()) == 0
    assert torch.equal(grad_g[owned], grad_t) and torch.equal(loss_g, loss_t) and torch.equal(mean_g, mean_t)


def test_degenerate_and_cut_off_rays_contribute_nothing(bound):
    """far <= near: 0 loss, 0 gradient over the ray's rows (written, not left), the other rays unchanged bit for bit.  A ray whose range
    runs past M is treated the same way (the compositing kernels skip it too)."""
    import torch
    weights, ts, rays, nears, fars = R.case("random")
    base = _run((weights, ts, rays, nears, fars), "linear", 1.0)
    fars2 = fars.clone()
    fars2[9] = nears[9]
    mean, loss_ray, grad = _run((weights, ts, rays, nears, fars2), "linear", 1.0)
    off, cnt = rays[9].tolist()
    assert float(loss_ray[9]) == 0 and float(grad[off:off + cnt].abs().max()) == 0
    keep = torch.ones(weights.shape[0], dtype=torch.bool)
    keep[off:off + cnt] = False
    assert torch.equal(grad[keep], base[2][keep]) and torch.equal(loss_ray[:9], base[1][:9]) and torch.equal(loss_ray[10:], base[1][10:])
    rays2 = rays.clone()
    rays2[10, 1] += 7                                                                # the last ray with samples now ends behind M
    mean, loss_ray, grad = _run((weights, ts, rays2, nears, fars), "linear", 1.0)
    off, cnt = rays[10].tolist()
    assert float(loss_ray[10]) == 0 and float(grad[off:].abs().max()) == 0 and torch.equal(grad[:off], base[2][:off])


def test_real_marcher_output(bound):
    """256 rays of the synthetic lego scene through model.render in training mode after one occupancy refresh (a Stage0Trainer's own
    preparation: refresh, batch, march): distortion_loss on the render's weights / ts / rays / nears / fars against the float64 model,
    both spaces, under the same bound.  At least half of the 256 rays must carry samples -- a condition on the set-up, checked."""
    import torch
    from nerf2mesh_amd import synthetic
    from nerf2mesh_amd.losses import distortion_loss
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    from nerf2mesh_amd.trainer import Stage0Trainer
    torch.manual_seed(0)
    opt = make_options(O=True, bound=1, dt_gamma=0, iters=30000, fused_mlp=True, num_rays=256)
    tr = Stage0Trainer(NeRFNetwork(opt), opt, synthetic.make_cameras(8, seed=0), torch.device("cuda", 0), seed=0)
    tr.mark_untrained()
    rays_o, rays_d, images, ticket, bg, noises = tr._prepare()
    tr.model.train()
    out = tr.model.render(rays_o, rays_d, bg_color=bg, perturb=True, shading="diffuse", dt_gamma=opt.dt_gamma, max_steps=opt.max_steps,
                          ticket=ticket, blend_bg=False)
    weights, ts, rays, nears, fars = (out[k].detach() for k in ("weights", "ts", "rays", "nears", "fars"))
    M, N = weights.shape[0], rays.shape[0]
    with_samples = int((rays[:, 1] > 0).sum())
    print(f"real batch: {N} rays, {with_samples} with samples, {M} samples, longest ray {int(rays[:, 1].max())}")
    assert N == 256 and ts.shape == (M, 2) and nears.shape == fars.shape == (N,) and M == out["num_points"]
    assert with_samples >= N // 2, f"only {with_samples} of {N} rays carry samples: the scene set-up no longer marches real rays"
    assert int(rays[:, 1].sum()) == M and bool((fars[rays[:, 1] > 0] > nears[rays[:, 1] > 0]).all())
    # the intervals lie inside the ray's [near, far] (to the marcher's own rounding): the normalised coordinate is in [0, 1]
    first = rays[rays[:, 1] > 0, 0].long()
    assert bool((ts[first, 0] - ts[first, 1] >= nears[rays[:, 1] > 0] * (1 - 1e-5)).all())
    for space in R.SPACES:
        w = weights.clone().requires_grad_(True)
        mean, loss_ray = distortion_loss(w, ts, rays, nears, fars, space=space, rays_tile_samples=True, return_per_ray=True)
        mean.backward()
        ref_loss, ref_mean, ref_grad = R.model_f64(weights, ts, rays, nears, fars, space=space, grad_ray=1.0 / N)
        el, eg = R.loss_error(loss_ray.detach().cpu(), ref_loss), R.grad_error(w.grad.cpu(), ref_grad, rays.cpu())
        print(f"real batch / {space}: mean {float(mean):.6g} vs {float(ref_mean):.6g}, loss error {el:.3g}, gradient error {eg:.3g}")
        assert float(ref_mean) > 0
        # (the mean: the per-ray bound plus a tree sum of 256 values <= 4/3, eight levels, and its division)
        assert el <= bound["loss"] and eg <= bound["grad"] and abs(float(mean) - float(ref_mean)) <= bound["loss"] + 9 * 2.0 ** -24 * 4 / 3
