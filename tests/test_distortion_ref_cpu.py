"""CPU: the statements of the distortion loss agree with each other -- the fp32 O(n) restatement and the torch statement behind
losses.distortion_loss (its CPU branch) against the float64 O(n^2) definition of tests/distortion_ref.py -- and with values worked out by
hand."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import distortion_ref as R   # noqa: E402


def _one_ray(w, t, dt, near, far):
    f = lambda a: torch.tensor(a, dtype=torch.float32)
    return f(w), torch.stack([f(t), f(dt)], 1), torch.tensor([[0, len(w)]], dtype=torch.int32), f([near]), f([far])


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("space", R.SPACES)
def test_fp32_restatement_agrees_with_the_float64_model(kind, space):
    """fp32 against float64.  A sequential fp32 sum of n terms errs by at most n eps times the sum of their absolute values, eps = 2^-24;
    here n <= 1024 and that sum is at most 4/3 for the loss (weights sum to at most 1, |m_i - m_j| <= 1), and the rounding of the
    per-sample coordinates doubles it at most: 1024 * 2^-24 * 4/3 * 2 = 1.6e-4.  The gradient's sums are bounded the same way relative
    to their own scale.  A worst-case bound: the measured figures (printed) are two to three orders below it."""
    ref_loss, ref_mean, ref_grad = R.reference(kind, space)
    loss_ray, grad = R.restatement_f32(*R.case(kind), space=space)
    el, eg = R.loss_error(loss_ray, ref_loss), R.grad_error(grad, ref_grad, R.case(kind)[2])
    print(f"{kind} / {space}: loss error {el:.3g}, gradient error {eg:.3g}, mean loss {float(ref_mean):.6g}")
    assert el <= 1.6e-4 and eg <= 1.6e-4
    assert float(ref_loss.max()) <= 1 + 1 / 3
    if kind == "zeros":
        assert float(ref_loss.abs().max()) == 0 and float(ref_grad.abs().max()) == 0
    else:
        assert float(ref_loss.max()) > 0


def test_yardstick_is_positive_and_small():
    y = R.yardstick()
    print("yardstick (fp32 O(n) restatement vs float64 O(n^2) model):", y)
    assert 0 < y["loss"] < 1e-5 and 0 < y["grad"] < 1e-4
    assert y["per_kind"]["zeros"] == (0.0, 0.0)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("space", R.SPACES)
def test_cpu_branch_of_distortion_loss_equals_the_model(kind, space):
    """The torch statement works in float64 and returns float32: the loss agrees to float32 rounding of the result (2^-24 relative, here
    absolute on values <= 4/3), the float32 gradient likewise relative to the ray's largest."""
    from nerf2mesh_amd.losses import distortion_loss
    weights, ts, rays, nears, fars = R.case(kind)
    ref_loss, ref_mean, ref_grad = R.reference(kind, space, 1024.0)
    w = weights.clone().requires_grad_(True)
    mean, loss_ray = distortion_loss(w, ts, rays, nears, fars, space=space, return_per_ray=True)
    assert mean.dtype == torch.float32 and loss_ray.shape == (len(R.COUNTS),)
    only_mean = distortion_loss(weights, ts, rays, nears, fars, space=space)
    assert torch.equal(only_mean, mean.detach())
    (loss_ray * 1024.0).sum().backward()
    assert R.loss_error(loss_ray.detach(), ref_loss) <= 2.0 ** -23
    assert abs(float(mean.detach()) - float(ref_mean)) <= 2.0 ** -22
    assert R.grad_error(w.grad, ref_grad, rays) <= 2.0 ** -22
    assert float(loss_ray[8]) == 0 and float(loss_ray[11]) == 0                      # the rays without samples


def test_cpu_branch_untiled_ranges_and_degenerate_rays():
    from nerf2mesh_amd.losses import distortion_loss
    weights, ts, rays, nears, fars = R.case("two_peaks", gap=5)
    tiled = R.case("two_peaks")
    w = weights.clone().requires_grad_(True)
    mean, loss_ray = distortion_loss(w, ts, rays, nears, fars, return_per_ray=True)
    assert torch.allclose(loss_ray.double(), R.reference("two_peaks", "linear")[0], atol=2.0 ** -23, rtol=0)
    mean.backward()
    owned = torch.zeros(weights.shape[0], dtype=torch.bool)
    for off, cnt in rays.tolist():
        owned[off:off + cnt] = True
    assert int((~owned).sum()) == 5 * sum(1 for c in R.COUNTS if c) and float(w.grad[~owned].abs().max()) == 0
    assert owned.sum() == tiled[0].shape[0]
    # far <= near: the ray contributes nothing, to the loss or to the gradient
    fars2 = fars.clone()
    fars2[9] = nears[9]
    w2 = weights.clone().requires_grad_(True)
    mean2, loss_ray2 = distortion_loss(w2, ts, rays, nears, fars2, return_per_ray=True)
    mean2.backward()
    off, cnt = rays[9].tolist()
    assert float(loss_ray2[9]) == 0 and float(w2.grad[off:off + cnt].abs().max()) == 0 and torch.equal(loss_ray2[:9], loss_ray.detach()[:9])
    ref = R.model_f64(weights, ts, rays, nears, fars2)
    assert float(ref[0][9]) == 0 and float(ref[2][off:off + cnt].abs().max()) == 0


def test_hand_one_sample():
    """One sample: L = w^2 delta / 3.  near 1, far 3, [t - dt, t] = [1.5, 2]: linear delta = 0.25."""
    from nerf2mesh_amd.losses import distortion_loss
    case = _one_ray([0.8], [2.0], [0.5], 1.0, 3.0)
    want = 0.8 ** 2 * 0.25 / 3
    assert abs(float(R.model_f64(*case)[0][0]) - want) < 1e-7                         # (0.8 as float32)
    assert abs(float(distortion_loss(*case)) - want) < 1e-7
    assert abs(float(R.restatement_f32(*case)[0][0]) - want) < 1e-7
    w = case[0].clone().requires_grad_(True)
    distortion_loss(w, *case[1:]).backward()
    assert abs(float(w.grad[0]) - 2 * 0.8 * 0.25 / 3) < 1e-6


def test_hand_two_samples_linear():
    """near 0, far 4; intervals [0, 1] and [2, 4]: s = t / 4, m = (0.125, 0.75), delta = (0.25, 0.5); w = (0.5, 0.25).
    L = 2 w0 w1 |m0 - m1| + (w0^2 d0 + w1^2 d1) / 3 = 2 * 0.125 * 0.625 + (0.0625 + 0.03125) / 3 = 0.15625 + 0.03125 = 0.1875.
    dL/dw0 = 2 w1 |m0 - m1| + 2 w0 d0 / 3 = 0.3125 + 0.25 / 3;  dL/dw1 = 2 w0 |m0 - m1| + 2 w1 d1 / 3 = 0.625 + 0.25 / 3."""
    from nerf2mesh_amd.losses import distortion_loss
    case = _one_ray([0.5, 0.25], [1.0, 4.0], [1.0, 2.0], 0.0, 4.0)
    loss_ray, _, grad = R.model_f64(*case)
    assert abs(float(loss_ray[0]) - 0.1875) < 1e-12
    assert abs(float(grad[0]) - (0.3125 + 0.25 / 3)) < 1e-12 and abs(float(grad[1]) - (0.625 + 0.25 / 3)) < 1e-12
    w = case[0].clone().requires_grad_(True)
    loss = distortion_loss(w, *case[1:])
    loss.backward()
    assert abs(float(loss) - 0.1875) < 1e-7 and abs(float(w.grad[0]) - (0.3125 + 0.25 / 3)) < 1e-6
    f32_loss, f32_grad = R.restatement_f32(*case)
    assert abs(float(f32_loss[0]) - 0.1875) < 1e-7 and abs(float(f32_grad[1]) - (0.625 + 0.25 / 3)) < 1e-6


def test_hand_all_weight_in_one_sample():
    """All the weight in one sample of several: the pair sum vanishes (every product w_i w_j with i != j holds a zero) and L is the
    intra-interval term of that sample alone."""
    from nerf2mesh_amd.losses import distortion_loss
    case = _one_ray([0.0, 0.0, 1.0, 0.0], [1.0, 2.0, 3.0, 4.0], [0.5, 0.5, 1.0, 0.5], 0.0, 4.0)
    want = 1.0 * 0.25 / 3                                                             # [2, 3] / 4: delta = 0.25
    assert abs(float(R.model_f64(*case)[0][0]) - want) < 1e-12
    assert abs(float(distortion_loss(*case)) - want) < 1e-7
    assert abs(float(R.restatement_f32(*case)[0][0]) - want) < 1e-7


def test_hand_disparity_differs_from_linear():
    """near 1, far 4, intervals [1, 2] and [2, 4], w = (0.75, 0.25).  Linear: s = (t - 1) / 3, m = (1/6, 2/3), delta = (1/3, 2/3).
    Disparity: s = (1/t - 1) / (1/4 - 1) = (4/3)(1 - 1/t), so s(1) = 0, s(2) = 2/3, s(4) = 1, m = (1/3, 5/6), delta = (2/3, 1/3).
    |m_0 - m_1| = 1/2 in both, so the pair term is 2 * 0.1875 * 0.5 in both; the interval terms differ:
    (0.5625 / 3 + 0.0625 * 2 / 3) / 3 against (0.5625 * 2 / 3 + 0.0625 / 3) / 3."""
    from nerf2mesh_amd.losses import distortion_loss
    case = _one_ray([0.75, 0.25], [2.0, 4.0], [1.0, 2.0], 1.0, 4.0)
    lin = 2 * 0.1875 * 0.5 + (0.5625 / 3 + 0.0625 * 2 / 3) / 3
    disp = 2 * 0.1875 * 0.5 + (0.5625 * 2 / 3 + 0.0625 / 3) / 3
    assert abs(lin - disp) > 0.03
    for space, want in (("linear", lin), ("disparity", disp)):
        assert abs(float(R.model_f64(*case, space=space)[0][0]) - want) < 1e-12
        assert abs(float(distortion_loss(*case, space=space)) - want) < 1e-7
        assert abs(float(R.restatement_f32(*case, space=space)[0][0]) - want) < 2e-7


def test_python_layer_refuses_bad_arguments():
    from nerf2mesh_amd.losses import distortion_loss
    weights, ts, rays, nears, fars = R.case("random")
    with pytest.raises(ValueError, match="space must be one of"):
        distortion_loss(weights, ts, rays, nears, fars, space="log")
    with pytest.raises(ValueError, match="expected weights"):
        distortion_loss(weights[:-1], ts, rays, nears, fars)
    with pytest.raises(ValueError, match="expected weights"):
        distortion_loss(weights, ts, rays, nears[:-1], fars)
    with pytest.raises(ValueError, match="expected weights"):
        distortion_loss(weights, ts.reshape(-1), rays, nears, fars)
