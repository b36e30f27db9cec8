"""CPU: the float64 model of the pose-refinement gradient (tests/pose_ref.py) against central finite differences of the function it
differentiates, the package's torch statement (pose_refine.attach_torch, pose_apply_torch) against the model, and three planted mistakes.

The function: delta -> sum_i <c_i, x_i(delta)> + <e_i, d(delta)> with x_i = o + t_i d over packed rays of several views, c and e random, the
sample depths fixed.  Its terms are O(1) and there are a few dozen of them, so |f| <~ 1e2: central differences at step 1e-6 carry
f''' step^2 ~ 1e-10 of truncation and eps |f| / step ~ 1e-8 of rounding.  The comparison allows 1e-6 of the gradient's largest entry (O(1)
to O(10)): a hundred times the finite differences' own error, five orders below the effect of any planted mistake."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pose_ref as R   # noqa: E402

NORMS = (0.0, 1e-9, 1e-4, 0.3, 2.5)
FD_TOL = 1e-6


@pytest.fixture(scope="module")
def case():
    return R.make_case(V=5, rays_per_view=3, samples=(0, 1, 5, 7), seed=3, norms=NORMS)


def test_the_case_covers_every_angle(case):
    assert np.allclose(np.linalg.norm(case["delta"][:, :3], axis=1), NORMS, rtol=1e-12, atol=0)
    assert sorted(set(case["rays"][:, 1].tolist())) == [0, 1, 5, 7] and case["rays"][:, 1].sum() == case["M"]


def test_series_and_closed_forms_agree():
    """The model's power series against Rodrigues' closed form where that is well conditioned."""
    for th in (0.3, 2.5):
        w = np.array([0.6, -0.48, 0.64]) * th
        K = R.skew(w)
        E = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
        J = np.eye(3) + (1 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * K @ K
        assert np.abs(R.rotation(w) - E).max() < 1e-14 and np.abs(R.left_jacobian(w) - J).max() < 1e-14
        assert np.abs(R.rotation(w) @ R.rotation(w).T - np.eye(3)).max() < 1e-14


def test_model_gradient_equals_finite_differences(case):
    g = R.model_gradient(case, case["delta"])
    fd = R.finite_differences(case, case["delta"])
    scale = np.abs(fd).max()
    err = np.abs(g - fd).max(axis=1) / scale
    print("per view (|omega| = %s): relative error %s" % (NORMS, err))
    assert scale > 0.1 and (err < FD_TOL).all()


@pytest.mark.parametrize("planted", ["no_jacobian", "no_t", "swap_cross"])
def test_planted_mistakes_are_caught(case, planted):
    """At |omega| = 0.3 (view 3): each mistake moves the rotational gradient by far more than the tolerance."""
    g = R.model_gradient(case, case["delta"], planted=planted)
    fd = R.finite_differences(case, case["delta"])
    err = np.abs(g[3] - fd[3]).max() / np.abs(fd).max()
    print(f"{planted}: relative error {err:.3g} at |omega| = 0.3")
    assert err > 1e4 * FD_TOL


def _tensors(case, delta):
    d = R.world_dirs(case, delta)
    t = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
    M = case["M"]
    xyzs = torch.zeros(M, 3, dtype=torch.float64)
    dirs = torch.zeros(M, 3, dtype=torch.float64)
    return dict(xyzs=xyzs, dirs=dirs, delta=t(delta).requires_grad_(True), ts=t(case["ts"]), rays=t(case["rays"], torch.int32), rays_d=t(d),
                view=t(case["view"], torch.int32), c=t(case["c"]), e=t(case["e"]))


def test_attach_torch_matches_the_model(case):
    from nerf2mesh_amd.pose_refine import attach_torch
    T = _tensors(case, case["delta"])
    x, d = attach_torch(T["xyzs"], T["dirs"], T["delta"], T["ts"], T["rays"], T["rays_d"], T["view"])
    assert torch.equal(x, T["xyzs"]) and torch.equal(d, T["dirs"]) and x.requires_grad and d.requires_grad
    ((x * T["c"]).sum() + (d * T["e"]).sum()).backward()
    want = R.model_gradient(case, case["delta"])
    got = T["delta"].grad.numpy()
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"attach_torch vs the model: {err:.3g}")
    assert err < 1e-12


def test_attach_torch_without_a_direction_gradient_and_with_one_view(case):
    from nerf2mesh_amd.pose_refine import attach_torch
    T = _tensors(case, case["delta"])
    x, _ = attach_torch(T["xyzs"], T["dirs"], T["delta"], T["ts"], T["rays"], T["rays_d"], 2)            # one integer: every ray is view 2's
    (x * T["c"]).sum().backward()
    r6, _ = R.ray_grad(case["c"], None, case["ts"], case["rays"], R.world_dirs(case, case["delta"]))
    want = R.view_grad(r6, np.full(case["N"], 2), case["delta"])[0]
    got = T["delta"].grad.numpy()
    assert np.abs(got - want).max() / np.abs(want).max() < 1e-12
    assert (got[[0, 1, 3, 4]] == 0).all()


def test_a_view_outside_the_table_is_skipped(case):
    from nerf2mesh_amd.pose_refine import pose_grad_torch
    T = _tensors(case, case["delta"])
    view = T["view"].clone()
    view[0], view[1] = -1, case["V"]
    got = pose_grad_torch(T["c"], T["e"], T["ts"], T["rays"], T["rays_d"], view, T["delta"]).numpy()
    r6, _ = R.ray_grad(case["c"], case["e"], case["ts"], case["rays"], R.world_dirs(case, case["delta"]))
    want = R.view_grad(r6, view.numpy(), case["delta"])[0]
    assert np.abs(got - want).max() / np.abs(want).max() < 1e-12


def test_pose_apply_torch(case):
    """fp32 poses through the torch statement: float64 inside, so half an ulp of the entries (|entry| <= 4 here: 2^-22); rows whose
    correction is zero come back bit for bit, a -0 included."""
    from nerf2mesh_amd.pose_refine import pose_apply_torch
    poses0 = torch.from_numpy(case["poses0"]).float()
    poses0[0, 0, 3] = -0.0
    delta = torch.from_numpy(case["delta"]).float()
    delta[0] = 0
    out = pose_apply_torch(poses0, delta)
    assert out[0].numpy().tobytes() == poses0[0].numpy().tobytes()
    want = R.apply(poses0.numpy(), delta.numpy())
    assert np.abs(out.numpy() - want).max() <= 2.0 ** -22
    assert (out[:, 3] == poses0[:, 3]).all()


def test_torch_jacobian_across_the_series_threshold():
    from nerf2mesh_amd.pose_refine import SERIES_THETA, left_jacobian, rotation
    axis = np.array([0.36, 0.48, -0.8])
    for th in (0.0, 1e-9, SERIES_THETA * (1 - 1e-6), SERIES_THETA * (1 + 1e-6), 0.3, 2.5):
        w = torch.from_numpy(axis * th)[None]
        assert np.abs(left_jacobian(w)[0].numpy() - R.left_jacobian(axis * th)).max() < 1e-14
        assert np.abs(rotation(w)[0].numpy() - R.rotation(axis * th)).max() < 1e-14


def test_contract_vjp_is_the_transposed_jacobian_of_contract():
    from nerf2mesh_amd.pose_refine import contract_vjp
    from nerf2mesh_amd.renderer import contract
    gen = torch.Generator().manual_seed(0)
    x = (torch.rand(64, 3, generator=gen, dtype=torch.float64) * 2 - 1) * 6          # inside and outside the unit box
    x[:8] *= 0.1
    x.requires_grad_(True)
    g = torch.randn(64, 3, generator=gen, dtype=torch.float64)
    y = contract(x)
    want, = torch.autograd.grad(y, x, g)
    got = contract_vjp(y.detach(), g)
    assert int((x.detach().abs().amax(1) > 1).sum()) > 16 and int((x.detach().abs().amax(1) <= 1).sum()) >= 8
    assert (got - want).abs().max() / want.abs().max() < 1e-12


def test_the_models_contraction_is_the_packages():
    from nerf2mesh_amd.pose_refine import contract_vjp
    rng = np.random.default_rng(2)
    y = rng.uniform(-1.97, 1.97, size=(200, 3))
    y[::5] *= 0.4
    g = rng.normal(size=(200, 3))
    want, mag = R.contract_vjp(y, g)
    got = contract_vjp(torch.from_numpy(y), torch.from_numpy(g)).numpy()
    assert np.abs(got - want).max() < 1e-12 * np.abs(want).max() and (mag >= np.abs(want) - 1e-12).all()
