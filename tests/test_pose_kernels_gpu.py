"""GPU: n2m_pose_apply / n2m_pose_ray_grad / n2m_pose_view_grad (csrc/posegrad.hip) against the float64 model of
tests/pose_ref.py evaluated on the kernels' fp32 inputs.

Bounds.  apply: the largest entry error measured on an MI355X is 0.5 units of 2^-24 (the kernel forms E R0 in double and rounds once; the
entries and translations of this case are below 1); the test allows four times that, 2.0 units.  ray_grad / view_grad: a component that
is a sum of n terms lies within (n + 8) 2^-24 S of the float64 value, S the sum of the absolute values of its terms -- the bound of fp32
summation in any order, the 8 for the roundings inside a term; view_grad's rotational half times the largest absolute row sum of J_l^T.
The reductions have a fixed order, so two calls agree bitwise; they are not independent of the order of the rays, and a permutation of
the rays is held to the bound, not to equal bits."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pose_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
APPLY_MEASURED_UNITS = 0.5          # largest entry error on an MI355X, in units of 2^-24
APPLY_BOUND_UNITS = 4 * APPLY_MEASURED_UNITS


@pytest.fixture(scope="module")
def L():
    from nerf2mesh_amd import _lib
    _lib.lib()
    return _lib


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda().contiguous()


# ------------------------------------------------------------------------------------------------------------------- apply
def _apply_case():
    from nerf2mesh_amd.pose_refine import SERIES_THETA
    rng = np.random.default_rng(5)
    norms = [0.0, 1e-7, SERIES_THETA * (1 - 1e-3), SERIES_THETA * (1 + 1e-3), 0.3, 2.5]
    poses0 = np.tile(np.eye(4, dtype=np.float32), (6, 1, 1))
    delta = np.zeros((6, 6), dtype=np.float32)
    for v, th in enumerate(norms):
        poses0[v, :3, :3] = R.rotation(rng.normal(size=3)).astype(np.float32)
        poses0[v, :3, 3] = rng.uniform(-0.45, 0.45, size=3).astype(np.float32)
        axis = rng.normal(size=3)
        delta[v, :3] = (axis / np.linalg.norm(axis) * th).astype(np.float32)
        delta[v, 3:] = rng.uniform(-0.45, 0.45, size=3).astype(np.float32) if v else 0
    poses0[0, 1, 3] = -0.0
    return norms, poses0, delta


def test_pose_apply(L):
    from nerf2mesh_amd.pose_refine import SERIES_THETA
    norms, poses0, delta = _apply_case()
    got_norms = np.linalg.norm(delta[:, :3].astype(np.float64), axis=1)
    assert got_norms[2] < SERIES_THETA < got_norms[3]                       # one row on either side of the branch
    p0, d = dev(poses0), dev(delta)
    out = torch.full((6, 4, 4), float("nan"), device="cuda")
    L.call("n2m_pose_apply", L.ptr(p0), L.ptr(d), 6, L.ptr(out), L.stream())
    out = out.cpu().numpy()
    assert out[0].tobytes() == poses0[0].tobytes()                          # delta == 0: the stored pose, bit for bit (a -0 included)
    want = R.apply(poses0, delta)
    err = np.abs(out.astype(np.float64) - want).reshape(6, -1).max(1) / U
    print("n2m_pose_apply: largest entry error per row, units of 2^-24:", err, "(bound %.2f)" % APPLY_BOUND_UNITS)
    assert (err <= APPLY_BOUND_UNITS).all()
    assert (out[:, 3] == poses0[:, 3]).all()
    # the bound tells the first-order rotation I + [omega]x from the exponential at |omega| = 0.3
    first = (np.eye(3) + R.skew(delta[4, :3])) @ poses0[4, :3, :3].astype(np.float64)
    assert np.abs(first - want[4, :3, :3]).max() > 1e4 * APPLY_BOUND_UNITS * U
    assert np.abs(first - out[4, :3, :3]).max() > 1e-2


# ---------------------------------------------------------------------------------------------------------------- ray_grad
COUNTS = (0, 1, 2, 63, 64, 65, 127, 130, 1024)


def _ray_case(seed=11):
    rng = np.random.default_rng(seed)
    cnt = np.array(COUNTS, dtype=np.int32)
    N, M = len(cnt), int(cnt.sum())
    order = rng.permutation(N)
    off = np.zeros(N, dtype=np.int32)
    off[order] = np.concatenate([[0], np.cumsum(cnt[order])[:-1]])
    rays = np.stack([off, cnt], 1).astype(np.int32)
    dt = rng.uniform(0.002, 0.01, size=M).astype(np.float32)
    ts = np.stack([rng.uniform(0.3, 3.0, size=M).astype(np.float32) + dt, dt], 1).astype(np.float32)
    y = rng.uniform(-1.97, 1.97, size=(M, 3)).astype(np.float32)          # contracted samples: most outside the unit box, some inside
    y[::5] *= 0.4
    return dict(rays=rays, ts=ts, y=y, g=rng.normal(size=(M, 3)).astype(np.float32), h=rng.normal(size=(M, 3)).astype(np.float32),
                d=rng.normal(size=(N, 3)).astype(np.float32), N=N, M=M)


def _ray_grad(L, c, with_dirs, contract=False):
    g, ts, rays, d = dev(c["g"]), dev(c["ts"]), dev(c["rays"], torch.int32), dev(c["d"])
    h = dev(c["h"]) if with_dirs else None
    y = dev(c["y"]) if contract else None
    out = torch.full((c["N"], 6), float("nan"), device="cuda")
    L.call("n2m_pose_ray_grad", L.ptr(g), L.ptr(h), L.ptr(y), L.ptr(ts), L.ptr(rays), L.ptr(d), c["M"], c["N"], L.ptr(out), L.stream())
    return out.cpu().numpy()


@pytest.mark.parametrize("with_dirs", [True, False])
def test_pose_ray_grad(L, with_dirs):
    c = _ray_case()
    assert sorted(c["rays"][:, 1].tolist()) == sorted(COUNTS) and not np.array_equal(np.argsort(c["rays"][:, 0]), np.arange(c["N"]))
    out = _ray_grad(L, c, with_dirs)
    want, S = R.ray_grad(c["g"], c["h"] if with_dirs else None, c["ts"], c["rays"], c["d"])
    n = c["rays"][:, 1].astype(np.float64)[:, None]
    bound = (n + 8) * U * S
    err = np.abs(out.astype(np.float64) - want)
    print("n2m_pose_ray_grad (grad_dirs %s): error / bound per ray:" % ("given" if with_dirs else "NULL"), (err / np.maximum(bound, 1e-300)).max(1))
    assert np.isfinite(out).all() and (err <= bound).all()
    assert (out[0] == 0).all() and out[0].tobytes() == np.zeros(6, np.float32).tobytes()          # the ray without samples
    assert np.abs(want[1:]).min() > 0
    assert _ray_grad(L, c, with_dirs).tobytes() == out.tobytes()                                   # two calls, identical bits


def test_pose_ray_grad_through_the_contraction(L):
    """xyzs given (opt.contract): every sample's gradient goes back through the contraction first.  The same bound, S now the sum of the
    absolute values of the terms of the contracted gradient (k g and k' <x, g> apart), and 24 in place of 8: the back-projection is a
    dozen more roundings per term (1/m, k, k', three products and two sums of the dot, its division by k, the product and the sum)."""
    c = _ray_case()
    mag = np.abs(c["y"]).max(1)
    assert (mag > 1).sum() > c["M"] // 2 and (mag <= 1).sum() > c["M"] // 20
    out = _ray_grad(L, c, True, contract=True)
    want, S = R.ray_grad(c["g"], c["h"], c["ts"], c["rays"], c["d"], xyzs=c["y"])
    plain, _ = R.ray_grad(c["g"], c["h"], c["ts"], c["rays"], c["d"])
    bound = (c["rays"][:, 1].astype(np.float64)[:, None] + 24) * U * S
    err = np.abs(out.astype(np.float64) - want)
    print("n2m_pose_ray_grad (contracted samples): error / bound per ray:", (err / np.maximum(bound, 1e-300)).max(1))
    assert np.isfinite(out).all() and (err <= bound).all()
    assert (np.abs(plain - want)[3:].max(1) > 100 * bound[3:].max(1)).all()          # the contraction matters on every ray of 63 samples and more
    assert out[0].tobytes() == np.zeros(6, np.float32).tobytes()
    assert _ray_grad(L, c, True, contract=True).tobytes() == out.tobytes()


def test_pose_ray_grad_skips_a_ray_cut_off_by_M(L):
    c = _ray_case()
    whole = _ray_grad(L, c, True)
    ends = c["rays"][:, 0] + c["rays"][:, 1]
    last = int(np.nonzero((ends == c["M"]) & (c["rays"][:, 1] > 0))[0][0])   # the ray that ends at M
    c["M"] -= 1                                                              # (the tensors keep their rows: nothing is read past them)
    out = _ray_grad(L, c, True)
    assert (out[last] == 0).all() and (whole[last] != 0).all()
    keep = np.arange(c["N"]) != last
    assert out[keep].tobytes() == whole[keep].tobytes()


# --------------------------------------------------------------------------------------------------------------- view_grad
def _view_case(seed=17):
    rng = np.random.default_rng(seed)
    V, N = 5, 257
    view = np.concatenate([np.full(200, 3), np.full(1, 1), np.full(30, 0), np.full(26, 4)]).astype(np.int32)      # view 2 has no ray
    rng.shuffle(view)
    delta = np.zeros((V, 6), dtype=np.float32)
    for v, th in enumerate((0.3, 2.5, 0.7, 1e-4, 0.05)):
        axis = rng.normal(size=3)
        delta[v, :3] = (axis / np.linalg.norm(axis) * th).astype(np.float32)
        delta[v, 3:] = rng.normal(size=3).astype(np.float32) * 0.1
    return dict(V=V, N=N, view=view, delta=delta, ray6=rng.normal(size=(N, 6)).astype(np.float32))


def _view_grad(L, c, ray6=None, view=None):
    r6, vw, d = dev(c["ray6"] if ray6 is None else ray6), dev(c["view"] if view is None else view, torch.int32), dev(c["delta"])
    out = torch.full((c["V"], 6), float("nan"), device="cuda")
    L.call("n2m_pose_view_grad", L.ptr(r6), L.ptr(vw), L.ptr(d), c["N"], c["V"], L.ptr(out), L.stream())
    return out.cpu().numpy()


def test_pose_view_grad(L):
    c = _view_case()
    out = _view_grad(L, c)
    want, S, count = R.view_grad(c["ray6"], c["view"], c["delta"])
    assert count.tolist() == [30, 1, 0, 200, 26]
    bound = (count[:, None] + 8) * U * S
    err = np.abs(out.astype(np.float64) - want)
    print("n2m_pose_view_grad: error / bound per view:", (err / np.maximum(bound, 1e-300)).max(1))
    assert np.isfinite(out).all() and (err <= bound).all()
    assert out[2].tobytes() == np.zeros(6, np.float32).tobytes()            # the view without a ray
    assert _view_grad(L, c).tobytes() == out.tobytes()
    # dropping J_l^T is far outside the bound at |omega| = 2.5 (view 1, a single ray)
    assert np.abs(c["ray6"][c["view"] == 1][0, 3:] - want[1, :3]).max() > 1e3 * bound[1, :3].max()
    # a permutation of the rays: the same sums in another order -- within the bound (the reduction is not order-independent)
    perm = np.random.default_rng(1).permutation(c["N"])
    again = _view_grad(L, c, c["ray6"][perm], c["view"][perm])
    assert (np.abs(again.astype(np.float64) - want) <= bound).all()


def test_pose_view_grad_skips_views_outside_the_table(L):
    c = _view_case()
    view = c["view"].copy()
    rows = np.nonzero(view == 3)[0][:7]
    view[rows[:3]], view[rows[3:5]], view[rows[5:]] = -1, c["V"], 2 ** 31 - 1
    out = _view_grad(L, c, view=view)
    want, S, count = R.view_grad(c["ray6"], view, c["delta"])
    assert count.tolist() == [30, 1, 0, 193, 26]
    assert (np.abs(out.astype(np.float64) - want) <= (count[:, None] + 8) * U * S).all()


# ------------------------------------------------------------------------------------------------------------ error returns
def test_error_returns_launch_nothing(L):
    """N2M_EINVAL (-1) for a NULL pointer and for V = 0; the output keeps the bits it had."""
    c = _view_case()
    r6, vw, d = dev(c["ray6"]), dev(c["view"], torch.int32), dev(c["delta"])
    out = torch.full((c["V"], 6), 7.0, device="cuda")
    for args in ((None, L.ptr(vw), L.ptr(d), c["N"], c["V"], L.ptr(out)), (L.ptr(r6), L.ptr(vw), L.ptr(d), c["N"], 0, L.ptr(out))):
        assert L.lib().n2m_pose_view_grad(*args, L.stream()) == -1
    poses = torch.full((c["V"], 4, 4), 7.0, device="cuda")
    p0 = torch.eye(4, device="cuda").repeat(c["V"], 1, 1).contiguous()
    assert L.lib().n2m_pose_apply(L.ptr(p0), None, c["V"], L.ptr(poses), L.stream()) == -1
    assert L.lib().n2m_pose_apply(L.ptr(p0), L.ptr(d), 0, L.ptr(poses), L.stream()) == -1
    rc = _ray_case()
    ray6 = torch.full((rc["N"], 6), 7.0, device="cuda")
    g, ts, rays, dd = dev(rc["g"]), dev(rc["ts"]), dev(rc["rays"], torch.int32), dev(rc["d"])
    assert L.lib().n2m_pose_ray_grad(L.ptr(g), None, None, L.ptr(ts), None, L.ptr(dd), rc["M"], rc["N"], L.ptr(ray6), L.stream()) == -1
    assert L.lib().n2m_pose_ray_grad(L.ptr(g), None, None, L.ptr(ts), L.ptr(rays), L.ptr(dd), 0, rc["N"], L.ptr(ray6), L.stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((poses == 7).all()) and bool((ray6 == 7).all())
