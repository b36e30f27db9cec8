"""CPU: the float64 model of the TSDF integration rule (tests/tsdf_ref.py) against the project's ray generator and an analytic sphere, the
near-decision share of the fixture the GPU test compares the kernel on, and the model's independence of how the views are chunked."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_ref as R  # noqa: E402


def test_camera_convention_matches_the_ray_generator():
    """A point rays_o + t rays_d of capture.view(v) has depth t in the model's camera and lands in the pixel of its own ray.
    The rays are fp32 results and the stored poses are orthonormal to fp32 rounding only, so zc == t holds to a few fp32 ulps, not to fp64
    rounding: per component the direction carries <= 3 roundings (2^-24 each, relative), the rotation's R^T R differs from the identity by
    <= 4 * 2^-24 per entry, and |dir| <= 1.7 here -- |zc - t| <= 16 * 2^-24 * t < 1e-6 t.  A pixel centre sits 0.5 px from the pixel's
    edges, so the same error (times fx <= 70) cannot move the point into a neighbour."""
    import torch
    from nerf2mesh_amd import synthetic
    from nerf2mesh_amd.capture import Capture
    H, W = 6, 9
    rows = np.array([[70.0, 60.0, 4.5, 3.25], [55.0, 65.0, 4.0, 2.5], [62.0, 58.0, 5.25, 3.0]])
    cap = Capture.synthetic(synthetic.make_cameras(3, seed=2), H=H, W=W, intrinsics=rows)
    assert cap.per_view_intrinsics
    cams = R.camera_rows(cap.poses.numpy(), np.array([cap.intrinsics_of(v) for v in range(3)]))
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for v in range(3):
        rays_o, rays_d = (x.double().numpy() for x in cap.view(v)[:2])
        for t in (0.25, 1.0, 3.7):
            zc, col, row = R.project(cams[v], rays_o + t * rays_d)
            assert np.abs(zc - t).max() <= 1e-6 * t
            assert np.array_equal(np.floor(col).astype(int), ii.reshape(-1)) and np.array_equal(np.floor(row).astype(int), jj.reshape(-1))
            assert np.abs(col - (ii.reshape(-1) + 0.5)).max() < 1e-3 and np.abs(row - (jj.reshape(-1) + 0.5)).max() < 1e-3


@pytest.fixture(scope="module")
def sphere_model():
    cams, z, hit = R.sphere_fixture()
    depth = np.where(hit, z, np.inf).astype(np.float32)                   # a ray that misses stops at nothing: +inf carves
    res = (R.R_SPHERE,) * 3
    spacing = 2.0 / (R.R_SPHERE - 1)
    return R.integrate(np.ones(res), np.zeros(res), R.LO, R.HI, cams, depth, 4 * spacing, 0.0, 64.0), spacing


def test_analytic_sphere_surface(sphere_model):
    """The zero crossings of the fused volume along observed lattice edges lie on the sphere: mean | |x| - 0.6 | <= half a lattice spacing,
    max <= two spacings."""
    (t, w, _, used), spacing = sphere_model
    X = R.zero_crossings(t, w, R.LO, R.HI)
    err = np.abs(np.linalg.norm(X, axis=1) - R.RADIUS)
    print(f"\n{len(X)} crossings: mean error {err.mean() / spacing:.3f}, max {err.max() / spacing:.3f} lattice spacings; "
          f"{(w > 0).mean():.3f} of the lattice observed")
    assert len(X) > 500
    assert err.mean() <= 0.5 * spacing and err.max() <= 2.0 * spacing
    assert (w <= 8).all() and used.any(axis=0).mean() > 0.5


def test_near_decision_share_of_the_gpu_fixture():
    """At most 2 % of the (point, view) pairs of the kernel-against-model fixture are near-decision, and the fixture exercises what it is
    for: every view updates points, some points lie behind a camera or nearer than min_depth, the weight cap binds."""
    cams, depth = R.small_fixture()
    t, w, near, used = R.integrate(np.ones(R.R_SMALL), np.zeros(R.R_SMALL), R.LO, R.HI, cams, depth, **R.SMALL)
    zc = np.stack([R.project(c, R.lattice(R.R_SMALL, R.LO, R.HI))[0] for c in cams])
    print(f"\nnear-decision share {near.mean():.4f}; updated {used.mean():.3f} of the pairs; behind or too near: {(zc <= R.SMALL['min_depth']).mean():.3f}")
    assert near.mean() <= 0.02
    assert used.reshape(5, -1).any(axis=1).all()
    assert (zc[4] <= R.SMALL["min_depth"]).any() and (zc[4] > R.SMALL["min_depth"]).any()
    assert (w == R.SMALL["w_max"]).any() and (used.sum(axis=0) > R.SMALL["w_max"]).any()
    assert (t < 0).any() and (t == 1).any() and ((t > 0) & (t < 1)).any()
    assert np.isnan(depth).sum() == 3 and (depth == 0).sum() == 3 and (depth < 0).sum() == 3 and np.isinf(depth).any()


def test_model_is_chunk_invariant():
    cams, depth = R.small_fixture()
    t1, w1, near1, _ = R.integrate(np.ones(R.R_SMALL), np.zeros(R.R_SMALL), R.LO, R.HI, cams, depth, **R.SMALL)
    t, w = np.ones(R.R_SMALL), np.zeros(R.R_SMALL)
    nears = []
    for part in ([0, 1], [2], [3, 4]):
        t, w, near, _ = R.integrate(t, w, R.LO, R.HI, cams[part], depth[part], **R.SMALL)
        nears.append(near)
    assert np.array_equal(t, t1) and np.array_equal(w, w1) and np.array_equal(np.concatenate(nears), near1)
