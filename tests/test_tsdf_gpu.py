"""GPU: n2m_tsdf_integrate against the float64 model of its rule (tests/tsdf_ref.py), its bit-exactness across chunking, TSDFVolume.extract
on an analytic sphere, and export_stage0(method="tsdf") on a briefly trained model.

Tolerance of the kernel-against-model comparison, from the arithmetic of the rule (u = 2^-24, the relative error of one fp32 operation;
the model reads the same fp32 inputs, so only the kernel's own roundings count):
  * a lattice coordinate x = lo + index * step carries three roundings (step, the product, the sum) of values <= B = max(|lo|, |hi|):
    |dx| <= 3 u B;  d = x - c then has |dd| <= 3 u B + u D, D the largest |x_k - c_k| (<= max |c_k| + B);
  * zc = -((R2 d0 + R5 d1) + R8 d2), |R| <= 1: three products (each |R| dd + u |R d|) and two sums (each u times a partial sum
    <= 3 D):  |dzc| <= 3 (3 u B + u D) + 3 u D + 6 u D = (9 B + 12 D) u;
  * sdf = dm - zc adds u |sdf|, which matters only where |sdf| <= trunc (beyond, s is clipped to 1 or the view is skipped), and the
    division one more u |s| <= u:  |ds| <= (9 B + 12 D) u / trunc + 2 u;
  * a running-average step (tsdf w + s) / (w + 1) rounds three times on values <= w + 1, i.e. <= 3 u after the division, and hands the
    errors of its inputs on with weights w / (w + 1) and 1 / (w + 1), which sum to 1:  after n views <= 3 n u + max |ds|.
  tol = (3 n + 2 + (9 B + 12 D) / trunc) * 2^-24.  Decisions (which pixel, skip or not) are not rounding errors: the model marks the
  (point, view) pairs within 1e-3 px / 1e-4 of one, and those points are left out -- at most 2 % of the pairs, asserted."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsdf_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _tol(cams, n, trunc, B=1.0):
    D = float(np.abs(cams[:, 9:12]).max()) + B
    return (3 * n + 2 + (9 * B + 12 * D) / trunc) * U


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _volume(res, cams, depth, parts=None, **kw):
    import torch
    from nerf2mesh_amd.tsdf import TSDFVolume
    vol = TSDFVolume(res, R.LO, R.HI, device="cuda", **kw)
    c, d = torch.from_numpy(cams).cuda(), torch.from_numpy(depth).cuda()
    for part in (parts or [list(range(len(cams)))]):
        vol.integrate(c[part], d[part])
    return vol


@pytest.fixture(scope="module")
def small():
    cams, depth = R.small_fixture()
    return cams, depth


@pytest.mark.parametrize("res", [R.R_SMALL, (2, 2, 2)])
def test_kernel_matches_the_float64_model(small, res):
    cams, depth = small
    vol = _volume(res, cams, depth, **R.SMALL)
    t, w, near, used = R.integrate(np.ones(res), np.zeros(res), R.LO, R.HI, cams, depth, **R.SMALL)
    tol = _tol(cams, len(cams), R.SMALL["trunc"])
    gt, gw = vol.tsdf.cpu().numpy().astype(np.float64), vol.weight.cpu().numpy().astype(np.float64)
    ok = ~near.any(axis=0)
    err = np.abs(gt - t)[ok].max()
    print(f"\n{res}: near-decision share {near.mean():.4f}, {ok.mean():.3f} of the points compared, {used.mean():.3f} of the pairs update; "
          f"max |tsdf - model| {err:.3e} (tol {tol:.3e}), weight mismatches {(gw != w)[ok].sum()}")
    assert near.mean() <= 0.02
    assert np.array_equal(gw[ok], w[ok])
    assert err <= tol
    assert used.any() and np.isfinite(gt).all()


def test_bit_exact_across_chunking_and_runs(small):
    import torch
    cams, depth = small
    one = _volume(R.R_SMALL, cams, depth, **R.SMALL)
    again = _volume(R.R_SMALL, cams, depth, **R.SMALL)
    parts = _volume(R.R_SMALL, cams, depth, parts=[[0, 1], [2], [3, 4]], **R.SMALL)
    for other in (again, parts):
        assert torch.equal(_bits(one.tsdf), _bits(other.tsdf)) and torch.equal(_bits(one.weight), _bits(other.weight))
    assert float(one.weight.max()) == R.SMALL["w_max"]


def test_skipped_observations_leave_the_volume_untouched(small):
    import torch
    cams, depth = small
    nothing = np.stack([np.zeros_like(depth[0]), -np.ones_like(depth[0]), np.full_like(depth[0], np.nan), np.full_like(depth[0], -np.inf),
                        np.zeros_like(depth[0])])
    away = cams.copy()
    away[:4, :9] = (cams[:4, :9].reshape(4, 3, 3) * np.array([-1.0, 1.0, -1.0], np.float32)).reshape(4, 9)      # turned by 180 degrees about y
    far_surface = np.full_like(depth, 1e-3)                            # in front of every point by > trunc, for the four cameras at radius 3
    for c, d, kw in ((cams, nothing, R.SMALL), (away[:4], depth[:4], R.SMALL), (cams[:4], far_surface[:4], R.SMALL),
                     (cams, depth, {**R.SMALL, "min_depth": 10.0})):
        vol = _volume(R.R_SMALL, c, d, **kw)
        assert bool((vol.tsdf == 1).all()) and bool((vol.weight == 0).all())
        assert torch.equal(_bits(vol.tsdf), _bits(torch.ones_like(vol.tsdf)))


# ------------------------------------------------------------------------------------------------ extraction
def _fuse_sphere(blob, carve):
    """The sphere fixture through surface_depth: opacity 1 where a ray hits, 0 where it misses."""
    import torch
    from nerf2mesh_amd.tsdf import TSDFVolume, surface_depth
    cams, z, hit = R.sphere_fixture(blob=blob)
    alpha = torch.from_numpy(hit.astype(np.float32)).cuda()
    depth = surface_depth({"depth": torch.from_numpy(z).cuda() * alpha, "weights_sum": alpha}, carve=carve)
    vol = TSDFVolume(R.R_SPHERE, device="cuda")
    return vol.integrate(torch.from_numpy(cams).cuda(), depth)


def _edge_endpoints(vol, v):
    """Index-space position of every vertex and the lattice indices of its edge's endpoints.  A vertex comes back as lo + p * spacing
    rounded to fp32 (error <= 2^-23 of a coordinate <= 1, i.e. 2e-6 lattice spacings at R = 32): a coordinate within 1e-4 of an integer
    is that integer."""
    p = (v.double().cpu().numpy() - np.array(vol.lo)) / np.array(vol.spacing)
    snap = np.abs(p - np.round(p)) < 1e-4
    p = np.where(snap, np.round(p), p)
    return p, np.floor(p).astype(int), np.ceil(p).astype(int)


def test_extract_on_the_analytic_sphere():
    vol = _fuse_sphere(blob=False, carve=True)
    v, tri = vol.extract()
    assert v.shape[0] > 500 and tri.shape[0] > 500 and int(tri.max()) < v.shape[0] and int(tri.min()) >= 0
    spacing = 2.0 / (R.R_SPHERE - 1)
    err = (v.double().norm(dim=1) - R.RADIUS).abs()
    print(f"\n{v.shape[0]} vertices, {tri.shape[0]} triangles: mean error {float(err.mean()) / spacing:.3f}, max {float(err.max()) / spacing:.3f} spacings")
    assert float(err.mean()) <= 0.5 * spacing and float(err.max()) <= 2.0 * spacing          # the model's bounds (test_tsdf_ref_cpu)
    p, a, b = _edge_endpoints(vol, v)
    assert ((a != b).sum(axis=1) <= 1).all()                                                 # every vertex sits on one lattice edge
    w = vol.weight.cpu().numpy()
    assert (w[a[:, 0], a[:, 1], a[:, 2]] > 0).all() and (w[b[:, 0], b[:, 1], b[:, 2]] > 0).all()
    # the removal is not vacuous: the raw level set has the sheet towards the unobserved inside of the sphere
    from nerf2mesh_amd.marching_cubes import marching_cubes
    raw = marching_cubes(vol.tsdf, 0.0, div=R.R_SPHERE - 1.0, mul=2.0, add=-1.0)[0]
    assert raw.shape[0] > v.shape[0] and float((raw.norm(dim=1) - R.RADIUS).abs().max()) > 2.0 * spacing
    assert bool((vol.weight == 0).any())


def test_carving_removes_a_floater_one_view_saw():
    kept = _fuse_sphere(blob=True, carve=False).extract()[0]
    assert int((kept.norm(dim=1) > 0.7).sum()) > 0                   # without carving the floater is meshed
    v, tri = _fuse_sphere(blob=True, carve=True).extract()
    assert v.shape[0] > 500 and tri.shape[0] > 500
    assert float(v.norm(dim=1).max()) <= 0.7


# ------------------------------------------------------------------------------------------------ export path
@pytest.fixture(scope="module")
def trained():
    """The schedule of the export tests (test_marching_cubes.test_export_stage0_feeds_stage1: -O --bound 1 --dt_gamma 0, fused field, 400
    steps) on the set of test_capture_pipeline_gpu: six views of 48 x 64."""
    import torch
    from nerf2mesh_amd import synthetic
    from nerf2mesh_amd.capture import Capture
    from nerf2mesh_amd.engine import Stage0Engine
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    torch.manual_seed(0)
    cap = Capture.synthetic(synthetic.make_cameras(6, seed=0), H=48, W=64, intrinsics=(70.0, 60.0, 30.5, 25.25), device="cuda")
    opt = make_options(O=True, bound=1, dt_gamma=0, iters=30000, fused_mlp=True)
    eng = Stage0Engine(NeRFNetwork(opt), opt, None, torch.device("cuda:0"), seed=0, capture=cap)
    eng.mark_untrained()
    for _ in range(400):
        eng.train_step()
    return eng.model, cap


def test_export_stage0_tsdf(trained, tmp_path):
    import torch
    from nerf2mesh_amd import export
    model, cap = trained
    same = lambda a, b: torch.equal(a[1], b[1]) and torch.equal(_bits(a[0]), _bits(b[0]))
    before = model.export_stage0(str(tmp_path / "d0"), resolution=40)[0]
    res = 40
    v, t = model.export_stage0(str(tmp_path / "tsdf"), resolution=res, dataset=cap, method="tsdf")[0]
    after = model.export_stage0(str(tmp_path / "d1"), resolution=40, method="density")[0]
    assert same(before, after)
    print(f"\nTSDF export at {res}^3: {v.shape[0]} vertices, {t.shape[0]} triangles (density: {before[0].shape[0]} / {before[1].shape[0]})")
    assert v.shape[0] > 0 and t.shape[0] > 0 and int(t.max()) < v.shape[0] and float(v.abs().max()) <= 1.0
    pv, pt = export.read_ply(str(tmp_path / "tsdf" / "mesh_0.ply"))
    assert np.array_equal(pv, v.cpu().numpy()) and np.array_equal(pt, t.cpu().numpy())
    # the resolution is honoured: every vertex sits on an edge of the 40^3 lattice (two coordinates on lattice planes; a coordinate is
    # lo + p * spacing rounded to fp32, 2^-23 of <= 1 = 2.4e-6 spacings at R = 40)
    p = (v.double().cpu().numpy() + 1.0) / 2.0 * (res - 1)
    assert ((np.abs(p - np.round(p)) < 1e-4).sum(axis=1) >= 2).all()
    # the keywords reach the volume and the depth encoding; an unknown one is refused
    v2, _ = model.export_stage0(str(tmp_path / "tsdf2"), resolution=res, dataset=cap, method="tsdf", tsdf=dict(trunc=0.2, carve=True, alpha_min=0.3, chunk=4))[0]
    assert v2.shape[0] > 0 and not (v2.shape == v.shape and torch.equal(v2, v))
    with pytest.raises(ValueError, match="unknown tsdf option"):
        model.export_stage0(str(tmp_path / "tsdf3"), resolution=res, dataset=cap, method="tsdf", tsdf=dict(truncation=0.2))
