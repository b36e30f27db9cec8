"""CPU: the lens models, their host inverse, the zoom rule, the fp32 statement capture.undistort_bank / undistort_depth and the loader's
undistort=True path against the float64 loop model of tests/undistort_ref.py.  No GPU needed."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import undistort_ref as R   # noqa: E402
from nerf2mesh_amd import capture as C   # noqa: E402
from nerf2mesh_amd import synthetic   # noqa: E402

IDS = [c[0] for c in R.CASES]


def _lens(model, intr, coeff):
    f4, family, row = C.lens_row(model, R.colmap_params(model, intr, coeff))
    assert f4 == tuple(intr)
    return family, row


@pytest.mark.parametrize("name,model,coeff,intr", R.CASES, ids=IDS)
def test_forward_map_is_the_published_definition_and_the_inverse_undoes_it(name, model, coeff, intr):
    family, row = _lens(model, intr, coeff)
    fx, fy, cx, cy = intr
    jj, ii = np.meshgrid(np.linspace(0, R.H, 13), np.linspace(0, R.W, 17), indexing="ij")       # the whole frame, its edges included
    x, y = ((ii - cx) / fx).ravel(), ((jj - cy) / fy).ravel()
    xd, yd = C.lens_distort(family, row, x, y)
    want = np.array([R.distort(model, coeff, a, b) for a, b in zip(x, y)])
    assert np.abs(xd - want[:, 0]).max() < 1e-14 and np.abs(yd - want[:, 1]).max() < 1e-14
    bx, by = C.lens_undistort(family, row, xd, yd)
    err = max(np.abs(bx - x).max(), np.abs(by - y).max())
    print(f"{name}: inverse o forward, max error {err:.3g} (normalised units)")
    assert err < 1e-10
    assert np.abs(xd - x).max() > 1e-3                                                            # the case distorts at all


def test_the_inverse_refuses_a_point_it_cannot_reach():
    family, row = _lens("OPENCV_FISHEYE", R.CENTRED, (0.0, 0.0, 0.0, 0.0))       # rd = theta < pi / 2: a distorted radius of 5 is beyond the field of view
    with pytest.raises(ValueError, match="did not converge"):
        C.lens_undistort(family, row, np.array([5.0]), np.array([0.0]))


@pytest.mark.parametrize("name,model,coeff,intr", R.CASES, ids=IDS)
def test_zoom_rule_is_exact_at_its_edges(name, model, coeff, intr):
    family, row = _lens(model, intr, coeff)
    s = C.undistort_zoom(R.H, R.W, intr, family, row)
    print(f"{name}: zoom {s:.7f}")
    assert 1.0 <= s <= 4.0
    assert R.taps_inside(model, coeff, intr, R.H, R.W, s)
    if name == "barrel":
        assert s == 1.0
    if s != 1.0:
        assert not R.taps_inside(model, coeff, intr, R.H, R.W, s - 1e-5)
    else:
        assert name in ("barrel", "fisheye")                              # atan compresses like a barrel; every other case needs a zoom


def test_zoom_of_zero_coefficients_is_one_and_an_impossible_lens_is_refused():
    family, row = _lens("OPENCV", R.CENTRED, (0.0, 0.0, 0.0, 0.0))
    assert C.undistort_zoom(R.H, R.W, R.CENTRED, family, row) == 1.0
    family, row = _lens("SIMPLE_RADIAL", R.CENTRED, (4000.0,))
    with pytest.raises(ValueError, match="camera 7"):
        C.undistort_zoom(R.H, R.W, R.CENTRED, family, row, name="camera 7")


def _out(intr, s):
    return (s * intr[0], s * intr[1], intr[2], intr[3])


def _smooth_images(V, model, coeff, intr):
    """The smooth pattern of the reference, evaluated at the pixel centres in normalised coordinates (as an image it is just smooth)."""
    jj, ii = np.meshgrid(np.arange(R.H) + 0.5, np.arange(R.W) + 0.5, indexing="ij")
    x, y = (ii - intr[2]) / intr[0], (jj - intr[3]) / intr[1]
    ims = np.stack([np.stack([R.pattern(x + 0.1 * v, y, f) for f in (1.0, 1.3, 0.7, 1.9)], -1) for v in range(V)])
    return np.clip(np.floor(ims + 0.5), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("name,model,coeff,intr", R.CASES, ids=IDS)
def test_fp32_statement_is_within_one_lsb_of_the_float64_model(name, model, coeff, intr):
    """|fp32 - float64| <= 1 LSB on every channel of every pixel: the bilinear value is continuous in the sample point, the fp32 sample point
    is within 1e-4 px of the float64 one at these sizes, so the value moves by < 0.03 LSB before rounding and only a rounding tie flips."""
    family, row = _lens(model, intr, coeff)
    s = C.undistort_zoom(R.H, R.W, intr, family, row)
    V = 2
    for kind, images in (("noise", R.noise_images(V, R.H, R.W, seed=len(name))), ("smooth", _smooth_images(V, model, coeff, intr))):
        bank, _ = C.pack_rgba8(images)
        got = C.undistort_bank(bank, R.H, R.W, intr, _out(intr, s), row, family)
        got = got.view(torch.uint8).view(V, R.H, R.W, 4).numpy().astype(np.int64)
        want, _ = R.undistort_images(images, model, coeff, intr, _out(intr, s))
        diff = np.abs(got - want.astype(np.int64))
        print(f"{name} {kind}: max |fp32 - float64| = {diff.max()} LSB, values that differ: {(diff != 0).mean():.4%}")
        assert diff.max() <= 1
        assert (got != images).any()                                      # the pass resampled something


def test_statement_takes_a_row_per_view_and_equals_the_broadcast_rows():
    name, model, coeff, intr = R.CASES[3]
    family, row = _lens(model, intr, coeff)
    V = 3
    bank, _ = C.pack_rgba8(R.noise_images(V, R.H, R.W, seed=5))
    out = _out(intr, 1.2)
    one = C.undistort_bank(bank, R.H, R.W, intr, out, row, family)
    tab = C.undistort_bank(bank, R.H, R.W, np.tile(intr, (V, 1)), np.tile(out, (V, 1)), np.tile(row, (V, 1)), family)
    assert torch.equal(one, tab)
    rows = np.tile(row, (V, 1))
    rows[1] = 0                                                           # view 1 has no lens: at zoom 1 it comes back untouched
    outs = np.tile(out, (V, 1))
    outs[1] = intr
    mixed = C.undistort_bank(bank, R.H, R.W, intr, outs, rows, family)
    assert torch.equal(mixed[0], one[0]) and torch.equal(mixed[2], one[2]) and torch.equal(mixed[1], bank[1])


@pytest.mark.parametrize("name,model,coeff,intr", [R.CASES[0], R.CASES[4], R.CASES[6]], ids=[IDS[0], IDS[4], IDS[6]])
def test_depth_statement_takes_the_nearest_texel(name, model, coeff, intr):
    family, row = _lens(model, intr, coeff)
    s = C.undistort_zoom(R.H, R.W, intr, family, row)
    plane = np.random.default_rng(3).random((R.H, R.W)).astype(np.float32)
    got = C.undistort_depth(torch.from_numpy(plane).view(1, -1), R.H, R.W, intr, _out(intr, s), row, family).view(R.H, R.W).numpy()
    want = R.undistort_depth(plane, model, coeff, intr, _out(intr, s))
    assert np.isin(got, plane).all()
    # the two models may choose neighbouring texels only where the sample point is within fp32 rounding of a texel border
    assert (got != want).mean() < 0.01


# ------------------------------------------------------------------------------------------------ the loader
KH, KW = 48, 64
KINTR = (40.0, 40.0, KW / 2, KH / 2)           # the corners are at r = 1: a wide lens


def _synthetic_set(tmp, model, coeff, intr=KINTR, Hh=KH, Ww=KW, V=4, seed=0):
    """A set on disk whose keypoints are the DISTORTED projections of random points (the images are not distorted: these tests read cameras
    and keypoints).  -> the capture it was written from, per view (ideal normalised xy [n,2], index into the points)."""
    poses = synthetic.make_cameras(V, seed=seed)
    cap = C.Capture.synthetic(poses, H=Hh, W=Ww, intrinsics=intr, alpha=False)
    pts = np.random.default_rng(seed).uniform(-0.45, 0.45, (160, 3))
    kps, ideal = [], []
    for v in range(V):
        P = cap.poses[v].double().numpy()
        pc = (pts - P[:3, 3]) @ P[:3, :3]                                 # OpenGL camera: x right, y up, looking along -z
        x, y = pc[:, 0] / -pc[:, 2], -pc[:, 1] / -pc[:, 2]                # COLMAP's normalised coordinates: y down
        d = np.array([R.distort(model, coeff, a, b) for a, b in zip(x, y)])
        px = np.stack([intr[0] * d[:, 0] + intr[2], intr[1] * d[:, 1] + intr[3]], -1)
        m = (pc[:, 2] < 0) & (px[:, 0] >= 0) & (px[:, 0] < Ww) & (px[:, 1] >= 0) & (px[:, 1] < Hh)
        assert m.sum() >= 20
        kps.append((px[m], np.nonzero(m)[0]))
        ideal.append((np.stack([x[m], y[m]], -1), np.nonzero(m)[0]))
    cap.save_colmap(str(tmp), pts, keypoints=kps, distortion=(coeff, model))
    return cap, kps, ideal


def test_keypoints_go_through_the_inverse_and_the_new_intrinsics(tmp_path):
    coeff = (0.1,)
    src, kps, ideal = _synthetic_set(tmp_path, "SIMPLE_RADIAL", coeff)
    family, row = _lens("SIMPLE_RADIAL", KINTR, coeff)
    s = C.undistort_zoom(KH, KW, KINTR, family, row)
    cap = C.Capture.load_colmap(str(tmp_path), split="trainval", scale=1.0, undistort=True, sparse_depth=True, keep_model=True)
    old = C.Capture.load_colmap(str(tmp_path), split="trainval", scale=1.0, sparse_depth=True, keep_model=True)
    assert cap.undistort_zoom == s and s > 1 and old.undistort_zoom is None
    assert cap.intrinsics == (s * KINTR[0], s * KINTR[1], KINTR[2], KINTR[3]) and old.intrinsics == KINTR
    worst = 0.0
    for v in range(len(cap)):
        want = np.stack([s * KINTR[0] * ideal[v][0][:, 0] + KINTR[2], s * KINTR[1] * ideal[v][0][:, 1] + KINTR[3]], -1)
        got, got_old = cap.colmap["keypoints"][v][0], old.colmap["keypoints"][v][0]
        assert np.abs(got - want).max() < 1e-6                            # the pinhole projection under the new intrinsics
        assert np.array_equal(got_old, kps[v][0])                         # without the flag: the coordinates as written
        worst = max(worst, np.abs(got_old - want).max())
        inside = (want[:, 0] >= 0) & (want[:, 0] < KW) & (want[:, 1] >= 0) & (want[:, 1] < KH)      # points that left the frame are dropped
        rc = np.round(np.stack([want[inside, 1], want[inside, 0]], -1)).astype(np.int32)
        rc[:, 0], rc[:, 1] = rc[:, 0].clip(0, KH - 1), rc[:, 1].clip(0, KW - 1)
        assert np.array_equal(cap.sparse_depth.view(v)[0].numpy(), rc)
    print(f"distorted keypoints miss the pinhole projection by up to {worst:.2f} px")
    assert worst > 0.5                                                    # ... which is what reading them as pinhole gets wrong


@pytest.mark.parametrize("model,coeff", [("RADIAL", (0.12, -0.03)), ("OPENCV_FISHEYE", (0.05, 0.01, 0.0, 0.0))])
def test_radial_and_fisheye_cameras_need_the_flag(tmp_path, model, coeff):
    _synthetic_set(tmp_path, model, coeff, Hh=24, Ww=32, intr=(30.0, 30.0, 16.0, 12.0))
    with pytest.raises(ValueError, match="unsupported COLMAP camera model"):
        C.Capture.load_colmap(str(tmp_path), split="trainval", scale=1.0)
    cap = C.Capture.load_colmap(str(tmp_path), split="trainval", scale=1.0, undistort=True)
    family, row = _lens(model, (30.0, 30.0, 16.0, 12.0), coeff)
    s = C.undistort_zoom(24, 32, (30.0, 30.0, 16.0, 12.0), family, row)
    assert cap.undistort_zoom == s and cap.intrinsics == (30.0 * s, 30.0 * s, 16.0, 12.0)
    assert R.taps_inside(model, coeff, (30.0, 30.0, 16.0, 12.0), 24, 32, s)
    assert s == 1.0 or not R.taps_inside(model, coeff, (30.0, 30.0, 16.0, 12.0), 24, 32, s - 1e-5)


def test_full_opencv_keeps_its_error_with_the_flag():
    with pytest.raises(ValueError, match="unsupported COLMAP camera model: FULL_OPENCV"):
        C.lens_row("FULL_OPENCV", [1.0] * 12)


def test_loaded_bank_is_the_statement_of_the_written_one_and_zero_coefficients_skip_the_pass(tmp_path):
    coeff = (0.1, -0.02, 0.003, -0.002)
    intr = (31.0, 28.5, 16.0, 12.0)
    src, _, _ = _synthetic_set(tmp_path / "a", "OPENCV", coeff, Hh=24, Ww=32, intr=intr)
    family, row = _lens("OPENCV", intr, coeff)
    s = C.undistort_zoom(24, 32, intr, family, row)
    cap = C.Capture.load_colmap(str(tmp_path / "a"), split="trainval", scale=1.0, undistort=True)
    plain = C.Capture.load_colmap(str(tmp_path / "a"), split="trainval", scale=1.0)
    assert torch.equal(plain.bank, src.bank) and plain.intrinsics == intr                           # the default: coefficients ignored, as before
    assert torch.equal(cap.bank, C.undistort_bank(src.bank, 24, 32, intr, _out(intr, s), row, family))
    assert not torch.equal(cap.bank, src.bank) and cap.intrinsics == _out(intr, s)
    _synthetic_set(tmp_path / "z", "OPENCV", (0.0, 0.0, 0.0, 0.0), Hh=24, Ww=32, intr=intr)
    a = C.Capture.load_colmap(str(tmp_path / "z"), split="trainval", scale=1.0, undistort=True, sparse_depth=True)
    b = C.Capture.load_colmap(str(tmp_path / "z"), split="trainval", scale=1.0, sparse_depth=True)
    assert a.undistort_zoom == 1.0 and a.intrinsics == b.intrinsics == intr
    assert torch.equal(a.bank, b.bank) and torch.equal(a.mvps, b.mvps) and torch.equal(a.sparse_depth.coords, b.sparse_depth.coords)


def test_downscale_comes_first_then_the_zoom(tmp_path):
    coeff = (0.1,)
    src, _, _ = _synthetic_set(tmp_path, "SIMPLE_RADIAL", coeff)
    half = tuple(x / 2 for x in KINTR)
    family, row = _lens("SIMPLE_RADIAL", KINTR, coeff)
    s = C.undistort_zoom(KH // 2, KW // 2, half, family, row)
    cap = C.Capture.load_colmap(str(tmp_path), split="trainval", scale=1.0, downscale=2, undistort=True)
    assert (cap.H, cap.W) == (KH // 2, KW // 2) and cap.undistort_zoom == s
    assert cap.intrinsics == (half[0] * s, half[1] * s, half[2], half[3])
    small = C.box_downscale(src.bank, KH, KW, 2)
    assert torch.equal(cap.bank, C.undistort_bank(small, KH // 2, KW // 2, half, _out(half, s), row, family))


def test_per_view_cameras_get_a_zoom_each(tmp_path):
    V, intr = 4, (30.0, 30.0, 16.0, 12.0)
    poses = synthetic.make_cameras(V, seed=2)
    table = np.tile(intr, (V, 1))
    table[:, :2] *= np.array([1.0, 1.1, 1.2, 1.3])[:, None]
    src = C.Capture.synthetic(poses, H=24, W=32, intrinsics=table, alpha=False)
    pts = np.random.default_rng(1).uniform(-0.3, 0.3, (80, 3))
    coeffs = np.array([[0.1], [-0.1], [0.05], [0.0]])
    src.save_colmap(str(tmp_path), pts, distortion=(coeffs, "SIMPLE_RADIAL"))
    with pytest.raises(ValueError, match="per_view_intrinsics"):
        C.Capture.load_colmap(str(tmp_path), split="trainval", scale=1.0, undistort=True)
    cap = C.Capture.load_colmap(str(tmp_path), split="trainval", scale=1.0, undistort=True, per_view_intrinsics=True)
    zooms = [C.undistort_zoom(24, 32, table[v], *_lens("SIMPLE_RADIAL", tuple(table[v]), tuple(coeffs[v]))) for v in range(V)]
    assert np.array_equal(cap.undistort_zoom, zooms) and zooms[1] == zooms[3] == 1.0 and zooms[0] > zooms[2] > 1.0
    want = table * np.array([[z, z, 1, 1] for z in zooms])
    assert cap.per_view_intrinsics and np.array_equal(cap.intrinsics_host, want)
    rows = np.zeros((V, 8))
    rows[:, 0] = coeffs[:, 0]
    assert torch.equal(cap.bank, C.undistort_bank(src.bank, 24, 32, table, want, rows, C.LENS_BROWN))
    assert torch.equal(cap.bank[3], src.bank[3])                          # the view without a lens, at zoom 1: untouched


def test_dense_depth_is_resampled_then_calibrated(tmp_path):
    coeff, intr = (0.1,), (30.0, 30.0, 16.0, 12.0)
    poses = synthetic.make_cameras(4, seed=0)
    src = C.Capture.synthetic(poses, H=24, W=32, intrinsics=intr, alpha=False)
    pts = np.random.default_rng(0).uniform(-0.4, 0.4, (120, 3))
    maps = [np.random.default_rng(10 + v).uniform(1.0, 3.0, (24, 32)).astype(np.float32) for v in range(4)]
    src.save_colmap(str(tmp_path), pts, distortion=(coeff, "SIMPLE_RADIAL"), depths=maps)
    cap = C.Capture.load_colmap(str(tmp_path), split="trainval", scale=1.0, undistort=True, dense_depth=True, sparse_depth=True, keep_model=True)
    family, row = _lens("SIMPLE_RADIAL", intr, coeff)
    out = cap.intrinsics
    for v in range(4):
        sc, bi = cap.dense_depth_scale_bias[v]
        plane = C.dense_depth_fill(torch.from_numpy(maps[v]), 24, 32, sc, bi).view(1, -1)
        want = C.undistort_depth(plane, 24, 32, intr, out, row, family)
        assert torch.equal(cap.dense_depth[v], want[0])
        # what was fitted is the UNDISTORTED plane at the undistorted keypoints
        rc = cap.sparse_depth.view(v)[0].long()
        raw = C.undistort_depth(torch.from_numpy(maps[v]).view(1, -1), 24, 32, intr, out, row, family)[0]
        assert np.array_equal(cap.dense_depth_samples[v][:, 0], raw[rc[:, 0] * 32 + rc[:, 1]].double().numpy())
