"""capture.Capture.load_colmap(dense_depth=True) / save_colmap(depths=...): the per-view calibration of depths/NAME.npy against the sparse
keypoints and the fp32 depth bank it fills.  Host code only.  The set is the committed tiny reconstruction (9 views of 12 x 10 px, fx != fy,
off-centre principal point, differing keypoint counts) written back with depth maps of the test's own."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dense_depth_case as DC   # noqa: E402

from nerf2mesh_amd import capture as C   # noqa: E402

H, W = 10, 12
SIZES = [(10, 12), (5, 7), (20, 24)]
# a different (scale, bias) per view: the stored map is (depth map - bias) / scale, an exactly affine image of a map that agrees with the
# view's sparse depths
AFFINE = [(0.5 + 0.25 * v, 0.3 - 0.1 * v) for v in range(9)]


@pytest.fixture(scope="module")
def base():
    return DC.tiny()


def _maps(base, h, w):
    out = []
    for v in range(len(base)):
        coords, depth, _ = base.sparse_depth.view(v)
        s, b = AFFINE[v]
        out.append(((DC.nearest_keypoint_map(coords.numpy(), depth.numpy(), H, W, h, w) - b) / s).astype(np.float32))
    return out


@pytest.fixture(scope="module")
def affine_sets(base, tmp_path_factory):
    """{(h, w): (root, maps)}"""
    return {hw: (DC.write(base, str(tmp_path_factory.mktemp(f"dd{hw[0]}x{hw[1]}")), _maps(base, *hw)), _maps(base, *hw)) for hw in SIZES}


_COORDS = {}


def base_coords(root, v):
    """(row, col) of the keypoints of view v, from the sparse table of the same files."""
    if root not in _COORDS:
        _COORDS[root] = C.Capture.load_colmap(root, split="trainval", scale=1.0, sparse_depth=True).sparse_depth
    return _COORDS[root].view(v)[0].long()


def test_calibration_matches_the_lstsq_restatement(affine_sets):
    """The fitted (scale, bias) of every view at every map size against numpy.linalg.lstsq on the same float64 samples.  Tolerance: what
    lstsq itself moves by when its inputs are rounded to fp32 (the precision the bank and the sparse table are held in), times 10 --
    per parameter, the largest over all 27 fits.  Measured: see DESIGN 4.20."""
    got, want, moved = [], [], []
    for hw, (root, maps) in affine_sets.items():
        cap = C.Capture.load_colmap(root, split="trainval", scale=1.0, dense_depth=True, keep_model=True)
        assert cap.sparse_depth is None                                   # dense depth does not need the sparse table
        assert cap.dense_depth.shape == (9, H * W) and cap.dense_depth.dtype == torch.float32
        assert cap.dense_depth_scale_bias.shape == (9, 2) and cap.dense_depth_scale_bias.dtype == np.float64
        for v in range(9):
            x, y, w = cap.dense_depth_samples[v].T
            assert x.dtype == np.float64 and len(x) >= 3
            # the samples are the resized map at the keypoints' pixels
            m = torch.from_numpy(maps[v])
            rc = base_coords(root, v)
            assert np.array_equal(C.resize_linear_at(m, H, W, rc[:, 0], rc[:, 1]).double().numpy(), x)
            if hw == (H, W):
                assert torch.equal(C.dense_depth_fill(m, H, W).view(H, W), m)
            sb = cap.dense_depth_scale_bias[v]
            got.append(sb)
            want.append(DC.lstsq_scale_bias(x, y, w))
            r32 = lambda a: a.astype(np.float32).astype(np.float64)
            moved.append(np.abs(np.subtract(DC.lstsq_scale_bias(r32(x), r32(y), r32(w)), want[-1])))
            assert sb[0] > 0
            # the bank row is the statement at the fitted pair, bit for bit
            assert torch.equal(cap.dense_depth[v], C.dense_depth_fill(m, H, W, sb[0], sb[1])), (hw, v)
            if hw == (H, W):                                              # ... and at equal size the map's own values under the affine map
                s32, b32 = np.float32(sb[0]), np.float32(sb[1])
                assert np.array_equal(cap.dense_depth[v].numpy(), (maps[v].reshape(-1) * s32 + b32).astype(np.float32))
    got, want, moved = np.asarray(got), np.asarray(want), np.asarray(moved)
    tol = 10 * moved.max(0)
    gap = np.abs(got - want).max(0)
    print(f"lstsq moves by (scale, bias) <= {moved.max(0)} under fp32 rounding of its inputs; loader vs lstsq: {gap}; tolerance {tol}")
    assert (tol > 0).all() and (gap <= tol).all(), (gap, tol)


def _decreasing_set(base, tmp_path, fix_top_two):
    """Maps that DEcrease with depth (least squares finds a negative scale); fix_top_two: the pixels of the two most confident keypoints of
    every view are then set to their depths, so the line through those two has slope 1."""
    maps, used = [], []
    for v in range(len(base)):
        coords, depth, weight = (t.numpy() for t in base.sparse_depth.view(v))
        m = (8.0 - DC.nearest_keypoint_map(coords, depth, H, W, H, W)).astype(np.float32)
        k0, k1 = np.argsort(weight.astype(np.float64), kind="stable")[::-1][:2]
        ok = tuple(coords[k0]) != tuple(coords[k1]) and depth[k0] != depth[k1]
        if fix_top_two and ok:
            m[tuple(coords[k0])], m[tuple(coords[k1])] = depth[k0], depth[k1]
        maps.append(m)
        used.append(ok)
    return DC.write(base, str(tmp_path), maps), used


@pytest.mark.parametrize("which", ["two_samples", "one_sample"])
def test_negative_scale_takes_the_fall_backs(base, tmp_path, which):
    root, usable = _decreasing_set(base, tmp_path, which == "two_samples")
    cap = C.Capture.load_colmap(root, split="trainval", scale=1.0, dense_depth=True, keep_model=True)
    taken = 0
    for v in range(9):
        x, y, w = cap.dense_depth_samples[v].T
        if not usable[v] or DC.lstsq_scale_bias(x, y, w)[0] >= 0:
            continue
        two = DC.fallback_two(x, y, w)
        if which == "two_samples":
            if two[0] < 0:
                continue
            assert tuple(cap.dense_depth_scale_bias[v]) == two, v
            assert abs(two[0] - 1) < 1e-6                                  # the two pixels hold the two depths
        else:
            if two[0] >= 0:
                continue
            one = DC.fallback_one(x, y, w)
            assert tuple(cap.dense_depth_scale_bias[v]) == one and one[0] > 0 and one[1] == 0.0, v
        taken += 1
        m = torch.from_numpy(np.load(os.path.join(root, "depths", f"r_{v}.npy")))
        assert torch.equal(cap.dense_depth[v], C.dense_depth_fill(m, H, W, *cap.dense_depth_scale_bias[v]))
    assert taken >= 1, "no view took this fall-back"


def test_fit_degenerate_inputs():
    # one sample, and all x equal: straight to the one-sample fall-back
    assert C.fit_scale_bias([2.0], [3.0], [1.0]) == (1.5, 0.0)
    assert C.fit_scale_bias([2.0, 2.0, 2.0], [1.0, 3.0, 5.0], [0.1, 0.9, 0.5]) == (1.5, 0.0)
    # an exact line is recovered
    x = np.array([1.0, 2.0, 4.0, 7.0])
    s, b = C.fit_scale_bias(x, 0.5 * x + 0.25, [1.0, 0.5, 2.0, 1.5])
    assert abs(s - 0.5) < 1e-12 and abs(b - 0.25) < 1e-12
    with pytest.raises(ValueError):
        C.fit_scale_bias([], [], [])
    with pytest.raises(ValueError, match="most confident"):
        C.fit_scale_bias([0.0], [3.0], [1.0])


def test_missing_map_raises_and_names_it(affine_sets, tmp_path):
    import shutil
    root = str(tmp_path / "rec")
    shutil.copytree(affine_sets[(5, 7)][0], root)
    os.remove(os.path.join(root, "depths", "r_3.npy"))
    with pytest.raises(FileNotFoundError, match="r_3.npy"):
        C.Capture.load_colmap(root, split="trainval", scale=1.0, dense_depth=True)
    assert len(C.Capture.load_colmap(root, split="val", scale=1.0, dense_depth=True)) == 2      # the val split does not need view 3
    np.save(os.path.join(root, "depths", "r_3.npy"), np.zeros((2, 3, 4), np.float32))
    with pytest.raises(ValueError, match="2-D depth map"):
        C.Capture.load_colmap(root, split="trainval", scale=1.0, dense_depth=True)


def test_splits_bytes_and_the_flag_off(affine_sets):
    root, maps = affine_sets[(20, 24)]
    full = C.Capture.load_colmap(root, split="trainval", scale=1.0, dense_depth=True)
    for split, ids in (("val", [0, 8]), ("train", [1, 2, 3, 4, 5, 6, 7])):
        cap = C.Capture.load_colmap(root, split=split, scale=1.0, dense_depth=True)
        assert torch.equal(cap.dense_depth, full.dense_depth[ids]) and torch.equal(cap.bank, full.bank[ids])
        assert np.array_equal(cap.dense_depth_scale_bias, full.dense_depth_scale_bias[ids])
        assert cap.dense_depth_samples is None                            # kept with keep_model=True only
    off = C.Capture.load_colmap(root, split="trainval", scale=1.0)
    assert off.dense_depth is None and off.dense_depth_scale_bias is None and off.nbytes == off.bank.numel() * 4
    assert full.nbytes - off.nbytes == 4 * 9 * H * W
    # without the flag the folder of maps changes nothing: the capture of the reconstruction without it
    plain = C.Capture.load_colmap(DC.TINY, split="trainval", scale=1.0)
    assert torch.equal(off.bank, plain.bank) and off.intrinsics == plain.intrinsics and (off.H, off.W) == (plain.H, plain.W)
    assert (off.poses - plain.poses).abs().max() <= 4 * 2.4e-7             # tests/test_colmap_io.py ROUND_TRIP_TOL: a quaternion and back


def test_save_then_load_gives_the_bank_back(affine_sets, tmp_path):
    """load -> save_colmap(depths = the maps read) -> load: the files hold the arrays given, and the bank comes back.  The second set's poses
    went through a quaternion and back once more (tests/test_colmap_io.py: one fp32 ulp of a magnitude below 4, 2.4e-7, x 4), so its
    sparse depths move by that much; the calibration is a least squares on them with the maps' own values as abscissae (0.5 .. 20 here,
    spread over more than 1), so scale and bias move by a small multiple of it and a bank value |scale| * |map| + |bias| < 64 by its
    ulp (3.8e-6) on top: 1e-4 absolute covers both with a factor of 10."""
    root, maps = affine_sets[(5, 7)]
    a = C.Capture.load_colmap(root, split="trainval", scale=1.0, dense_depth=True, keep_model=True)
    read = [np.load(os.path.join(root, "depths", f"r_{v}.npy")) for v in range(9)]
    for m, r in zip(maps, read):
        assert r.dtype == np.float32 and np.array_equal(m, r)
    again = str(tmp_path / "again")
    a.save_colmap(again, scale=1.0, depths=read, **a.colmap)
    b = C.Capture.load_colmap(again, split="trainval", scale=1.0, dense_depth=True)
    assert torch.equal(a.bank, b.bank)
    assert np.abs(a.dense_depth_scale_bias - b.dense_depth_scale_bias).max() <= 1e-4
    assert (a.dense_depth - b.dense_depth).abs().max() <= 1e-4
    assert float(a.dense_depth.abs().max()) < 64
    # a second load of the same files is the same bank, bit for bit
    assert torch.equal(b.dense_depth, C.Capture.load_colmap(again, split="trainval", scale=1.0, dense_depth=True).dense_depth)
    with pytest.raises(ValueError, match="one 2-D array per view"):
        a.save_colmap(again, scale=1.0, depths=read[:3], **a.colmap)
    # save_colmap without the argument writes no depths folder
    bare = str(tmp_path / "bare")
    a.save_colmap(bare, scale=1.0, **a.colmap)
    assert not os.path.exists(os.path.join(bare, "depths"))
