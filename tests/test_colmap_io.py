"""capture.Capture.load_colmap / save_colmap against what the reference's ColmapDataset makes of the committed tiny reconstruction
(tests/golden/colmap_tiny/, colmap_tiny.npz; generator: tests/golden/make_golden_colmap.py).  Host code only."""
import os
import shutil

import numpy as np
import pytest
import torch

from nerf2mesh_amd import capture as C

HERE = os.path.dirname(os.path.abspath(__file__))
TINY = os.path.join(HERE, "golden", "colmap_tiny")

# Measured gap between the reference's float64 path cast to fp32 (the npz) and the loader (its own reader, the analytic inverse [R^T | -R^T t]
# instead of numpy.linalg.inv, float64 throughout, one cast at the end), largest absolute difference over the three recorded runs:
#   poses 0, intrinsics 0, pts_aabb 0, cam_near_far 0, depth 0, weight 0 (every field bitwise equal; scale equal to 1e-12 relative).
# The two float64 paths differ by a few 1e-16 at most, and none of the ~700 recorded values lies that close to a rounding boundary of fp32.
# 4 x the measured gap is therefore 0: the float fields are compared exactly.
GAP = 0.0
TOL = 4 * GAP
# save_colmap -> load_colmap goes through a quaternion and back and re-centres an already centred set: a few float64 roundings, which may
# move an fp32 result (magnitude below 4, ulp 2.4e-7) to its neighbour -- one ulp, with the same 4 x margin
ROUND_TRIP_TOL = 4 * 2.4e-7


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(HERE, "golden", "colmap_tiny.npz")))


def _gaps(cap, g, tag):
    sd = cap.sparse_depth
    return {"poses": np.abs(cap.poses.numpy() - g[tag + "poses"]).max(),
            "pts_aabb": np.abs(cap.pts_aabb.numpy() - g[tag + "pts_aabb"].astype(np.float32)).max(),
            "cam_near_far": np.abs(cap.cam_near_far.numpy() - g[tag + "cam_near_far"]).max(),
            "depth": np.abs(sd.depth.numpy() - g[tag + "depth"]).max(),
            "weight": np.abs(sd.weight.numpy() - g[tag + "weight"]).max(),
            "intrinsics": np.abs(np.asarray(cap.intrinsics, dtype=np.float32) - g[tag + "intrinsics"]).max()}


@pytest.mark.parametrize("tag,kw", [("", dict(scale=-1)), ("ds2_", dict(scale=-1, downscale=2)), ("cc_", dict(scale=0.5, enable_cam_center=True))])
def test_load_colmap_matches_reference(gold, tag, kw):
    """Integer fields exact, float fields within 4 x the measured gap (see GAP above).  `ds2_` reads the images_2 folder."""
    cap = C.Capture.load_colmap(TINY, split="trainval", sparse_depth=True, **kw)
    g = gold
    assert (cap.H, cap.W) == tuple(g[tag + "HW"])
    assert len(cap) == 9
    sd = cap.sparse_depth
    assert sd.offsets.dtype == torch.int32 and sd.coords.dtype == torch.int32 and sd.depth.dtype == torch.float32
    assert np.array_equal(sd.offsets.numpy(), g[tag + "offsets"])
    assert np.array_equal(sd.coords.numpy(), g[tag + "coords"])
    assert np.array_equal(cap.bank_bytes().numpy()[..., :3], g[tag + "images"]) and not cap.has_alpha
    assert (cap.bank_bytes().numpy()[..., 3] == 255).all()
    assert abs(cap.scale / float(g[tag + "scale"]) - 1) < 1e-12
    gaps = _gaps(cap, g, tag)
    print(tag or "plain", {k: float(v) for k, v in gaps.items()})
    for k, v in gaps.items():
        assert v <= TOL, (k, v)
    # every intrinsic is the fp32 of the same quotient
    assert np.array_equal(np.asarray(cap.intrinsics, dtype=np.float32), g[tag + "intrinsics"][0])
    assert (g[tag + "intrinsics"] == g[tag + "intrinsics"][0]).all()
    assert tuple(cap.cam_near_far.shape) == (9, 2) and tuple(cap.pts_aabb.shape) == (6,)


def test_scale_auto_is_inverse_of_nearest_camera(gold):
    cap = C.Capture.load_colmap(TINY, split="trainval", scale=-1)
    assert cap.sparse_depth is None
    r = torch.linalg.norm(cap.poses[:, :3, 3].double(), dim=-1)
    assert abs(float(r.min()) - 1.0) < 1e-6
    one = C.Capture.load_colmap(TINY, split="trainval", scale=1.0)
    assert abs(1.0 / float(torch.linalg.norm(one.poses[:, :3, 3].double(), dim=-1).min()) / cap.scale - 1) < 1e-6


def test_splits(gold):
    full = C.Capture.load_colmap(TINY, split="trainval", sparse_depth=True)
    for split in ("train", "val"):
        ids = gold[split + "_ids"].tolist()
        cap = C.Capture.load_colmap(TINY, split=split, sparse_depth=True)
        assert len(cap) == len(ids)
        assert torch.equal(cap.poses, full.poses[ids]) and torch.equal(cap.bank, full.bank[ids])
        assert torch.equal(cap.cam_near_far, full.cam_near_far[ids]) and torch.equal(cap.pts_aabb, full.pts_aabb)
        assert cap.sparse_depth.counts == [full.sparse_depth.counts[i] for i in ids]
        for n, i in enumerate(ids):
            for a, b in zip(cap.sparse_depth.view(n), full.sparse_depth.view(i)):
                assert torch.equal(a, b)
    assert gold["val_ids"].tolist() == [0, 8] and gold["train_ids"].tolist() == [1, 2, 3, 4, 5, 6, 7]


def test_downscale_without_folder_takes_the_box_mean(gold, tmp_path):
    """downscale = 2 without images_2/: the bank's own box downscale of images/ -- which is how the fixture's images_2 was made, so both
    routes give the same bank; geometry is the reference's downscale-2 run either way."""
    root = str(tmp_path / "rec")
    shutil.copytree(TINY, root, ignore=shutil.ignore_patterns("images_2"))
    a = C.Capture.load_colmap(root, split="trainval", downscale=2, sparse_depth=True)
    b = C.Capture.load_colmap(TINY, split="trainval", downscale=2, sparse_depth=True)
    assert (a.H, a.W) == (5, 6) == tuple(gold["ds2_HW"])
    assert torch.equal(a.bank, b.bank) and torch.equal(a.poses, b.poses) and a.intrinsics == b.intrinsics
    assert np.array_equal(a.sparse_depth.coords.numpy(), gold["ds2_coords"])
    with pytest.raises(ValueError, match="integer downscale"):
        C.Capture.load_colmap(root, split="trainval", downscale=1.5)        # no box of 1.5 x 1.5 pixels


def test_save_then_load_is_identity(tmp_path):
    """A capture that load_colmap produced is already centred: written back with its own points and keypoints it loads as itself."""
    a = C.Capture.load_colmap(TINY, split="trainval", scale=0.7, sparse_depth=True, keep_model=True)
    a.save_colmap(str(tmp_path / "again"), scale=0.7, **a.colmap)
    b = C.Capture.load_colmap(str(tmp_path / "again"), split="trainval", scale=0.7, sparse_depth=True, keep_model=True)
    assert C.Capture.load_colmap(TINY, split="trainval").colmap is None       # kept on request only
    assert (a.H, a.W, a.intrinsics, a.has_alpha) == (b.H, b.W, b.intrinsics, b.has_alpha)
    assert torch.equal(a.bank, b.bank)
    assert torch.equal(a.sparse_depth.offsets, b.sparse_depth.offsets) and torch.equal(a.sparse_depth.coords, b.sparse_depth.coords)
    assert torch.equal(a.sparse_depth.weight, b.sparse_depth.weight)
    for x, y in ((a.poses, b.poses), (a.pts_aabb, b.pts_aabb), (a.cam_near_far, b.cam_near_far), (a.sparse_depth.depth, b.sparse_depth.depth)):
        assert (x - y).abs().max() <= ROUND_TRIP_TOL
    for (xa, ia), (xb, ib) in zip(a.colmap["keypoints"], b.colmap["keypoints"]):
        assert np.array_equal(xa, xb) and np.array_equal(ia, ib)           # the ones without a point and outside the image included


def test_save_colmap_from_points_and_masks(tmp_path):
    """A capture that did not come from a reconstruction: save_colmap projects the point list itself; SIMPLE_PINHOLE; alpha from mask/."""
    from PIL import Image
    from nerf2mesh_amd import synthetic as S
    cap = C.Capture.synthetic(S.make_cameras(4, seed=1), H=8, W=8, intrinsics=(9.0, 9.0, 4.0, 4.0), alpha=False)
    pts = np.random.default_rng(0).uniform(-0.3, 0.3, (12, 3))
    root = str(tmp_path / "rec")
    cap.save_colmap(root, pts, model="SIMPLE_PINHOLE", folder="colmap")
    os.makedirs(os.path.join(root, "mask"))
    mask = np.zeros((8, 8), np.uint8)
    mask[2:6] = 200
    Image.fromarray(mask).save(os.path.join(root, "mask", "r_1.png"))
    got = C.Capture.load_colmap(root, split="trainval", scale=1.0)
    assert got.has_alpha and got.intrinsics == cap.intrinsics and len(got) == 4
    by = got.bank_bytes().numpy()
    assert np.array_equal(by[1, :, :, 3], mask) and (by[[0, 2, 3], :, :, 3] == 255).all()
    assert np.array_equal(by[..., :3], cap.bank_bytes().numpy()[..., :3])
    with pytest.raises(ValueError, match="SIMPLE_PINHOLE when"):
        C.Capture.synthetic(S.make_cameras(2, seed=1), H=4, W=4, intrinsics=(9.0, 8.0, 2.0, 2.0)).save_colmap(root, pts, model="SIMPLE_PINHOLE")


def _rewrite_cameras(root, cams):
    import struct
    with open(os.path.join(root, "sparse", "0", "cameras.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(cams)))
        for cid, model, w, h, params in cams:
            f.write(struct.pack("<iiQQ", cid, model, w, h))
            f.write(np.asarray(params, dtype="<f8").tobytes())


def test_value_errors(tmp_path):
    with pytest.raises(ValueError, match="no COLMAP model"):
        C.Capture.load_colmap(str(tmp_path))
    with pytest.raises(ValueError, match="split"):
        C.Capture.load_colmap(TINY, split="test")
    root = str(tmp_path / "rec")
    shutil.copytree(TINY, root)
    _rewrite_cameras(root, [(1, 5, 12, 10, [14, 13, 6.5, 4.25, 0, 0, 0, 0])])
    with pytest.raises(ValueError, match="unsupported COLMAP camera model: OPENCV_FISHEYE"):
        C.Capture.load_colmap(root)
    _rewrite_cameras(root, [(1, 77, 12, 10, [14, 13, 6.5, 4.25])])
    with pytest.raises(ValueError, match="unknown camera model id"):
        C.Capture.load_colmap(root)
    # the other supported models read their focal lengths and centre, and ignore the distortion
    for model, params, want in ((0, [14, 6.5, 4.25], (14, 14, 6.5, 4.25)), (2, [14, 6.5, 4.25, 0.1], (14, 14, 6.5, 4.25)),
                                (4, [14, 13, 6.5, 4.25, 0.1, 0.01, 0, 0], (14, 13, 6.5, 4.25))):
        _rewrite_cameras(root, [(1, model, 12, 10, params)])
        assert C.Capture.load_colmap(root).intrinsics == want
    # two cameras with different parameters among the kept images
    ims = C.read_colmap_images(os.path.join(root, "sparse", "0", "images.bin"))
    blob = bytearray(open(os.path.join(root, "sparse", "0", "images.bin"), "rb").read())
    at = 8 + 4 + 56                                # count, the first image's id, q + t: its camera id
    assert int.from_bytes(blob[at:at + 4], "little") == ims[1]["camera_id"] == 1
    blob[at:at + 4] = (2).to_bytes(4, "little")
    open(os.path.join(root, "sparse", "0", "images.bin"), "wb").write(bytes(blob))
    _rewrite_cameras(root, [(1, 1, 12, 10, [14, 13, 6.5, 4.25]), (2, 1, 12, 10, [15, 13, 6.5, 4.25])])
    with pytest.raises(ValueError, match="one camera model per set"):
        C.Capture.load_colmap(root)
    _rewrite_cameras(root, [(1, 1, 12, 10, [14, 13, 6.5, 4.25]), (2, 1, 12, 10, [14, 13, 6.5, 4.25])])
    assert len(C.Capture.load_colmap(root, split="trainval")) == 9           # equal parameters: still one camera model
    # an image without its file is dropped, and the split moves with it
    os.remove(os.path.join(root, "images", "r_0.png"))
    assert len(C.Capture.load_colmap(root, split="trainval")) == 8 and len(C.Capture.load_colmap(root, split="val")) == 1
    # truncated file
    open(os.path.join(root, "sparse", "0", "points3D.bin"), "wb").write(open(os.path.join(TINY, "sparse", "0", "points3D.bin"), "rb").read()[:100])
    with pytest.raises(ValueError, match="truncated"):
        C.Capture.load_colmap(root)
