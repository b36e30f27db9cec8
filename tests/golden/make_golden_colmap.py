#!/usr/bin/env python3
"""Generates tests/golden/colmap_tiny/ (a tiny COLMAP reconstruction written by capture.Capture.save_colmap) and tests/golden/colmap_tiny.npz
(what the reference makes of it).

The reconstruction: 9 views of the box scene, 12 x 10 px, one PINHOLE camera with fx != fy and an off-centre principal point, 40 points
with errors that differ; besides the projections of the points every view carries keypoints without a 3D point and keypoints (with a 3D
point) outside the image.  images_2/ holds the same views reduced by capture.box_downscale, so that the reference -- whose resize is cv2's
-- can be run at downscale 2 as well.

The reference side is the UNCHANGED nerf/colmap_provider.py: `ColmapDataset.__init__` (which calls colmap_utils.read_cameras_binary /
read_images_binary / read_points3d_binary and center_poses) is driven as it is, once per split and downscale.  cv2 is absent here, so the
module's `cv2` is a PIL-backed stand-in (imread returning BGR[A] as cv2 does, cvtColor swapping back; resize refuses, no image needs it).
Recorded (auto-scale at downscale 1 and 2, and --enable_cam_center at scale 0.5): poses and intrinsics (the fp32 the class stores), pts3d
and pts_aabb (float64), cam_near_far, per-view coords / depth / weight, and the train / val index lists (positions in the sorted, existing image list).

Needs the reference checkout (build container only).      python tests/golden/make_golden_colmap.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_python as RP                          # noqa: E402
from nerf2mesh_amd import capture as C, synthetic as S       # noqa: E402

OUT = os.path.join(HERE, "colmap_tiny")
H, W = 10, 12
INTR = (14.0, 13.0, 6.5, 4.25)
V, M = 9, 40


def write_reconstruction():
    rng = np.random.default_rng(7)
    poses = S.make_cameras(V, seed=3)
    cap = C.Capture.synthetic(poses, scene="lego", H=H, W=W, intrinsics=INTR, alpha=False)
    points = rng.uniform(-0.8, 0.8, (M, 3))               # wide enough that no view sees them all
    errors = rng.uniform(0.2, 2.5, M)
    cap.save_colmap(OUT, points, errors=errors)
    ims = C.read_colmap_images(os.path.join(OUT, "sparse", "0", "images.bin"))
    kps = []
    for k in sorted(ims):
        xy, ids = ims[k]["xys"], ims[k]["point3D_ids"] - 1           # save_colmap numbers the points from 1
        assert len(ids) >= 3, "every view must see some points"
        n_free, n_out = 3, 2
        free = np.stack([rng.uniform(0, W, n_free), rng.uniform(0, H, n_free)], -1)          # no 3D point
        out = np.stack([rng.choice([-1.75, W + 0.5], n_out), rng.uniform(0, H, n_out)], -1)  # a 3D point, but left / right of the image
        out[0, 1] = H + 1.25                                                                 # ... and one below it
        kps.append((np.concatenate([xy, free, out]), np.concatenate([ids, -np.ones(n_free, np.int64), rng.integers(0, M, n_out)])))
    cap.save_colmap(OUT, points, errors=errors, keypoints=kps)
    # the same views at half size, for the reference's downscale = 2 run
    from PIL import Image
    os.makedirs(os.path.join(OUT, "images_2"), exist_ok=True)
    half = C.box_downscale(cap.bank, H, W, 2).view(torch.uint8).view(V, H // 2, W // 2, 4).numpy()
    for v in range(V):
        Image.fromarray(np.ascontiguousarray(half[v, :, :, :3])).save(os.path.join(OUT, "images_2", f"r_{v}.png"))
    return cap


def reference_module():
    assert os.path.isdir(RP.REFERENCE), "needs the reference checkout"
    RP._install_stubs()
    if RP.REFERENCE not in sys.path:
        sys.path.insert(0, RP.REFERENCE)
    cv2 = sys.modules["cv2"]
    from PIL import Image

    def imread(name, flags=None):
        a = np.asarray(Image.open(name))
        return a[..., [2, 1, 0] + ([3] if a.shape[-1] == 4 else [])] if a.ndim == 3 else a

    def resize(image, size, interpolation=None):
        raise AssertionError("the stand-in cv2 does not resize; give the run an images_{downscale} folder")

    cv2.imread, cv2.resize = imread, resize
    cv2.cvtColor = lambda a, code: a[..., code]
    cv2.IMREAD_UNCHANGED, cv2.INTER_AREA, cv2.COLOR_BGR2RGB, cv2.COLOR_BGRA2RGBA = -1, 3, [2, 1, 0], [2, 1, 0, 3]
    import importlib
    return importlib.import_module("nerf.colmap_provider")


def run_reference(mod, split, downscale, cam_center=False, scale=-1):
    opt = types.SimpleNamespace(downscale=downscale, preload=False, scale=scale, fp16=False, path=OUT, enable_cam_center=cam_center, bound=1,
                                enable_sparse_depth=True, enable_dense_depth=False, min_near=0.05, vis_pose=False, camera_traj="", stage=0)
    return mod.ColmapDataset(opt, "cpu", type=split)


def main():
    write_reconstruction()
    mod = reference_module()
    fx = {}
    for tag, ds, cc, sc in (("", 1, False, -1), ("ds2_", 2, False, -1), ("cc_", 1, True, 0.5)):
        d = run_reference(mod, "trainval", ds, cc, sc)
        n = len(d.poses)
        assert n == V
        fx[tag + "poses"] = d.poses.numpy()
        fx[tag + "intrinsics"] = d.intrinsics.numpy()
        fx[tag + "HW"] = np.array([d.H, d.W])
        fx[tag + "scale"] = np.float64(d.scale)
        fx[tag + "pts_aabb"] = np.asarray(d.pts_aabb, dtype=np.float64)
        fx[tag + "pts3d"] = np.asarray(d.pts3d, dtype=np.float64)
        fx[tag + "cam_near_far"] = d.cam_near_far.numpy()
        fx[tag + "images"] = d.images.numpy()
        fx[tag + "offsets"] = np.concatenate([[0], np.cumsum([len(s[1]) for s in d.sparse_depth_info])]).astype(np.int32)
        fx[tag + "coords"] = np.concatenate([s[0].numpy() for s in d.sparse_depth_info]).astype(np.int32)
        fx[tag + "depth"] = np.concatenate([s[1].numpy() for s in d.sparse_depth_info])
        fx[tag + "weight"] = np.concatenate([s[2].numpy() for s in d.sparse_depth_info])
        if tag == "":
            allp = d.poses.numpy()
            for split in ("train", "val"):
                p = run_reference(mod, split, 1).poses.numpy()
                fx[split + "_ids"] = np.array([int(np.nonzero((allp == q).all((1, 2)))[0][0]) for q in p])
    path = os.path.join(HERE, "colmap_tiny.npz")
    np.savez_compressed(path, **fx)
    size = sum(os.path.getsize(os.path.join(dp, f)) for dp, _, fs in os.walk(OUT) for f in fs)
    print(f"colmap_tiny: {V} views {H} x {W}, {M} points, {fx['offsets'][-1]} depth keypoints, train {fx['train_ids'].tolist()}, val "
          f"{fx['val_ids'].tolist()}, scale {float(fx['scale']):.4f}; reconstruction {size / 1024:.1f} KiB, npz {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
