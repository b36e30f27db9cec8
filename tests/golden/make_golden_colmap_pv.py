#!/usr/bin/env python3
"""Generates tests/golden/colmap_pv.npz: what the reference makes of the tiny COLMAP reconstruction when its nine images use three
different cameras (tests/test_per_view_io.py writes that set: a copy of tests/golden/colmap_tiny with cameras.bin and the images' camera
ids rewritten).

The reference side is the UNCHANGED nerf/colmap_provider.py, driven exactly as tests/golden/make_golden_colmap.py drives it (its PIL-backed
cv2 stand-in is imported from there).  Recorded at downscale 1 and 2 (auto-scale): the fp32 intrinsics [N,4] the class stores, its poses,
H and W, and the train / val index lists at downscale 1.

Needs the reference checkout (build container only).      python tests/golden/make_golden_colmap_pv.py
"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import make_golden_colmap as G          # noqa: E402  (main guard: importing it generates nothing)
import test_per_view_io as T            # noqa: E402  (the set under test is written by the test's own helpers)


def run_reference(mod, root, split, downscale):
    opt = types.SimpleNamespace(downscale=downscale, preload=False, scale=-1, fp16=False, path=root, enable_cam_center=False, bound=1,
                                enable_sparse_depth=True, enable_dense_depth=False, min_near=0.05, vis_pose=False, camera_traj="", stage=0)
    return mod.ColmapDataset(opt, "cpu", type=split)


def main():
    mod = G.reference_module()
    fx = {}
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "rec")
        ids = T.write_pv_copy(root)
        for tag, ds in (("", 1), ("ds2_", 2)):
            d = run_reference(mod, root, "trainval", ds)
            assert len(d.poses) == 9
            fx[tag + "poses"] = d.poses.numpy()
            fx[tag + "intrinsics"] = d.intrinsics.numpy()
            fx[tag + "HW"] = np.array([d.H, d.W])
        allp = fx["poses"]
        for split in ("train", "val"):
            p = run_reference(mod, root, split, 1).poses.numpy()
            fx[split + "_ids"] = np.array([int(np.nonzero((allp == q).all((1, 2)))[0][0]) for q in p])
        fx["camera_ids"] = np.array(ids)
    assert fx["intrinsics"].dtype == np.float32
    path = os.path.join(HERE, "colmap_pv.npz")
    np.savez_compressed(path, **fx)
    print(f"colmap_pv: 9 views, cameras {ids}, train {fx['train_ids'].tolist()}, val {fx['val_ids'].tolist()}; npz {os.path.getsize(path) / 1024:.1f} KiB")
    print(fx["intrinsics"])


if __name__ == "__main__":
    main()
