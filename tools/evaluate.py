#!/usr/bin/env python3
"""Held-out PSNR and SSIM of every stage's product on the same views: the field (stage-0 inference render), the stage-1 mesh
(render_stage1) and the exported asset loaded back from its files (asset.ExportedAsset.render), each against the ground truth on white.

    tools/evaluate.py [--iters0 N --iters1 N --views N --size S --lambda_ssim w]            the short synthetic pipeline (tools/eval_export.py's flow)
    tools/evaluate.py --data PATH [--data_format nerf|colmap|dtu] [--split test|val|...]   a captured set: trains on its train split, evaluates --split
    tools/evaluate.py --patch_size 16 [--lambda_patch_ssim w] [--field_only]                stage 0 on patch batches (the autograd trainer)
    tools/evaluate.py --lambda_distort w [--distort_space disparity] [--field_only]         stage 0 with the distortion loss (the autograd trainer)
    tools/evaluate.py --data PATH --optimize_poses [--lr_pose r]                            stage 0 refines the camera poses (writes OUT/poses_refined.npy)
    tools/evaluate.py --data PATH --mesh_method tsdf [--tsdf_trunc d] [--tsdf_carve]       the stage-0 mesh by TSDF fusion of rendered depth

With a checkpoint of the needed stage in OUT/checkpoints (--ckpt, default latest) the model is loaded instead of trained:
--iters0 0 / --iters1 0 are then legal, and the stage-1 file brings its mesh with it.

Prints one table row per view and stage, then one JSON line.  LPIPS, the reference's other meter, is not built (no VGG weights here)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from nerf2mesh_amd import checkpoint, export, metrics, synthetic as S, tsdf
from nerf2mesh_amd.asset import ExportedAsset
from nerf2mesh_amd.capture import Capture
from nerf2mesh_amd.engine import Stage0Engine
from nerf2mesh_amd.engine_stage1 import Stage1Engine
from nerf2mesh_amd.network import NeRFNetwork
from nerf2mesh_amd.options import make_options
from nerf2mesh_amd.trainer import Stage0Trainer, Stage1Trainer

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--out", default="bench_runs/evaluate")
ap.add_argument("--data", default=None, help="a captured set (default: the synthetic box scene)")
ap.add_argument("--data_format", choices=["nerf", "colmap", "dtu"], default="nerf")
ap.add_argument("--split", default=None, help="held-out split of --data (default: test for nerf, val for colmap / dtu)")
ap.add_argument("--downscale", type=int, default=1)
ap.add_argument("--undistort", action="store_true", help="colmap: undistort the images at load with the cameras' lens coefficients (DESIGN 4.26)")
ap.add_argument("--iters0", type=int, default=3000)
ap.add_argument("--iters1", type=int, default=300)
ap.add_argument("--resolution", type=int, default=256)
ap.add_argument("--texture", type=int, default=2048)
ap.add_argument("--views", type=int, default=8, help="held-out views")
ap.add_argument("--size", type=int, default=400, help="synthetic: side of the held-out frames")
ap.add_argument("--lambda_ssim", type=float, default=0.0, help="stage 1: weight of 1 - SSIM (0: the reference's loss)")
ap.add_argument("--patch_size", type=int, default=1, help="stage 0: batches of P x P patches instead of random pixels (1: pixels)")
ap.add_argument("--lambda_patch_ssim", type=float, default=0.0, help="stage 0: weight of 1 - SSIM over the batch's patches (needs --patch_size >= 11)")
ap.add_argument("--lambda_distort", type=float, default=0.0, help="stage 0: weight of the distortion loss of the ray weights (0: off; not a reference option)")
ap.add_argument("--distort_space", choices=["linear", "disparity"], default="linear", help="--lambda_distort: normalise the sample intervals in t or in 1 / t")
ap.add_argument("--optimize_poses", action="store_true", help="stage 0: train a correction per camera next to the field (needs --data; the autograd trainer, unfused field)")
ap.add_argument("--lr_pose", type=float, default=1e-3, help="--optimize_poses: learning rate of the corrections")
ap.add_argument("--mesh_method", choices=["density", "tsdf"], default="density", help="the stage-0 mesh: an iso-surface of the density lattice, or TSDF fusion of the depth rendered at every training camera (DESIGN 4.32; needs --data; not a reference option)")
ap.add_argument("--tsdf_trunc", type=float, default=0.0, help="--mesh_method tsdf: truncation distance in world units (0: four lattice spacings)")
ap.add_argument("--tsdf_carve", action="store_true", help="--mesh_method tsdf: rays that stop at nothing mark the points along them as empty")
ap.add_argument("--ckpt", default="latest", help="latest | scratch | best | PATH: a trained model of OUT/checkpoints instead of training")
ap.add_argument("--field_only", action="store_true", help="stop after the field's evaluation (no mesh, no stage 1, no export)")
args = ap.parse_args()
if args.optimize_poses and args.data is None:
    ap.error("--optimize_poses needs --data (the synthetic scene's poses are exact)")
if args.mesh_method == "tsdf" and args.data is None:
    ap.error("--mesh_method tsdf needs --data (the depth maps are rendered at a captured set's cameras)")
dev = torch.device("cuda", 0)
torch.manual_seed(0)

opt = make_options(O=True, bound=1, dt_gamma=0, iters=args.iters0, fused_mlp=not args.optimize_poses, lambda_ssim=args.lambda_ssim, data_format=args.data_format,
                   patch_size=args.patch_size, lambda_patch_ssim=args.lambda_patch_ssim, lambda_distort=args.lambda_distort,
                   distort_space=args.distort_space, optimize_poses=args.optimize_poses, lr_pose=args.lr_pose,
                   per_view_intrinsics=args.data_format == "dtu", undistort=args.undistort, workspace=args.out,
                   mesh_method=args.mesh_method, tsdf_trunc=args.tsdf_trunc, tsdf_carve=args.tsdf_carve)
model = NeRFNetwork(opt)
if args.data is None:
    cap, poses = None, S.make_cameras(100, seed=0)
    f = S.LEGO_FOCAL * args.size / S.LEGO_HW
    held = Capture.synthetic(S.make_cameras(args.views, seed=1), H=args.size, W=args.size, intrinsics=(f, f, args.size / 2, args.size / 2), device=dev)
    views = list(range(len(held)))
else:
    def load(split):
        if args.data_format == "dtu":
            return Capture.load_dtu(args.data, split=split, downscale=args.downscale, device=dev)
        if args.data_format == "colmap":
            c = Capture.load_colmap(args.data, split=split, downscale=args.downscale, device=dev, undistort=args.undistort)
            c.cam_near_far = None
            return c
        return Capture.load_nerf(args.data, split=split, downscale=args.downscale, device=dev)
    cap, poses = load("train"), None
    held = load(args.split or ("test" if args.data_format == "nerf" else "val"))
    views = list(range(0, len(held), max(1, len(held) // max(1, args.views))))[:args.views]
    if args.data_format == "colmap":
        model.to(dev)
        model.update_aabb(cap.pts_aabb.to(dev))

# ---- stage 0 -> mesh -> stage 1 -> files
pixels = args.patch_size == 1 and args.lambda_patch_ssim == 0 and args.lambda_distort == 0 and not args.optimize_poses   # patch batches, their SSIM term, the distortion term and pose refinement are the autograd trainer's
cls = Stage0Engine if (cap is None and pixels) or Stage0Engine.supported(model, opt, capture=cap) else Stage0Trainer
eng = cls(model, opt, poses, dev, seed=0, capture=cap)
eng.mark_untrained()
ckpt0, _ = checkpoint.restore_or_init(eng, args.out, args.ckpt)
saved_mesh = None if args.field_only else checkpoint.stage1_mesh(args.out, args.ckpt)
if ckpt0 is None and saved_mesh is None and args.iters0 <= 0:
    raise SystemExit(f"--iters0 0 needs a stage-0 checkpoint in {os.path.join(args.out, 'checkpoints')}")
todo0 = 0 if ckpt0 is not None or saved_mesh is not None else args.iters0
import time
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(todo0):
    eng.train_step()
torch.cuda.synchronize()
ms0 = (time.perf_counter() - t0) * 1e3 / max(1, todo0)
if ckpt0 is not None:
    print(f"[ckpt] stage 0: loaded {ckpt0} (step {eng.global_step}), nothing trained", flush=True)
print(f"[stage 0] {todo0} steps ({cls.__name__}, patch_size {args.patch_size}, lambda_patch_ssim {args.lambda_patch_ssim:g}, lambda_distort {args.lambda_distort:g} ({args.distort_space})): "
      f"{ms0:.3f} ms / step, "
      f"{eng.rays_seen / max(1, eng.global_step):.0f} rays / step", flush=True)
if args.optimize_poses:
    # the export and stage 1 see the training views where stage 0 left them; held-out views have no correction
    cap = eng.refiner.refined(cap)
    os.makedirs(args.out, exist_ok=True)
    np.save(os.path.join(args.out, "poses_refined.npy"), cap.poses.cpu().numpy())
    print(f"[poses] refined poses of {len(cap)} training views -> {os.path.join(args.out, 'poses_refined.npy')}; held-out views are evaluated with "
          f"their stored poses", flush=True)
model.eval()
with eng.averaged_parameters():
    field = metrics.evaluate_views(metrics.field_renderer(model, held), held, views)
if args.field_only:
    print(f"field: mean PSNR {field['mean_psnr']:.2f}, mean SSIM {field['mean_ssim']:.4f} over {len(views)} held-out views {held.H} x {held.W}")
    print(json.dumps({"views": views, "H": held.H, "W": held.W, "iters0": args.iters0, "patch_size": args.patch_size,
                      "lambda_patch_ssim": args.lambda_patch_ssim, "lambda_distort": args.lambda_distort, "distort_space": args.distort_space,
                      "stage0_ms_per_step": round(ms0, 4), "stage0_driver": cls.__name__,
                      "field": {k: field[k] for k in ("psnr", "ssim", "mean_psnr", "mean_ssim")}}))
    sys.exit(0)
opt.stage, opt.iters = 1, max(args.iters1, 501)
if saved_mesh is not None:              # the stage-1 file brings its mesh with it
    rt = saved_mesh[1]
    tr = Stage1Trainer(model, opt, poses, saved_mesh[0], rt, dev, capture=cap, v_cumsum=saved_mesh[2], f_cumsum=saved_mesh[3])
else:
    with eng.averaged_parameters():
        model.export_stage0(os.path.join(args.out, "mesh_stage0"), resolution=args.resolution, **({} if cap is None else dict(dataset=cap, clean=True, decimate=True)),
                            **tsdf.export_options(opt))
    rv, rt = export.read_ply(os.path.join(args.out, "mesh_stage0", "mesh_0.ply"))
    tr = Stage1Trainer(model, opt, poses, torch.from_numpy(rv), torch.from_numpy(rt), dev, capture=cap)
drv = Stage1Engine(tr) if Stage1Engine.supported(tr) else tr
mode1 = checkpoint.restore_or_init(drv, args.out, args.ckpt)[1] if saved_mesh is not None else None
todo1 = 0 if mode1 == "full" else args.iters1
for _ in range(todo1):
    drv.train_step()
torch.cuda.synchronize()
model.eval()
print(f"[pipeline] stage 0: {todo0} steps ({cls.__name__}); stage 1: {todo1} steps on {rt.shape[0]} faces, lambda_ssim {args.lambda_ssim:g} "
      f"({'executor' if Stage1Engine.supported(tr) else 'autograd trainer'}); {len(views)} held-out views {held.H} x {held.W}", flush=True)
mesh = metrics.evaluate_views(metrics.mesh_renderer(model, held), held, views)
out_dir = os.path.join(args.out, "mesh_stage1")
model.export_stage1(out_dir, args.texture, args.texture, atlas="charts")
asset = metrics.evaluate_views(metrics.asset_renderer(ExportedAsset.load(out_dir), held, ssaa=int(opt.ssaa)), held, views)

stages = (("field", field), ("mesh", mesh), ("asset", asset))
print(f"{'view':>5s} " + " ".join(f"{n + ' PSNR':>11s} {n + ' SSIM':>11s}" for n, _ in stages))
for k, v in enumerate(views):
    print(f"{v:5d} " + " ".join(f"{ev['psnr'][k]:11.2f} {ev['ssim'][k]:11.4f}" for _, ev in stages))
print(f"{'mean':>5s} " + " ".join(f"{ev['mean_psnr']:11.2f} {ev['mean_ssim']:11.4f}" for _, ev in stages), flush=True)
print(json.dumps({"views": views, "H": held.H, "W": held.W, "iters0": args.iters0, "iters1": args.iters1, "lambda_ssim": args.lambda_ssim,
                  "faces": int(rt.shape[0]), **{n: {k: ev[k] for k in ("psnr", "ssim", "mean_psnr", "mean_ssim")} for n, ev in stages}}))
