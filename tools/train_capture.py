#!/usr/bin/env python3
"""Both stages on a captured image set in the nerf format (transforms_{train,test}.json or transforms.json + images), with
--data_format colmap on a COLMAP reconstruction (colmap_sparse/0 | sparse/0 | colmap + images[_k]/; capture.Capture.load_colmap), or with
--data_format dtu on a DTU scan (cameras_sphere.npz + image/ + mask/; capture.Capture.load_dtu):

    tools/train_capture.py PATH --workspace DIR [--iters0 N --iters1 N --downscale k --scale s --bound b --color_space srgb|linear]
                           [--data_format colmap [--enable_sparse_depth | --enable_dense_depth] [--lambda_depth w] [--enable_cam_near_far] [--enable_cam_center]
                                                 [--per_view_intrinsics] [--undistort]]
                           [--data_format dtu]
                           [--test [--test_no_video] [--camera_traj circle] [--n_test N]]
                           [--ckpt latest|scratch|best|PATH] [--n_ckpt N]

  colmap: --scale defaults to -1 (1 / the nearest camera's distance), the model's training box is the sparse points' (update_aabb,
  main.py:234-235), --enable_cam_near_far clamps every ray to its view's keypoint depth range, --enable_sparse_depth makes one step in
  ten a depth step, --enable_dense_depth puts a depth target from PATH/depths/NAME.npy on every ray of every step, and the held-out views are the `val` split (every 8th image).
  --per_view_intrinsics accepts a reconstruction whose images use different cameras (COLMAP without --single_camera): one (fx, fy, cx, cy)
  row per view.  --undistort uses the cameras' lens coefficients (SIMPLE_RADIAL, RADIAL, OPENCV, OPENCV_FISHEYE): the bank is resampled once,
  on the device, to a pinhole camera; without it the coefficients are ignored, as the reference does.
  dtu: every view has its own K (per-view intrinsics are implied), --scale defaults to 1, the masks supply alpha, and the held-out view is
  the `val` split (the first frame).

  load (capture.Capture.load_nerf: the train split, and the test split if PATH has one) -> stage 0 (step executor on the uint8 bank)
  -> export_stage0(dataset=capture, clean, decimate) -> stage 1 on that mesh (views from the capture) -> export_stage1(atlas="charts")
  -> one JSON line: held-out PSNR of both stages (the test split; without one, the training views) and evaluate_export of the written files.
     `train_loss_tail` is the mean stage-0 training loss over the last 100 steps and `ind_dim` the code width (--ind_dim): two runs of the same
     schedule and seed with --ind_dim 0 and 8 report what the per-image codes buy on a set whose exposure varies.

  --test: after training, test mode (the reference's `main.py --test`): a path of cameras that are not in the set -- the
  interpolation between 5 random training views with N + 1 frames per segment, or with --camera_traj circle the reference's circle -- is
  rendered from the stage-1 mesh and written to WORKSPACE/results as {name}_{i:04d}_rgb.png / _depth.png, and as animated PNGs
  ({name}_rgb.apng, {name}_depth.apng: the stand-in for the reference's mp4) unless --test_no_video.

  --ckpt (default latest): each stage resumes from the newest checkpoint of its stage in WORKSPACE/checkpoints and trains the
  steps that are left of --iters0 / --iters1; without one it starts from scratch (stage 1: from the newest stage-0 file).  --n_ckpt N saves
  every N steps; every stage saves when it ends.  With --test and a checkpoint present nothing is trained.

Reads nothing but PATH; writes under --workspace.  With --bound > 1 stage 1 refines the inner mesh (cascade 0) only, except under --sdf:
`--sdf --bound 2` is the SDF recipe on an unbounded scene (contracted background), export_stage0 then writes the outer shell as mesh_1.ply
and stage 1 loads both files (export.load_stage0_meshes; one cascade when the shell came out empty).  That recipe switches the offset
gradient on, which the stage-1 executor does not cover: its stage 1 runs on the autograd trainer."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from nerf2mesh_amd import checkpoint, tsdf
from nerf2mesh_amd.asset import ExportedAsset, evaluate_export, psnr
from nerf2mesh_amd.capture import Capture
from nerf2mesh_amd.engine import Stage0Engine
from nerf2mesh_amd.engine_stage1 import Stage1Engine
from nerf2mesh_amd.network import NeRFNetwork
from nerf2mesh_amd.options import make_options
from nerf2mesh_amd.trainer import Stage0Trainer, Stage1Trainer

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("path")
ap.add_argument("--workspace", required=True)
ap.add_argument("--iters0", type=int, default=30000)
ap.add_argument("--iters1", type=int, default=10000)
ap.add_argument("--downscale", type=int, default=1)
ap.add_argument("--scale", type=float, default=None, help="default: 0.33 (nerf), -1 = automatic (colmap), 1 (dtu)")
ap.add_argument("--data_format", choices=["nerf", "colmap", "dtu"], default="nerf")
ap.add_argument("--per_view_intrinsics", action="store_true", help="colmap: one (fx, fy, cx, cy) row per view when the images' cameras differ; dtu implies it")
ap.add_argument("--undistort", action="store_true", help="colmap: undistort the images at load with the cameras' lens coefficients (pinhole from then on)")
ap.add_argument("--enable_sparse_depth", action="store_true")
ap.add_argument("--enable_dense_depth", action="store_true", help="every step supervises depth from PATH/depths/NAME.npy (calibrated per view)")
ap.add_argument("--enable_cam_near_far", action="store_true")
ap.add_argument("--enable_cam_center", action="store_true")
ap.add_argument("--lambda_depth", type=float, default=0.1)
ap.add_argument("--offset", type=float, nargs=3, default=[0, 0, 0])
ap.add_argument("--bound", type=float, default=1)
ap.add_argument("--sdf", action="store_true", help="the SDF recipe (main.py:138-153); with --bound > 1 the scene is contracted and the outer shell exported")
ap.add_argument("--color_space", choices=["srgb", "linear"], default="srgb")
ap.add_argument("--resolution", type=int, default=None, help="marching-cubes resolution (default: the occupancy grid's)")
ap.add_argument("--decimate_target", type=float, default=3e5)
ap.add_argument("--texture", type=int, default=2048)
ap.add_argument("--eval_views", type=int, default=8, help="held-out views the PSNRs are averaged over")
ap.add_argument("--ind_dim", type=int, default=0, help="per-image appearance code width (0 = off); up to 16 runs the fused field kernels")
ap.add_argument("--ind_num", type=int, default=500, help="code rows; at least the number of training views")
ap.add_argument("--patch_size", type=int, default=1, help="stage 0: batches of P x P patches instead of random pixels (the autograd trainer)")
ap.add_argument("--lambda_patch_ssim", type=float, default=0.0, help="stage 0: weight of 1 - SSIM over the batch's patches (needs --patch_size 11 .. 64)")
ap.add_argument("--lambda_distort", type=float, default=0.0, help="stage 0: weight of the distortion loss of the ray weights (not a reference option; the autograd trainer)")
ap.add_argument("--distort_space", choices=["linear", "disparity"], default="linear", help="--lambda_distort: normalise the sample intervals in t or in 1 / t")
ap.add_argument("--optimize_poses", action="store_true", help="stage 0: train a correction (rotation, translation) per camera next to the field (not a reference option; the autograd trainer, unfused field)")
ap.add_argument("--lr_pose", type=float, default=1e-3, help="--optimize_poses: learning rate of the corrections")
ap.add_argument("--mesh_method", choices=["density", "tsdf"], default="density", help="the stage-0 mesh: an iso-surface of the density lattice, or TSDF fusion of the depth rendered at every training camera (DESIGN 4.32; not a reference option)")
ap.add_argument("--tsdf_trunc", type=float, default=0.0, help="--mesh_method tsdf: truncation distance in world units (0: four lattice spacings)")
ap.add_argument("--tsdf_carve", action="store_true", help="--mesh_method tsdf: rays that stop at nothing mark the points along them as empty")
ap.add_argument("--test", action="store_true", help="after training, render a test-time camera path from the stage-1 mesh into WORKSPACE/results")
ap.add_argument("--test_no_video", action="store_true", help="--test: frames only, no animated PNGs")
ap.add_argument("--camera_traj", choices=["", "circle"], default="", help="--test: the path (default: interpolate between random training views)")
ap.add_argument("--n_test", type=int, default=24, help="--test: frames per segment of the interpolated path, less one")
ap.add_argument("--ckpt", default="latest", help="latest | scratch | best | PATH: where each stage starts from (default: the newest checkpoint of the workspace)")
ap.add_argument("--n_ckpt", type=int, default=0, help="save a checkpoint every N steps (0: only when a stage ends)")
ap.add_argument("--seed", type=int, default=0)
args = ap.parse_args()
dev = torch.device("cuda", 0)
torch.manual_seed(args.seed)
linear = args.color_space == "linear"
colmap, dtu = args.data_format == "colmap", args.data_format == "dtu"
if dtu:
    args.per_view_intrinsics = True
elif args.per_view_intrinsics and not colmap:
    ap.error("--per_view_intrinsics needs --data_format colmap or dtu (the nerf format states one camera)")
if args.undistort and not colmap:
    ap.error("--undistort needs --data_format colmap (the other formats state no lens)")
if args.scale is None:
    args.scale = -1 if colmap else 1 if dtu else 0.33
if not colmap and (args.enable_sparse_depth or args.enable_dense_depth or args.enable_cam_near_far or args.enable_cam_center):
    ap.error("--enable_sparse_depth / --enable_dense_depth / --enable_cam_near_far / --enable_cam_center need --data_format colmap (the sparse "
             "points supply them)")
if args.enable_sparse_depth and args.enable_dense_depth:
    ap.error("--enable_sparse_depth and --enable_dense_depth exclude each other")
if args.optimize_poses and args.sdf:
    ap.error("--optimize_poses does not run with --sdf")
if args.mesh_method == "tsdf" and args.sdf:
    ap.error("--mesh_method tsdf does not run with --sdf (the SDF recipe already meshes a signed distance)")


def clock(label, t0, extra=""):
    torch.cuda.synchronize()
    print(f"[{label}] {time.perf_counter() - t0:8.3f} s  {extra}", flush=True)


def load(split):
    if dtu:
        return Capture.load_dtu(args.path, split=split, scale=args.scale, offset=args.offset, downscale=args.downscale, linear=linear, device=dev)
    if not colmap:
        return Capture.load_nerf(args.path, split=split, scale=args.scale, offset=args.offset, downscale=args.downscale, linear=linear, device=dev)
    c = Capture.load_colmap(args.path, split=split, scale=args.scale, downscale=args.downscale, linear=linear,
                            enable_cam_center=args.enable_cam_center, sparse_depth=args.enable_sparse_depth and split == "train",
                            dense_depth=args.enable_dense_depth and split == "train", device=dev, per_view_intrinsics=args.per_view_intrinsics,
                            undistort=args.undistort)
    if not args.enable_cam_near_far:
        c.cam_near_far = None
    return c


t0 = time.perf_counter()
cap = load("train")
if colmap or dtu:
    held = load("val")
else:
    held = load("test") if os.path.exists(os.path.join(args.path, "transforms_test.json")) else cap
views = list(range(0, len(held), max(1, len(held) // max(1, args.eval_views))))[:args.eval_views]
clock("load", t0, f"{len(cap)} training views {cap.H} x {cap.W} ({cap.nbytes / 1e6:.1f} MB as uint8, {'RGBA' if cap.has_alpha else 'RGB'}), "
      f"{len(held) if held is not cap else 0} held-out views")

# ---- stage 0
opt = make_options(O=True, bound=args.bound, dt_gamma=0 if args.bound <= 1 else 1 / 256, iters=args.iters0, fused_mlp=not args.optimize_poses, scale=args.scale,
                   offset=list(args.offset), color_space=args.color_space, decimate_target=args.decimate_target, workspace=args.workspace,
                   data_format=args.data_format, enable_sparse_depth=args.enable_sparse_depth, enable_dense_depth=args.enable_dense_depth,
                   enable_cam_near_far=args.enable_cam_near_far, per_view_intrinsics=args.per_view_intrinsics, undistort=args.undistort,
                   lambda_depth=args.lambda_depth, ind_dim=args.ind_dim, ind_num=args.ind_num, sdf=args.sdf,
                   patch_size=args.patch_size, lambda_patch_ssim=args.lambda_patch_ssim, lambda_distort=args.lambda_distort,
                   distort_space=args.distort_space, optimize_poses=args.optimize_poses, lr_pose=args.lr_pose, camera_traj=args.camera_traj,
                   mesh_method=args.mesh_method, tsdf_trunc=args.tsdf_trunc, tsdf_carve=args.tsdf_carve)
model = NeRFNetwork(opt)
if colmap:
    model.to(dev)
    model.update_aabb(cap.pts_aabb.to(dev))              # main.py:234-235
cls = Stage0Engine if Stage0Engine.supported(model, opt, capture=cap) else Stage0Trainer
eng = cls(model, opt, None, dev, seed=args.seed, capture=cap)
eng.mark_untrained()
ckpt0, mode0 = checkpoint.restore_or_init(eng, args.workspace, args.ckpt)
todo0 = 0 if args.test and ckpt0 is not None else max(0, args.iters0 - eng.global_step)
print(f"[ckpt] stage 0: {'from scratch' if ckpt0 is None else f'{ckpt0} ({mode0}) at step {eng.global_step}'}, {todo0} steps to train", flush=True)
t0 = time.perf_counter()
tail0 = []                                   # the last training losses of stage 0 (device scalars): what two runs with and without --ind_dim compare
for _ in range(todo0):
    tail0.append(eng.train_step().detach().reshape(()).clone())
    if len(tail0) > 100:
        tail0.pop(0)
    if args.n_ckpt > 0 and eng.global_step % args.n_ckpt == 0:
        checkpoint.save_checkpoint(eng, args.workspace)
if todo0 > 0:
    checkpoint.save_checkpoint(eng, args.workspace)
train_loss_tail = float(torch.stack(tail0).mean()) if tail0 else float("nan")
psnr0 = [eng.eval_psnr(cam=v, downscale=1, use_ema=True, capture=held) for v in views]
clock("stage 0", t0, f"{todo0} steps ({cls.__name__}), held-out PSNR {np.mean(psnr0):.2f} dB")
if args.optimize_poses:
    # the mesh export, stage 1 and the camera paths see the training views where stage 0 left them; held-out views have no correction
    cap = eng.refiner.refined(cap)
    os.makedirs(args.workspace, exist_ok=True)
    np.save(os.path.join(args.workspace, "poses_refined.npy"), cap.poses.cpu().numpy())
    moved = eng.refiner.delta.detach().abs().amax(0).cpu().numpy()
    print(f"[poses] refined poses of {len(cap)} training views -> {os.path.join(args.workspace, 'poses_refined.npy')} (largest |omega| component "
          f"{moved[:3].max():.3g} rad, largest |tau| component {moved[3:].max():.3g}); held-out views are evaluated with their stored poses", flush=True)

t0 = time.perf_counter()
saved_mesh = checkpoint.stage1_mesh(args.workspace, args.ckpt)          # a stage-1 checkpoint brings its mesh with it
if saved_mesh is None:
    with eng.averaged_parameters():          # the mesh comes from the averaged weights, like the reference's (nerf/utils.py:1340-1341)
        meshes = model.export_stage0(os.path.join(args.workspace, "mesh_stage0"), resolution=args.resolution, decimate_target=args.decimate_target,
                                     dataset=cap, clean=True, decimate=True, **tsdf.export_options(opt))
    v0, f0 = meshes[0]
    clock("export_stage0", t0, f"{v0.shape[0]} vertices, {f0.shape[0]} triangles ({'TSDF fusion, ' if opt.mesh_method == 'tsdf' else ''}visibility filter, clean, decimate)")
    if f0.shape[0] == 0:
        raise SystemExit("export_stage0 left no face: stage 0 has not found the object (more --iters0, or check --scale / --bound)")

# ---- stage 1
opt.stage, opt.iters = 1, max(args.iters1, 501)
if saved_mesh is not None:
    v0, f0, v_cumsum, f_cumsum = saved_mesh
    tr = Stage1Trainer(model, opt, None, v0, f0, dev, seed=args.seed, capture=cap, v_cumsum=v_cumsum, f_cumsum=f_cumsum)
elif opt.sdf and model.cascade > 1:          # the contracted recipe: every cascade export_stage0 wrote (mesh_0.ply, and mesh_1.ply unless the shell was empty)
    from nerf2mesh_amd import export
    va, fa, v_cumsum, f_cumsum = export.load_stage0_meshes(os.path.join(args.workspace, "mesh_stage0"), model.cascade)
    print(f"[stage 1] {len(v_cumsum) - 1} cascade(s): vertices {v_cumsum}, faces {f_cumsum}", flush=True)
    tr = Stage1Trainer(model, opt, None, torch.from_numpy(va), torch.from_numpy(fa), dev, seed=args.seed, capture=cap, v_cumsum=v_cumsum,
                       f_cumsum=f_cumsum)
else:
    tr = Stage1Trainer(model, opt, None, v0, f0, dev, seed=args.seed, capture=cap)
drv = Stage1Engine(tr) if Stage1Engine.supported(tr) else tr
ckpt1, mode1 = checkpoint.restore_or_init(drv, args.workspace, args.ckpt)
todo1 = 0 if args.test and (mode1 == "full" or ckpt0 is not None) else max(0, args.iters1 - tr.global_step)
print(f"[ckpt] stage 1: {'from the stage-0 model in memory' if ckpt1 is None else f'{ckpt1} ({mode1}) at step {tr.global_step}'}, {todo1} steps to train", flush=True)
t0 = time.perf_counter()
for _ in range(todo1):
    drv.train_step()
    if args.n_ckpt > 0 and tr.global_step % args.n_ckpt == 0:
        checkpoint.save_checkpoint(drv, args.workspace)
if todo1 > 0:
    checkpoint.save_checkpoint(drv, args.workspace)
f0 = model.triangles
model.eval()
psnr1, eval_views = [], []
with torch.no_grad():
    for v in views:
        _, rays_d, rgba, _ = held.view(v)
        gt = rgba[:, :3] * rgba[:, 3:] + (1 - rgba[:, 3:])
        psnr1.append(psnr(model.render_stage1(None, rays_d, held.mvps[v], held.H, held.W)["image"].view(-1, 3), gt))
        eval_views.append((rays_d, held.mvps[v]))
clock("stage 1", t0, f"{todo1} steps on {f0.shape[0]} faces, held-out PSNR {np.mean(psnr1):.2f} dB")

t0 = time.perf_counter()
out_dir = os.path.join(args.workspace, "mesh_stage1")
model.export_stage1(out_dir, h0=args.texture, w0=args.texture, atlas="charts")
ev = evaluate_export(model, ExportedAsset.load(out_dir), eval_views, held.H, held.W)
clock("export_stage1", t0, "files: " + ", ".join(sorted(os.listdir(out_dir))))

test_frames = 0
if args.test:
    from nerf2mesh_amd import camera_path, metrics
    t0 = time.perf_counter()
    path = camera_path.path_for(cap, opt, n_test=args.n_test, seed=args.seed)
    rgb, depth = camera_path.render_path(metrics.mesh_renderer(model, path), path, linear=linear)
    camera_path.save_frames(rgb, depth, os.path.join(args.workspace, "results"), "ngp_stage1", video=None if args.test_no_video else "apng")
    test_frames = len(path)
    clock("test", t0, f"{test_frames} frames {path.H} x {path.W} of the {'circle' if args.camera_traj else 'interpolated'} path -> {os.path.join(args.workspace, 'results')}")

depth_steps = sum(v is not None for v in eng.depth_schedule.log[:args.iters0]) if getattr(eng, "depth_schedule", None) is not None else 0
if args.enable_dense_depth:
    depth_steps = args.iters0                  # every step carries the depth term
print(json.dumps({"data_format": args.data_format, "test_frames": test_frames, "ind_dim": args.ind_dim, "train_loss_tail": train_loss_tail, "per_view_intrinsics": bool(cap.per_view_intrinsics), "depth_steps": depth_steps, "train_views": len(cap), "held_out_views": len(views), "held_out_is_test_split": held is not cap, "H": cap.H, "W": cap.W,
                  "bank_mb": round(cap.nbytes / 1e6, 3), "iters0": args.iters0, "iters1": args.iters1, "trained0": todo0, "trained1": todo1, "resumed0": ckpt0, "resumed1": ckpt1 if mode1 == "full" else None, "faces": int(f0.shape[0]),
                  "psnr_stage0": float(np.mean(psnr0)), "psnr_stage1": float(np.mean(psnr1)), "export_psnr_vs_stage1": ev["mean"],
                  "export_psnr_per_view": ev["psnr_vs_stage1"]}))
