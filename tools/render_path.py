#!/usr/bin/env python3
"""Test mode: renders a path of cameras that are not in the set and writes the frames -- the reference's `main.py --test`.

    tools/render_path.py WORKSPACE [--source field|mesh|asset] [--camera_traj circle] [--n_test N] [--video apng]
                                   [--iters0 N --iters1 N --views V --size S [--width W]]          the short synthetic pipeline
                                   [--ckpt latest|scratch|best|PATH]                               a trained model of WORKSPACE/checkpoints
    tools/render_path.py WORKSPACE --data PATH [--data_format nerf|colmap|dtu] [--downscale k] ...   a captured set (its train split)

With a checkpoint of the needed stage in WORKSPACE/checkpoints (tools/train_capture.py writes them; --ckpt, default latest) the model is
loaded and nothing is trained -- --iters0 0 / --iters1 0 are then legal, and for --source mesh / asset the stage-1 file brings its mesh with it.
Otherwise: trains stage 0 (and, for --source mesh / asset, extracts the mesh, runs stage 1 and, for asset, exports and loads the files back), builds
the path -- by default the sine-eased interpolation between 5 random training views with N + 1 frames per segment (CameraPath.between),
with --camera_traj circle the reference's small circle of 100 look-at poses -- renders every frame from the chosen product and writes
WORKSPACE/results/{name}_{i:04d}_rgb.png and _depth.png; --video apng adds {name}_rgb.apng and {name}_depth.apng (animated PNG: the stand-in
for the reference's mp4).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from nerf2mesh_amd import camera_path, checkpoint, export, metrics, synthetic as S
from nerf2mesh_amd.asset import ExportedAsset
from nerf2mesh_amd.capture import Capture
from nerf2mesh_amd.engine import Stage0Engine
from nerf2mesh_amd.engine_stage1 import Stage1Engine
from nerf2mesh_amd.network import NeRFNetwork
from nerf2mesh_amd.options import make_options
from nerf2mesh_amd.trainer import Stage0Trainer, Stage1Trainer

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("workspace")
ap.add_argument("--source", choices=["field", "mesh", "asset"], default="field")
ap.add_argument("--camera_traj", choices=["", "circle"], default="")
ap.add_argument("--n_test", type=int, default=24, help="frames per segment of the interpolated path, less one")
ap.add_argument("--video", choices=["apng"], default=None)
ap.add_argument("--name", default="ngp")
ap.add_argument("--data", default=None, help="a captured set (default: the synthetic box scene)")
ap.add_argument("--data_format", choices=["nerf", "colmap", "dtu"], default="nerf")
ap.add_argument("--downscale", type=int, default=1)
ap.add_argument("--undistort", action="store_true", help="colmap: undistort the images at load (DESIGN 4.26)")
ap.add_argument("--color_space", choices=["srgb", "linear"], default="srgb")
ap.add_argument("--iters0", type=int, default=3000)
ap.add_argument("--iters1", type=int, default=300)
ap.add_argument("--resolution", type=int, default=256)
ap.add_argument("--texture", type=int, default=2048)
ap.add_argument("--views", type=int, default=100, help="synthetic: training views")
ap.add_argument("--size", type=int, default=400, help="synthetic: height of the frames (and width, without --width)")
ap.add_argument("--width", type=int, default=None)
ap.add_argument("--ckpt", default="latest", help="latest | scratch | best | PATH (default: the newest checkpoint of the workspace, if there is one)")
ap.add_argument("--seed", type=int, default=0)
args = ap.parse_args()
dev = torch.device("cuda", 0)
torch.manual_seed(args.seed)
linear = args.color_space == "linear"

opt = make_options(O=True, bound=1, dt_gamma=0, iters=args.iters0, fused_mlp=True, data_format=args.data_format, color_space=args.color_space,
                   per_view_intrinsics=args.data_format == "dtu", undistort=args.undistort, camera_traj=args.camera_traj, workspace=args.workspace)
model = NeRFNetwork(opt)
if args.data is None:
    Hs, Ws = args.size, args.width or args.size
    f = S.LEGO_FOCAL * Hs / S.LEGO_HW
    cap = Capture.synthetic(S.make_cameras(args.views, seed=0), H=Hs, W=Ws, intrinsics=(f, f, Ws / 2, Hs / 2), linear=linear, device=dev)
elif args.data_format == "dtu":
    cap = Capture.load_dtu(args.data, split="train", downscale=args.downscale, linear=linear, device=dev)
elif args.data_format == "colmap":
    cap = Capture.load_colmap(args.data, split="train", downscale=args.downscale, linear=linear, device=dev, undistort=args.undistort)
    cap.cam_near_far = None
    model.to(dev)
    model.update_aabb(cap.pts_aabb.to(dev))
else:
    cap = Capture.load_nerf(args.data, split="train", downscale=args.downscale, linear=linear, device=dev)

cls = Stage0Engine if Stage0Engine.supported(model, opt, capture=cap) else Stage0Trainer
eng = cls(model, opt, None, dev, seed=args.seed, capture=cap)
eng.mark_untrained()
ckpt0, _ = checkpoint.restore_or_init(eng, args.workspace, args.ckpt)
saved_mesh = checkpoint.stage1_mesh(args.workspace, args.ckpt) if args.source != "field" else None
if ckpt0 is None and saved_mesh is None and args.iters0 <= 0:
    raise SystemExit(f"--iters0 0 needs a stage-0 checkpoint in {os.path.join(args.workspace, 'checkpoints')}")
todo0 = 0 if ckpt0 is not None or saved_mesh is not None else args.iters0
for _ in range(todo0):
    eng.train_step()
torch.cuda.synchronize()
model.eval()
print(f"[stage 0] {f'loaded {ckpt0} (step {eng.global_step}), ' if ckpt0 is not None else ''}{todo0} steps trained ({cls.__name__}) on {len(cap)} views {cap.H} x {cap.W}", flush=True)

path = camera_path.path_for(cap, opt, n_test=args.n_test, seed=args.seed)
if args.source != "field":
    opt.stage, opt.iters = 1, max(args.iters1, 501)
    if saved_mesh is not None:          # the stage-1 file brings its mesh with it
        tr = Stage1Trainer(model, opt, None, saved_mesh[0], saved_mesh[1], dev, capture=cap, v_cumsum=saved_mesh[2], f_cumsum=saved_mesh[3])
    else:
        with eng.averaged_parameters():
            model.export_stage0(os.path.join(args.workspace, "mesh_stage0"), resolution=args.resolution, dataset=cap, clean=True, decimate=True)
        rv, rt = export.read_ply(os.path.join(args.workspace, "mesh_stage0", "mesh_0.ply"))
        if rt.shape[0] == 0:
            raise SystemExit("export_stage0 left no face: stage 0 has not found the object (more --iters0)")
        tr = Stage1Trainer(model, opt, None, torch.from_numpy(rv), torch.from_numpy(rt), dev, capture=cap)
    drv = Stage1Engine(tr) if Stage1Engine.supported(tr) else tr
    ckpt1, mode1 = checkpoint.restore_or_init(drv, args.workspace, args.ckpt) if saved_mesh is not None else (None, None)
    todo1 = 0 if mode1 == "full" else args.iters1
    for _ in range(todo1):
        drv.train_step()
    torch.cuda.synchronize()
    model.eval()
    print(f"[stage 1] {f'loaded {ckpt1} (step {tr.global_step}), ' if mode1 == 'full' else ''}{todo1} steps trained on {model.triangles.shape[0]} faces", flush=True)

torch.cuda.synchronize()
t0 = time.perf_counter()
if args.source == "field":
    with eng.averaged_parameters():
        rgb, depth = camera_path.render_path(metrics.field_renderer(model, path), path, linear=linear)
elif args.source == "mesh":
    rgb, depth = camera_path.render_path(metrics.mesh_renderer(model, path), path, linear=linear)
else:
    out_dir = os.path.join(args.workspace, "mesh_stage1")
    model.export_stage1(out_dir, args.texture, args.texture, atlas="charts")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rgb, depth = camera_path.render_path(metrics.asset_renderer(ExportedAsset.load(out_dir), path, ssaa=int(opt.ssaa)), path, linear=linear)
torch.cuda.synchronize()
t_render = time.perf_counter() - t0
results = os.path.join(args.workspace, "results")
files = camera_path.save_frames(rgb, depth, results, args.name, video=args.video)
t_save = time.perf_counter() - t0 - t_render
print(json.dumps({"source": args.source, "camera_traj": args.camera_traj, "frames": len(path), "H": path.H, "W": path.W, "results": results,
                  "files": len(files), "render_fps": round(len(path) / max(t_render, 1e-9), 2), "save_s": round(t_save, 3)}))
