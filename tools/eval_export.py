#!/usr/bin/env python3
"""What the shipped stage-1 asset looks like next to the field it was baked from: trains the synthetic pipeline's model
(tools/pipeline_demo.py's flow, shortened), exports it with the device chart atlas, loads the files back (nerf2mesh_amd.asset) and prints

  * the PSNR of the loaded asset against render_stage1 over held-out views, per texture filter, for the files (after the JPEG) and for
    the un-JPEG'd textures;
  * the same on an untrained field over the marching-cubes sphere (--sphere adds it);
  * the time of ExportedAsset.render and of render_stage1 for one view (device events).

One JSON line at the end."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from nerf2mesh_amd import export, synthetic as S
from nerf2mesh_amd.asset import ExportedAsset, evaluate_export
from nerf2mesh_amd.network import NeRFNetwork
from nerf2mesh_amd.options import make_options

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="bench_runs/eval_export")
ap.add_argument("--iters0", type=int, default=3000)
ap.add_argument("--iters1", type=int, default=300)
ap.add_argument("--resolution", type=int, default=256)
ap.add_argument("--texture", type=int, default=2048)
ap.add_argument("--views", type=int, default=8)
ap.add_argument("--size", type=int, default=800)
ap.add_argument("--sphere", action="store_true")
ap.add_argument("--no-pipeline", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda:0")
torch.manual_seed(0)


def held_out_views(n, size):
    poses = S.make_cameras(n, seed=1)                                 # the training set is seed 0
    focal = S.LEGO_FOCAL * size / S.LEGO_HW
    pix = torch.arange(size * size)
    out = []
    for cam in range(n):
        _, d = S.rays_from_pixels(poses, torch.full_like(pix, cam), pix, size, size, focal)
        out.append((d.to(dev).contiguous(), S.mvp_matrix(poses[cam], size, size, focal).to(dev)))
    return out


def event_ms(fn, warmup=3, reps=20):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def measure(label, model, path, views, size, texture):
    out = model.export_stage1(path, texture, texture, atlas="charts")
    loaded, baked = ExportedAsset.load(path), ExportedAsset.from_export(model, out)
    res = {"faces": int(loaded.triangles.shape[0]), "texture": texture, "views": len(views), "size": size, "ssaa": int(model.opt.ssaa)}
    for name, asset in (("files", loaded), ("no_jpeg", baked)):
        for filt in ("nearest", "linear"):
            ev = evaluate_export(model, asset, views, size, size, filter=filt)
            res[f"psnr_{name}_{filt}"] = round(ev["mean"], 3)
            print(f"[{label}] {name:8s} {filt:8s} PSNR vs render_stage1: mean {ev['mean']:.2f} dB  ("
                  + " ".join(f"{p:.2f}" for p in ev["psnr_vs_stage1"]) + ")", flush=True)
    rays_d, mvp = views[0]
    ssaa = int(model.opt.ssaa)
    with torch.no_grad():
        res["ms_asset_render"] = round(event_ms(lambda: loaded.render(rays_d, mvp, size, size, ssaa=ssaa)), 4)
        res["ms_asset_render_linear"] = round(event_ms(lambda: loaded.render(rays_d, mvp, size, size, ssaa=ssaa, filter="linear")), 4)
        res["ms_render_stage1"] = round(event_ms(lambda: model.render_stage1(None, rays_d, mvp, size, size)), 4)
    print(f"[{label}] one {size}x{size} view (ssaa {ssaa}): ExportedAsset.render {res['ms_asset_render']:.3f} ms (linear "
          f"{res['ms_asset_render_linear']:.3f}), render_stage1 {res['ms_render_stage1']:.3f} ms", flush=True)
    return res


result = {}
views = held_out_views(args.views, args.size)

if args.sphere:
    from nerf2mesh_amd.marching_cubes import marching_cubes
    R = 24
    x = torch.linspace(-1, 1, R, device=dev)
    X, Y, Z = torch.meshgrid(x, x, x, indexing="ij")
    v, t = marching_cubes((0.6 - torch.sqrt(X * X + Y * Y + Z * Z)).contiguous(), 0.0, div=R - 1.0, mul=2.0, add=-1.0)
    opt = make_options(O=True, bound=1, dt_gamma=0, iters=1000, fused_mlp=True)
    opt.stage, opt.ssaa = 1, 1
    sphere = NeRFNetwork(opt).to(dev)
    sphere.init_stage1(v, t)
    result["sphere"] = measure("sphere", sphere, os.path.join(args.out, "sphere"), views, args.size, args.texture)

if not args.no_pipeline:
    from nerf2mesh_amd.engine import Stage0Engine
    from nerf2mesh_amd.trainer import Stage1Trainer
    opt = make_options(O=True, bound=1, dt_gamma=0, iters=args.iters0, fused_mlp=True)
    poses = S.make_cameras(100, seed=0)
    eng = Stage0Engine(NeRFNetwork(opt), opt, poses, dev, seed=0)
    eng.mark_untrained()
    for _ in range(args.iters0):
        eng.train_step()
    model = eng.model
    model.export_stage0(os.path.join(args.out, "mesh_stage0"), resolution=args.resolution)
    rv, rt = export.read_ply(os.path.join(args.out, "mesh_stage0", "mesh_0.ply"))
    opt.stage, opt.iters = 1, max(args.iters1, 501)
    tr = Stage1Trainer(model, opt, poses, torch.from_numpy(rv), torch.from_numpy(rt), dev)
    for _ in range(args.iters1):
        tr.train_step()
    torch.cuda.synchronize()
    print(f"[pipeline] stage 0: {args.iters0} steps, stage 1: {args.iters1} steps on {rt.shape[0]} faces", flush=True)
    model.eval()
    result["pipeline"] = measure("pipeline", model, os.path.join(args.out, "mesh_stage1"), views, args.size, args.texture)

print(json.dumps(result))
