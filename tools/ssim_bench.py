#!/usr/bin/env python3
"""Times of the SSIM kernels and of the stage-1 step with and without the SSIM term, by device events.

  * one frame (default 800 x 800 x 3): metrics.ssim forward without a gradient request (n2m_ssim_forward + the partials' reduction), forward with
    the three derivative maps, and the backward (n2m_ssim_backward) -- each timed as a run of `--reps` calls after a warm-up, repeated
    `--rounds` times (the spread is printed), with the algorithmic bytes over the median time next to it;
  * one stage-1 step on the box-scene mesh at the frame's size: the fused head (the default), the torch-graph head with lambda_ssim = 0 and the
    torch-graph head with lambda_ssim = 0.2 -- the three alternate inside every round.

One JSON line at the end."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from nerf2mesh_amd import synthetic as S
from nerf2mesh_amd.metrics import ssim
from nerf2mesh_amd.network import NeRFNetwork
from nerf2mesh_amd.options import make_options
from nerf2mesh_amd.trainer import Stage1Trainer

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=800)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--faces", type=int, default=100000)
args = ap.parse_args()
dev = torch.device("cuda", 0)
torch.manual_seed(0)
H = W = args.size


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def rounds(fn, reps):
    for _ in range(10):
        fn()
    t = [event_ms(fn, reps) for _ in range(args.rounds)]
    return {"median_ms": round(statistics.median(t), 5), "min_ms": round(min(t), 5), "max_ms": round(max(t), 5)}


x, y = torch.rand(H, W, 3, device=dev), torch.rand(H, W, 3, device=dev)
xr = x.clone().requires_grad_()
n_img, n_map = H * W * 3 * 4, (H - 10) * (W - 10) * 3 * 4
result = {"size": args.size, "reps": args.reps, "rounds": args.rounds}
with torch.no_grad():
    result["forward"] = rounds(lambda: ssim(x, y), args.reps)                                    # reads x, y
result["forward"]["algo_bytes"] = 2 * n_img
result["forward_with_derivatives"] = rounds(lambda: ssim(xr, y), args.reps)                      # + writes the three maps
result["forward_with_derivatives"]["algo_bytes"] = 2 * n_img + 3 * n_map
val = ssim(xr, y)
g = torch.ones((), device=dev)
# (both entries through autograd, as the step calls them: the time includes the host's launch path, which the run of `reps` calls overlaps)
result["backward"] = rounds(lambda: torch.autograd.grad(val, xr, g, retain_graph=True), args.reps)      # reads x, y, three maps; writes grad
result["backward"]["algo_bytes"] = 3 * n_img + 3 * n_map
for k in ("forward", "forward_with_derivatives", "backward"):
    r = result[k]
    r["algo_gb_per_s"] = round(r["algo_bytes"] / (r["median_ms"] * 1e-3) / 1e9, 1)
    print(f"{k:26s} {r['median_ms'] * 1e3:8.1f} us (min {r['min_ms'] * 1e3:.1f}, max {r['max_ms'] * 1e3:.1f})  {r['algo_gb_per_s']:7.1f} GB/s algorithmic", flush=True)


def trainer(lam, graph):
    torch.manual_seed(0)
    opt = make_options(O=True, bound=1, dt_gamma=0, stage=1, fused_mlp=True, lambda_ssim=lam)
    v, f = S.scene_mesh(args.faces)
    tr = Stage1Trainer(NeRFNetwork(opt), opt, S.make_cameras(8, seed=0), v, f, dev, H=H, W=W)
    if graph:
        tr.fused_head = False
    for _ in range(500):
        tr.scheduler.step()
    tr.preload()
    return tr


trs = {"fused_head": trainer(0, False), "graph_head": trainer(0, True), "graph_head_ssim_0.2": trainer(0.2, True)}
for tr in trs.values():
    for _ in range(16):
        tr.train_step()
times = {k: [] for k in trs}
for _ in range(args.rounds):
    for k, tr in trs.items():
        times[k].append(event_ms(tr.train_step, args.steps))
result["stage1_step"] = {"faces": args.faces, "steps": args.steps, "ssaa": 2}
for k, t in times.items():
    result["stage1_step"][k] = {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}
    print(f"stage-1 step, {k:20s} {statistics.median(t):8.3f} ms (min {min(t):.3f}, max {max(t):.3f})", flush=True)
print(json.dumps(result))
