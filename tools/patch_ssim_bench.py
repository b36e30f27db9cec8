#!/usr/bin/env python3
"""Times of the batched patch SSIM (metrics.ssim_patches) against what the frame entry point can do for the same input --
metrics.ssim called once per patch in a loop --, by device events, in one process.

Per shape (B, P) at C = 3: forward without a gradient request, forward with the derivative maps, and the backward; each as a run of `--reps`
calls after a warm-up, the batched call and the loop alternating inside every one of `--rounds` rounds (median, min - max), with the
algorithmic bytes over the batched median next to it.  Both sides go through autograd, as a step calls them: the time includes the host's
launch path, which a run of calls overlaps where the device is the slower side.

One JSON line at the end."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from nerf2mesh_amd.metrics import ssim, ssim_patches

SHAPES = [(16, 16), (4, 32), (1, 64), (256, 16), (64, 32), (16, 64)]

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--loop_reps", type=int, default=0, help="calls of the per-patch loop per timed run (0: reps, at most 4096 frame calls)")
args = ap.parse_args()
dev = torch.device("cuda", 0)
torch.manual_seed(0)


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternate(batched, loop, reps, loop_reps):
    for _ in range(10):
        batched()
    for _ in range(2):
        loop()
    tb, tl = [], []
    for _ in range(args.rounds):
        tb.append(event_ms(batched, reps))
        tl.append(event_ms(loop, loop_reps))
    stat = lambda t: {"median_ms": round(statistics.median(t), 5), "min_ms": round(min(t), 5), "max_ms": round(max(t), 5)}
    return stat(tb), stat(tl)


result = {"reps": args.reps, "rounds": args.rounds, "shapes": {}}
g = torch.ones((), device=dev)
for B, P in SHAPES:
    x, y = torch.rand(B, P, P, 3, device=dev), torch.rand(B, P, P, 3, device=dev)
    xr = x.clone().requires_grad_()
    xs, ys = list(x.unbind(0)), list(y.unbind(0))
    xrs = [t.clone().requires_grad_() for t in xs]
    loop_reps = args.loop_reps or max(4, min(args.reps, 4096 // B))
    n_img, n_map = B * P * P * 3 * 4, B * (P - 10) * (P - 10) * 3 * 4
    entry = {"loop_reps": loop_reps}
    with torch.no_grad():
        entry["forward"] = alternate(lambda: ssim_patches(x, y), lambda: [ssim(a, b) for a, b in zip(xs, ys)], args.reps, loop_reps)
    entry["forward_with_derivatives"] = alternate(lambda: ssim_patches(xr, y), lambda: [ssim(a, b) for a, b in zip(xrs, ys)], args.reps, loop_reps)
    val = ssim_patches(xr, y)
    vals = [ssim(a, b) for a, b in zip(xrs, ys)]
    entry["backward"] = alternate(lambda: torch.autograd.grad(val, xr, g, retain_graph=True),
                                  lambda: [torch.autograd.grad(v, a, g, retain_graph=True) for v, a in zip(vals, xrs)], args.reps, loop_reps)
    bytes_ = {"forward": 2 * n_img + 4 * B, "forward_with_derivatives": 2 * n_img + 3 * n_map + 4 * B, "backward": 3 * n_img + 3 * n_map}
    for k, (tb, tl) in list(entry.items())[1:]:
        tb["algo_bytes"] = bytes_[k]
        tb["algo_gb_per_s"] = round(bytes_[k] / (tb["median_ms"] * 1e-3) / 1e9, 2)
        entry[k] = {"batched": tb, "loop": tl, "loop_over_batched": round(tl["median_ms"] / tb["median_ms"], 2)}
        print(f"B={B:4d} P={P:3d} {k:26s} batched {tb['median_ms'] * 1e3:8.1f} us (min {tb['min_ms'] * 1e3:.1f}, max {tb['max_ms'] * 1e3:.1f}) "
              f"{tb['algo_gb_per_s']:7.2f} GB/s algorithmic | loop of {B} frame calls {tl['median_ms'] * 1e3:9.1f} us (min {tl['min_ms'] * 1e3:.1f}, "
              f"max {tl['max_ms'] * 1e3:.1f}) | loop / batched {entry[k]['loop_over_batched']:.2f}", flush=True)
    result["shapes"][f"{B}x{P}"] = entry
print(json.dumps(result))
