#!/usr/bin/env python3
"""Timings of pose refinement on one device: n2m_pose_ray_grad + n2m_pose_view_grad on one 2^18-sample batch (4096 rays of 64
samples, 100 views) against the torch statement (pose_refine.pose_grad_torch, what attach_torch's backward runs) on the same tensors --
device events around each call, 20 warm-up calls, median / min / p90 of 200 (50 for torch) -- and the whole Stage0Trainer step with
optimize_poses on and off, both unfused and unpipelined (lego recipe on a 20-view capture, 60 warm-up steps, 100 timed, arms in turn twice).
Prints JSON lines.

    timeout -k 10 400 python tools/pose_bench.py"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from nerf2mesh_amd import _lib as L, synthetic
from nerf2mesh_amd.capture import Capture
from nerf2mesh_amd.network import NeRFNetwork
from nerf2mesh_amd.options import make_options
from nerf2mesh_amd.pose_refine import pose_grad_torch
from nerf2mesh_amd.trainer import Stage0Trainer

dev = torch.device("cuda", 0)
g = torch.Generator(device="cuda").manual_seed(0)
M, N, V = 1 << 18, 4096, 100
gx, gd = torch.randn(M, 3, device=dev, generator=g), torch.randn(M, 3, device=dev, generator=g)
ts = torch.rand(M, 2, device=dev, generator=g) + 0.5
cnt = torch.full((N,), M // N, dtype=torch.int32, device=dev)
rays = torch.stack([(torch.cumsum(cnt, 0) - cnt).int(), cnt], 1).contiguous()
rays_d = torch.randn(N, 3, device=dev, generator=g)
view = torch.randint(0, V, (N,), device=dev, generator=g).int()
delta = torch.randn(V, 6, device=dev, generator=g) * 0.01
ray6, out = torch.empty(N, 6, device=dev), torch.empty(V, 6, device=dev)

def pair():
    L.call("n2m_pose_ray_grad", L.ptr(gx), L.ptr(gd), None, L.ptr(ts), L.ptr(rays), L.ptr(rays_d), M, N, L.ptr(ray6), L.stream())
    L.call("n2m_pose_view_grad", L.ptr(ray6), L.ptr(view), L.ptr(delta), N, V, L.ptr(out), L.stream())

def events(fn, warm=20, reps=200):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    return {"median_us": times[len(times) // 2], "min_us": times[0], "p90_us": times[int(len(times) * 0.9)]}

res = {"kernels": events(pair), "torch": events(lambda: pose_grad_torch(gx, gd, ts, rays, rays_d, view, delta), warm=5, reps=50)}
ref = pose_grad_torch(gx, gd, ts, rays, rays_d, view, delta)
pair()
torch.cuda.synchronize()
res["kernels_vs_torch_max_abs"], res["grad_max_abs"] = float((out - ref).abs().max()), float(ref.abs().max())
print(json.dumps(res), flush=True)

cap = Capture.synthetic(synthetic.make_cameras(20, seed=0), device="cuda")
for on in (False, True, False, True):
    torch.manual_seed(0)
    opt = make_options(O=True, bound=1, dt_gamma=0, iters=30000, fused_mlp=False, optimize_poses=on)
    tr = Stage0Trainer(NeRFNetwork(opt), opt, None, dev, seed=0, capture=cap)
    tr.pipeline = False
    tr.mark_untrained()
    for _ in range(60):
        tr.train_step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(100):
        tr.train_step()
    torch.cuda.synchronize()
    print(json.dumps({"optimize_poses": on, "ms_per_step": (time.perf_counter() - t0) * 10, "samples": tr.last_num_points, "rays": tr.num_rays}), flush=True)
    del tr
