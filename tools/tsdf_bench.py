#!/usr/bin/env python3
"""Time of n2m_tsdf_integrate (TSDFVolume.integrate) against streaming: on an R^3 volume (default 256) with synthetic
S x S depth maps (default 800) of a sphere -- a ring of cameras at radius 3, +inf where a ray misses --

    one call with n = 1, 8 and 32 views;  32 calls with n = 1 (what a view-at-a-time kernel would pay in volume traffic);
    a plain device copy that moves the same 2 * 8 * R^3 bytes one call reads and writes (tsdf + weight, once each way).

Device events around `--reps` back-to-back repetitions after `--warmup` unmeasured ones; prints a table and one JSON line.  Not read by
bench.py."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from nerf2mesh_amd.tsdf import TSDFVolume, camera_rows

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--resolution", type=int, default=256)
ap.add_argument("--size", type=int, default=800, help="side of the depth maps")
ap.add_argument("--views", type=int, default=32)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("tsdf_bench: no GPU (the fusion runs on the device; there is no host path to time)")
dev = torch.device("cuda", 0)
R, S, V = args.resolution, args.size, args.views


def ring_pose(k):
    a = 2 * math.pi * k / V
    c = torch.tensor([3 * math.cos(a) * 0.9, 3 * math.sin(a) * 0.9, 3 * math.sqrt(1 - 0.81)], dtype=torch.float64)
    z = c / c.norm()
    x = torch.linalg.cross(torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64), z)
    x = x / x.norm()
    P = torch.eye(4, dtype=torch.float64)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = x, torch.linalg.cross(z, x), z, c
    return P


focal = 1.1 * S
poses = torch.stack([ring_pose(k) for k in range(V)]).float().to(dev)
cams = camera_rows(poses, (focal, focal, S / 2, S / 2))
jj, ii = torch.meshgrid(torch.arange(S, device=dev, dtype=torch.float32), torch.arange(S, device=dev, dtype=torch.float32), indexing="ij")
cam_dirs = torch.stack([(ii + 0.5 - S / 2) / focal, -(jj + 0.5 - S / 2) / focal, -torch.ones_like(ii)], -1)
depth = torch.empty(V, S, S, dtype=torch.float32, device=dev)
for v in range(V):                                     # the radius-0.6 sphere, closed form; |z| = 1, so t is the depth along the axis
    d = cam_dirs @ poses[v, :3, :3].T
    o = poses[v, :3, 3]
    a, b, c = (d * d).sum(-1), 2 * (d @ o), o @ o - 0.36
    disc = b * b - 4 * a * c
    depth[v] = torch.where(disc >= 0, (-b - disc.clamp(min=0).sqrt()) / (2 * a), torch.full_like(a, float("inf")))

vol = TSDFVolume(R, device=dev)
src = torch.empty(2 * R ** 3, dtype=torch.float32, device=dev)          # 8 R^3 bytes: copying them reads and writes 2 * 8 R^3 bytes
dst = torch.empty_like(src)


def timed(fn):
    for _ in range(args.warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.reps


def per_view():
    for v in range(V):
        vol.integrate(cams[v:v + 1], depth[v:v + 1])


res = {"resolution": R, "size": S, "reps": args.reps, "volume_bytes_per_call": 16 * R ** 3}
res["copy_ms"] = timed(lambda: dst.copy_(src))
for n in sorted({1, min(8, V), V}):
    res[f"integrate_n{n}_ms"] = timed(lambda n=n: vol.integrate(cams[:n], depth[:n]))
res[f"integrate_{V}x_n1_ms"] = timed(per_view)
observed = float((vol.weight > 0).float().mean())
res["observed_share"] = round(observed, 4)
gbs = lambda ms: 16 * R ** 3 / ms / 1e6
print(f"volume {R}^3 ({16 * R ** 3 / 1e6:.1f} MB read + written per call), {V} depth maps of {S} x {S}; {observed:.3f} of the lattice observed")
print(f"  device copy of the same bytes      {res['copy_ms']:9.4f} ms   {gbs(res['copy_ms']):8.1f} GB/s")
for n in sorted({1, min(8, V), V}):
    ms = res[f"integrate_n{n}_ms"]
    print(f"  one call, n = {n:<3d}                  {ms:9.4f} ms   {ms / n:9.4f} ms / view   volume traffic {gbs(ms):8.1f} GB/s")
ms = res[f"integrate_{V}x_n1_ms"]
print(f"  {V} calls, n = 1                    {ms:9.4f} ms   {ms / V:9.4f} ms / view   ({ms / res[f'integrate_n{V}_ms']:.2f} x the one call)")
print(json.dumps({k: (round(x, 5) if isinstance(x, float) else x) for k, x in res.items()}))
