#!/usr/bin/env python3
"""Time of the lens undistortion of a whole image bank (n2m_capture_undistort) next to a plain copy of the same bytes
(n2m_stream_copy) in the same process, by device events: the colour pass for the polynomial and the fisheye family, broadcast rows and a
row per view, and the depth pass.  Every variant is timed as a run of `--reps` calls after a warm-up, repeated `--rounds` times, the
variants alternating inside a round.  One JSON line at the end."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from nerf2mesh_amd import _lib as L
from nerf2mesh_amd import capture as C

ap = argparse.ArgumentParser()
ap.add_argument("--views", type=int, default=64)
ap.add_argument("--size", type=int, default=800)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda", 0)
V, H, W = args.views, args.size, args.size
intr = (1.2 * W, 1.2 * W, W / 2, H / 2)
bank = torch.randint(-2 ** 31, 2 ** 31 - 1, (V, H * W), dtype=torch.int32, device=dev)
planes = torch.rand(V, H * W, device=dev)
out_i, out_f = torch.empty_like(bank), torch.empty_like(planes)
nbytes = bank.numel() * 4


def case(model, coeff, depth, table):
    _, family, row = C.lens_row(model, (intr if model.startswith("OPENCV") else (intr[0], intr[2], intr[3])) + tuple(coeff))
    s = C.undistort_zoom(H, W, intr, family, row)
    rows = [intr, (s * intr[0], s * intr[1], intr[2], intr[3]), row]
    if table:
        rows = [np.tile(r, (V, 1)) for r in rows]
    fn, src, dst = (C.undistort_depth, planes, out_f) if depth else (C.undistort_bank, bank, out_i)
    return lambda: fn(src, H, W, *rows, family, out=dst)


wg = 256 * 8
variants = {"stream_copy": lambda: L.call("n2m_stream_copy", bank.data_ptr(), out_i.data_ptr(), nbytes, wg, L.stream()),
            "brown_broadcast": case("SIMPLE_RADIAL", (0.1,), False, False),
            "brown_table": case("OPENCV", (0.1, -0.02, 0.003, -0.002), False, True),
            "fisheye_broadcast": case("OPENCV_FISHEYE", (0.05, 0.01, 0.0, 0.0), False, False),
            "depth_broadcast": case("SIMPLE_RADIAL", (0.1,), True, False)}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(args.reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / args.reps


for fn in variants.values():
    for _ in range(3):
        fn()
times = {k: [] for k in variants}
for _ in range(args.rounds):
    for k, fn in variants.items():
        times[k].append(event_ms(fn))
result = {"views": V, "size": args.size, "bank_bytes": nbytes, "reps": args.reps, "rounds": args.rounds}
for k, t in times.items():
    med = statistics.median(t)
    result[k] = {"median_ms": round(med, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4), "read_plus_write_gb_per_s": round(2 * nbytes / (med * 1e-3) / 1e9, 1)}
    print(f"{k:18s} {med:8.4f} ms (min {min(t):.4f}, max {max(t):.4f})  {result[k]['read_plus_write_gb_per_s']:8.1f} GB/s (bank read once + written once)", flush=True)
print(json.dumps(result))
