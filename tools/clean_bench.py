#!/usr/bin/env python3
"""Wall time and effect of the device mesh cleaning (nerf2mesh_amd/mesh_clean.py): clean_mesh with the reference's call (min_f 8,
min_d 5, repair) at v_pct 1 (the default) and 0, on the marching-cubes surfaces of a sphere and of "lego boxes" (tools/mesh_bench.volume)
at 256^3 and 512^3, and on the 256^3 lego boxes with 300 injected floaters.  Per run: faces / vertices in and out, the per-step counts and
round counts, and for v_pct 1 the largest distance of an output vertex to the input surface's vertices, in voxels.  One timed run after
a warm-up.  Writes profiles/clean_bench.json and prints it.

    timeout -k 10 900 python tools/clean_bench.py"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from mesh_bench import timed, volume
from nerf2mesh_amd.marching_cubes import marching_cubes
from nerf2mesh_amd.mesh_clean import clean_mesh


def floaters(v, f, n, seed=0, scale=0.02):
    """n small closed blobs (octahedra, 8 faces) at random places inside the mesh's box."""
    g = torch.Generator().manual_seed(seed)
    lo, hi = v.amin(0).cpu(), v.amax(0).cpu()
    ov = torch.tensor([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=torch.float32) * scale
    of = torch.tensor([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=torch.int32)
    c = lo + torch.rand(n, 3, generator=g) * (hi - lo)
    bv = (ov[None] + c[:, None]).reshape(-1, 3)
    bf = (of[None] + 6 * torch.arange(n, dtype=torch.int32)[:, None, None]).reshape(-1, 3) + v.shape[0]
    return torch.cat([v, bv.cuda()]), torch.cat([f, bf.cuda()])


def max_displacement(v_in, v_out, voxel):
    """How far the merge moves the surface: the largest distance from an input vertex to the nearest output vertex, in voxels (a merged
    vertex is within r of its seed; output vertices are input vertices).  Exact, chunked."""
    best = 0.0
    for chunk in v_in.split(256):
        best = max(best, float(torch.cdist(chunk, v_out).min(1).values.max()))
    return best / voxel


def main():
    runs = []
    cases = []
    for kind in ("sphere", "lego boxes"):
        for R in (256, 512):
            vol, iso = volume(kind, R)
            v, f = marching_cubes(vol, iso, div=R - 1.0, mul=2.0, add=-1.0)
            del vol
            cases.append((kind, R, v, f))
    v, f = next((v, f) for k, R, v, f in cases if k == "lego boxes" and R == 256)
    fv, ff = floaters(v, f, 300)
    cases.append(("lego boxes + 300 floaters", 256, fv, ff))
    for kind, R, v, f in cases:
        for v_pct in (1, 0):
            clean_mesh(v, f, v_pct=v_pct)                   # warm-up
            st = {}
            (cv, cf, _), sec = timed(lambda: clean_mesh(v, f, v_pct=v_pct, stats=st))
            row = {"mesh": kind, "reso": R, "v_pct": v_pct, "faces_in": int(f.shape[0]), "faces_out": int(cf.shape[0]),
                   "vertices_in": int(v.shape[0]), "vertices_out": int(cv.shape[0]), "seconds": round(sec, 4), "stats": st}
            if v_pct == 1 and "floaters" not in kind:
                row["max_displacement_voxels"] = round(max_displacement(v, cv, 2.0 / (R - 1)), 3)
                row["r_voxels"] = round(0.01 * float((v.amax(0) - v.amin(0)).norm()) / (2.0 / (R - 1)), 3)
            runs.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    out = {"device": torch.cuda.get_device_name(0), "clean_mesh": runs}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "clean_bench.json"), "w") as fp:
        json.dump(out, fp, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
