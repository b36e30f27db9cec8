#!/usr/bin/env python3
"""Wall time of the device UV atlas (nerf2mesh_amd/uv_atlas.py) on the cleaned 300 000-face synthetic.scene_mesh at 2048^2 and 4096^2:
one warm-up, then REPEATS timed calls (median, min, max of the wall time between device synchronisations), then one call with per-phase
timings (labels + relaxation, components per round, every pack trial, every eviction round; each phase is bracketed by a
synchronisation, so their sum exceeds the untimed wall).  Writes profiles/uv_atlas_bench.json and prints it.

    timeout -k 10 600 python tools/uv_atlas_bench.py"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from nerf2mesh_amd import synthetic as S
from nerf2mesh_amd.mesh_clean import clean_mesh
from nerf2mesh_amd.uv_atlas import uv_atlas

REPEATS = 7


def main():
    v, f = S.scene_mesh(300000, device="cuda")
    v, f, _ = clean_mesh(v, f, v_pct=0)
    runs = []
    for res in (2048, 4096):
        uv_atlas(v, f, res, res)                              # warm-up
        wall = []
        for _ in range(REPEATS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            uv_atlas(v, f, res, res)
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
        st = {"timings": True}
        uv_atlas(v, f, res, res, stats=st)
        row = {"faces": int(f.shape[0]), "vertices": int(v.shape[0]), "height": res, "width": res, "repeats": REPEATS,
               "wall_median_s": round(statistics.median(wall), 5), "wall_min_s": round(min(wall), 5), "wall_max_s": round(max(wall), 5),
               "phases_s": {k: ([round(x, 5) for x in t] if isinstance(t, list) else round(t, 5)) for k, t in st["timings"].items()},
               "stats": {k: st[k] for k in ("charts", "uv_vertices", "relax_changed", "evict_rounds", "evicted_faces", "pack_trials", "scale",
                                            "utilisation", "density_min", "density_max")}}
        row["stats"]["density_over_scale2"] = [st["density_min"] / st["scale"] ** 2, st["density_max"] / st["scale"] ** 2]
        runs.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    out = {"device": torch.cuda.get_device_name(0), "uv_atlas": runs}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "uv_atlas_bench.json"), "w") as fp:
        json.dump(out, fp, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
