#!/usr/bin/env python3
"""Wall time of the device mesh passes (nerf2mesh_amd/mesh_simplify.py): decimation to 3e5 faces of the marching-cubes surfaces of a
sphere and of "lego boxes" (a steep sigmoid of the distance to the synthetic lego stand-in's boxes, synthetic.boxes -- flat faces and sharp
edges, not the density of a trained model) at 256^3 and 512^3, and one refine_and_decimate on a ~300 k-face mesh; under "remesh", the
isotropic re-meshing (nerf2mesh_amd/mesh_remesh.py) of the two 256^3 surfaces at 1.5 x their mean edge length and one
refine_and_decimate(remesh=True) on the same ~300 k-face mesh, with and without the re-projection (project=True); under "query", the
closest-point index (nerf2mesh_amd/mesh_query.py) of the 256^3 sphere: build, 1 M surface-sample queries, and 2^16 queries through the
exhaustive device scan (prune = 0).  Every decimated and re-meshed output reports its sampled one-sided distances to and from its input
(mesh_distance, 1e5 samples a side).  Prints one JSON object.

    timeout -k 10 600 python tools/mesh_bench.py"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from nerf2mesh_amd import synthetic as S
from nerf2mesh_amd.marching_cubes import marching_cubes
from nerf2mesh_amd.mesh_query import MeshIndex, mesh_distance, sample_surface
from nerf2mesh_amd.mesh_remesh import remesh_isotropic
from nerf2mesh_amd.mesh_simplify import decimate


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


def distances(v_out, f_out, v_in, f_in, n=100_000):
    """Sampled one-sided distances between an output mesh and its input: mean and maximum, each way."""
    d = mesh_distance(v_out, f_out, v_in, f_in, n=n, generator=torch.Generator(device="cuda").manual_seed(0))
    return {"out_to_in": {"mean": d["mean_ab"], "max": d["max_ab"]}, "in_to_out": {"mean": d["mean_ba"], "max": d["max_ba"]}, "samples": n}


def query_bench():
    """The 256^3 marching-cubes sphere: index build, 1 M pruned queries, 2^16 queries that visit every leaf; one warm-up call each."""
    vol, iso = volume("sphere", 256)
    v, f = marching_cubes(vol, iso, div=255.0, mul=2.0, add=-1.0)
    del vol
    g = torch.Generator(device="cuda").manual_seed(0)
    pts, _ = sample_surface(v, f, 1_000_000, g)
    MeshIndex(v, f)
    index, t_build = timed(lambda: MeshIndex(v, f))
    index.closest(pts[:4096])
    (d2, _, _), t_pruned = timed(lambda: index.closest(pts))
    few = pts[:1 << 16]
    index.closest(few[:256], prune=False)
    (e2, _, _), t_scan = timed(lambda: index.closest(few, prune=False))
    assert torch.equal(d2[:1 << 16].view(torch.int64), e2.view(torch.int64))
    per_pruned, per_scan = t_pruned / pts.shape[0], t_scan / few.shape[0]
    return {"mesh": "sphere", "reso": 256, "faces": int(f.shape[0]), "build_seconds": round(t_build, 5),
            "pruned": {"queries": int(pts.shape[0]), "seconds": round(t_pruned, 5), "ns_per_query": round(per_pruned * 1e9, 2)},
            "prune0": {"queries": int(few.shape[0]), "seconds": round(t_scan, 5), "ns_per_query": round(per_scan * 1e9, 2)},
            "prune0_over_pruned_per_query": round(per_scan / per_pruned, 1)}


def volume(kind, R):
    g = torch.linspace(-1, 1, R, device="cuda")
    if kind == "sphere":
        x, y, z = torch.meshgrid(g, g, g, indexing="ij")
        return 0.7 - torch.sqrt(x * x + y * y + z * z), 0.0
    # "lego boxes": a steep sigmoid of the signed distance to the nearest box of the synthetic stand-in (not a trained field)
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    d = torch.full_like(x, 1e9)
    for b in S.boxes("cuda")[:, :6]:
        q = torch.stack([(x - (b[0] + b[3]) / 2).abs() - (b[3] - b[0]) / 2, (y - (b[1] + b[4]) / 2).abs() - (b[4] - b[1]) / 2,
                         (z - (b[2] + b[5]) / 2).abs() - (b[5] - b[2]) / 2])
        d = torch.minimum(d, q.clamp(min=0).norm(dim=0) + q.max(0).values.clamp(max=0))
        del q
    return 50.0 * torch.sigmoid(-d * R), 10.0


def main():
    res = {"decimate": []}
    target = 300_000
    for kind in ("sphere", "lego boxes"):
        for R in (256, 512):
            vol, iso = volume(kind, R)
            v, f = marching_cubes(vol, iso, div=R - 1.0, mul=2.0, add=-1.0)
            del vol
            decimate(v, f, target)                          # warm-up (kernels loaded, allocator primed)
            stats = {}
            (dv, df, _), sec = timed(lambda: decimate(v, f, target, stats=stats))
            res["decimate"].append({"mesh": kind, "reso": R, "faces_in": int(f.shape[0]), "faces_out": int(df.shape[0]), "seconds": round(sec, 4),
                                    "rounds": stats["rounds"], "faces_per_round": stats["faces"], "distance": distances(dv, df, v, f)})
            print(json.dumps(res["decimate"][-1]), file=sys.stderr, flush=True)
    # one refine_and_decimate on a ~300 k-face mesh with a random error field
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    torch.manual_seed(0)
    v, f = S.scene_mesh(300_000)
    model = NeRFNetwork(make_options(O=True, bound=1, dt_gamma=0, stage=1)).cuda()
    model.init_stage1(v, f)
    g = torch.Generator(device="cuda").manual_seed(0)
    model.triangles_errors.copy_(torch.rand(f.shape[0], device="cuda", generator=g))
    model.triangles_errors_cnt.fill_(1)
    out, sec = timed(lambda: model.refine_and_decimate())
    res["refine_and_decimate"] = {"faces_in": out["before"]["faces"], "faces_out": out["after"]["faces"], "seconds": round(sec, 4),
                                  "decimate_class": out["decimate"], "refine_class": out["refine"]}
    # isotropic re-meshing: the 256^3 surfaces at 1.5 x their mean edge length, 3 iterations, one warm-up call, then one timed call
    res["remesh"] = {"meshes": []}
    for kind in ("sphere", "lego boxes"):
        vol, iso = volume(kind, 256)
        v, f = marching_cubes(vol, iso, div=255.0, mul=2.0, add=-1.0)
        del vol
        e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).long()
        target_len = 1.5 * float((v[e[:, 0]] - v[e[:, 1]]).norm(dim=1).mean())      # every edge twice on a closed surface: the same mean
        remesh_isotropic(v, f, target_len)
        stats = {}
        (rv, rf, _), sec = timed(lambda: remesh_isotropic(v, f, target_len, stats=stats))
        res["remesh"]["meshes"].append({"mesh": kind, "reso": 256, "target_len": round(target_len, 6), "faces_in": int(f.shape[0]),
                                        "faces_out": int(rf.shape[0]), "seconds": round(sec, 4),
                                        "rounds": [{k: it[k] for k in ("split_rounds", "collapse_rounds", "flip_rounds", "relax_reverts", "faces")}
                                                   for it in stats["iterations"]], "distance": distances(rv, rf, v, f)})
        print(json.dumps(res["remesh"]["meshes"][-1]), file=sys.stderr, flush=True)
        remesh_isotropic(v, f, target_len, project=True)
        stats = {}
        (rv, rf, _), sec = timed(lambda: remesh_isotropic(v, f, target_len, stats=stats, project=True))
        res["remesh"]["meshes"].append({"mesh": kind, "reso": 256, "project": True, "target_len": round(target_len, 6), "faces_in": int(f.shape[0]),
                                        "faces_out": int(rf.shape[0]), "seconds": round(sec, 4),
                                        "rounds": [{k: it[k] for k in ("split_rounds", "collapse_rounds", "flip_rounds", "relax_reverts", "faces",
                                                                       "projected")} for it in stats["iterations"]],
                                        "distance": distances(rv, rf, v, f)})
        print(json.dumps(res["remesh"]["meshes"][-1]), file=sys.stderr, flush=True)
    torch.manual_seed(0)
    v, f = S.scene_mesh(300_000)
    model = NeRFNetwork(make_options(O=True, bound=1, dt_gamma=0, stage=1)).cuda()
    model.init_stage1(v, f)
    g = torch.Generator(device="cuda").manual_seed(0)
    model.triangles_errors.copy_(torch.rand(f.shape[0], device="cuda", generator=g))
    model.triangles_errors_cnt.fill_(1)
    out, sec = timed(lambda: model.refine_and_decimate(remesh=True))
    res["remesh"]["refine_and_decimate"] = {"faces_in": out["before"]["faces"], "faces_out": out["after"]["faces"], "seconds": round(sec, 4),
                                            "decimate_class": out["decimate"], "refine_class": out["refine"], "remesh": out["remesh"]}
    res["query"] = query_bench()
    print(json.dumps(res["query"]), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
