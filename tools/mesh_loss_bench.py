#!/usr/bin/env python3
"""Device time of the normal-consistency / edge-length kernels (nerf2mesh_amd/csrc/meshloss.hip) on a mesh of the stage-1 working size
(synthetic.scene_mesh(300000): ~150 k vertices, ~300 k faces), and the stage-1 executor's step with lambda_normal = 1e-3 against the same
build with 0 (bench.py's stage-1 workload: one 800 x 800 view at ssaa 2 per step).

Kernels: device events around `--reps` back-to-back launches after a warm-up, five repeats, median and spread; the one-off topology build
(trainer.MeshEdgeTerms) as host wall time behind a synchronise.  Step: host clock around `--steps` steps ending in a synchronise, the two
builds alternated (A B B A ...) so that drift hits both.  Writes profiles/mesh_loss_bench.json and prints it.

    timeout -k 10 600 python tools/mesh_loss_bench.py"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from nerf2mesh_amd import _lib as L
from nerf2mesh_amd import synthetic as S
from nerf2mesh_amd.engine_stage1 import Stage1Engine
from nerf2mesh_amd.network import NeRFNetwork
from nerf2mesh_amd.options import make_options
from nerf2mesh_amd.trainer import MeshEdgeTerms, Stage1Trainer


def event_us(fn, reps, repeats=5):
    """Median and (min, max) microseconds per call of `fn`, `reps` calls between two events, `repeats` times, after a warm-up."""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return {"median_us": round(statistics.median(out), 2), "min_us": round(min(out), 2), "max_us": round(max(out), 2)}


def kernels(reps):
    dev = torch.device("cuda")
    v, f = S.scene_mesh(300000)
    v, f = torch.as_tensor(v, dtype=torch.float32, device=dev).contiguous(), torch.as_tensor(f, dtype=torch.int32, device=dev)
    MeshEdgeTerms(f, v.shape[0])                                      # warm-up of the torch ops it is built from
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t = MeshEdgeTerms(f, v.shape[0])
    torch.cuda.synchronize()
    build_ms = (time.perf_counter() - t0) * 1e3
    V, P, E, s = v.shape[0], t.n_pairs, t.n_edges, L.stream()
    x = v + 1e-3 * torch.randn(v.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    partial = torch.empty((P + 255) // 256 + (E + 255) // 256, device=dev)
    d, seed = torch.zeros(V, 3, device=dev), torch.tensor(1024.0, device=dev)
    w_n, w_e = t.weights(1e-3, 1e-3)
    bwd = (L.ptr(x), L.ptr(t.pairs), L.ptr(t.pair_ptr), L.ptr(t.pair_ref), P, L.ptr(t.edges), L.ptr(t.edge_ptr), L.ptr(t.edge_ref), E, V, L.ptr(seed))
    row = {"vertices": V, "faces": int(f.shape[0]), "edges": E, "pairs": P, "topology_build_ms": round(build_ms, 2), "launches_per_timing": reps}
    row["forward, both terms"] = event_us(lambda: L.call("n2m_mesh_losses_forward", L.ptr(x), L.ptr(t.pairs), P, L.ptr(t.edges), E, w_n, w_e,
                                                          L.ptr(partial), s), reps)
    row["forward, normal only"] = event_us(lambda: L.call("n2m_mesh_losses_forward", L.ptr(x), L.ptr(t.pairs), P, L.ptr(t.edges), 0, w_n, 0.0,
                                                           L.ptr(partial), s), reps)
    row["backward_acc, both terms"] = event_us(lambda: L.call("n2m_mesh_losses_backward_acc", *bwd, w_n, w_e, L.ptr(d), s), reps)
    bwd_n = bwd[:8] + (0,) + bwd[9:]
    row["backward_acc, normal only"] = event_us(lambda: L.call("n2m_mesh_losses_backward_acc", *bwd_n, w_n, 0.0, L.ptr(d), s), reps)
    row["backward, both terms"] = event_us(lambda: L.call("n2m_mesh_losses_backward", *bwd, w_n, w_e, L.ptr(d), s), reps)
    return row


def step(steps, warmup, rounds):
    dev = torch.device("cuda")

    def make(lam):
        torch.manual_seed(0)
        opt = make_options(O=True, bound=1, dt_gamma=0, stage=1, fused_mlp=True, lambda_normal=lam)
        v, f = S.scene_mesh(300000)
        tr = Stage1Trainer(NeRFNetwork(opt), opt, S.make_cameras(100, seed=0), v, f, dev)
        tr.preload()
        eng = Stage1Engine(tr)
        for _ in range(warmup):
            eng.train_step()
        torch.cuda.synchronize()
        return eng

    engines = {"lambda_normal 0": make(0.0), "lambda_normal 1e-3": make(1e-3)}
    times = {k: [] for k in engines}
    order = list(engines)
    for r in range(rounds):
        for k in (order if r % 2 == 0 else order[::-1]):
            t0 = time.perf_counter()
            for _ in range(steps):
                engines[k].train_step()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / steps)
    return {"steps_per_timing": steps, "warmup": warmup,
            **{k: {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)} for k, t in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=6)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a CPU run says nothing about these times"
    out = {"device": torch.cuda.get_device_name(0), "kernels": kernels(args.reps), "stage1_engine_step": step(args.steps, args.warmup, args.rounds)}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mesh_loss_bench.json"), "w") as fp:
        json.dump(out, fp, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
