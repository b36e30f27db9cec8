#!/usr/bin/env python3
"""Multi-rank stage-1 refinement (launch with torch.distributed.run; N2M_DIST_BACKEND=gloo lets the ranks share one GPU): a few steps
accumulate per-face errors on every rank's own views, Stage1Trainer.refine_mesh() sums them, rank 0 refines and decimates the mesh on the
device, every rank takes the new mesh over; the meshes must be bit-identical on all ranks and training goes on in lock-step with a new
Stage1Engine.  Prints 'DIST_CHECK_REFINE OK ...' on rank 0."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.distributed as dist
from nerf2mesh_amd import synthetic
from nerf2mesh_amd.engine_stage1 import Stage1Engine
from nerf2mesh_amd.network import NeRFNetwork
from nerf2mesh_amd.options import make_options
from nerf2mesh_amd.parallel import init_from_env
from nerf2mesh_amd.trainer import Stage1Trainer

rank, world, local = init_from_env()
device = torch.device("cuda", local % torch.cuda.device_count())
torch.cuda.set_device(device)
torch.manual_seed(0)
opt = make_options(O=True, bound=1, dt_gamma=0, stage=1, fused_mlp=True)
v, f = synthetic.scene_mesh(20000)
tr = Stage1Trainer(NeRFNetwork(opt), opt, synthetic.make_cameras(8, seed=0), v, f, device, H=200, W=200, rank=rank, world_size=world)
eng = Stage1Engine(tr)
losses = [float(eng.train_step()) for _ in range(8)]
stats = tr.refine_mesh(src=0)


def same_everywhere(t):
    got = [torch.zeros_like(t) for _ in range(world)]
    dist.all_gather(got, t)
    return all(torch.equal(g, got[0]) for g in got)


m = tr.model
n = torch.tensor([m.vertices.shape[0], m.triangles.shape[0]], device=device)
ok = same_everywhere(n) and same_everywhere(m.vertices.contiguous()) and same_everywhere(m.triangles.contiguous())
ok = ok and int(n[1]) != f.shape[0] and float(m.vertices_offsets.detach().abs().sum()) == 0 and float(m.triangles_errors_cnt.sum()) == 0
eng = Stage1Engine(tr)
more = [float(eng.train_step()) for _ in range(4)]
flat = torch.cat([p.detach().float().reshape(-1) for p in m.parameters()])
ok = ok and all(l == l for l in losses + more) and bool(torch.isfinite(flat).all()) and same_everywhere(flat.double().sum().reshape(1))
dist.barrier()
if rank == 0:
    print(f"DIST_CHECK_REFINE {'OK' if ok else 'FAILED'} world={world} backend={dist.get_backend()} faces {f.shape[0]} -> {int(n[1])} {stats}")
dist.destroy_process_group()
sys.exit(0 if ok else 1)
