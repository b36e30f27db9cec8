"""The uncontracted stage-1 executor case of tests/test_stage1.py (box-scene mesh of 20000 faces, six cameras, 200 x 200 at ssaa 2, the
schedule past its warm-up) as ONE executor step whose results are recorded: the loss, every colour / specular network parameter, the
vertex offsets and the colour table.

`record()` is executed
  * by tests/golden/make_golden_stage1_executor.py on the commit BEFORE the executor learnt to contract -> tests/golden/stage1_executor_step.npz;
  * by tests/test_stage1_contract_gpu.py on the current code, which must give the same bits with `contract` off.

The colour table (tens of MiB) is recorded as its SHA-256, the number of entries the step moved and every 4099th entry; the step's forward
images and lists (surface points, table coordinates, the shaded RGBA image, the antialiased image) as their SHA-256; everything else in
full.

The vertex offsets are NOT reproducible to the bit between two runs of one build: their gradient is summed with float atomics in the
raster / antialias backward.  The recorder therefore keeps three recordings of them, and the test holds the current code to four times the
largest distance between those three (a few fp32 ulp of the offsets' magnitude)."""
import hashlib

import numpy as np
import torch

H = W = 200
FACES = 20000
TABLE_STRIDE = 4099


def make(dev=None):
    from nerf2mesh_amd import synthetic as S
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    from nerf2mesh_amd.trainer import Stage1Trainer
    dev = dev or torch.device("cuda")
    v, f = S.scene_mesh(FACES)
    torch.manual_seed(0)
    opt = make_options(O=True, bound=1, dt_gamma=0, stage=1, fused_mlp=True)
    tr = Stage1Trainer(NeRFNetwork(opt), opt, S.make_cameras(6, seed=0), v, f, dev, H=H, W=W)
    for _ in range(500):
        tr.scheduler.step()
    return tr


def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8).copy()


def record():
    """One executor step from the seeded state -> {name: numpy array}."""
    from nerf2mesh_amd.engine_stage1 import Stage1Engine
    tr = make()
    m = tr.model
    table0 = m.encoder_color.embeddings.detach().clone()
    eng = Stage1Engine(tr)
    loss = eng.train_step()
    torch.cuda.synchronize()
    out = {"loss": np.float32(float(loss)), "covered": np.int64(m.last_covered),
           "offsets": m.vertices_offsets.detach().cpu().numpy()}
    for i, p in enumerate(list(m.color_net.parameters()) + list(m.specular_net.parameters())):
        out[f"mlp{i}"] = p.detach().cpu().numpy()
    table = m.encoder_color.embeddings.detach()
    t = table.cpu().numpy()
    out["table_sha256"] = _sha(t)
    out["table_moved"] = np.int64(int((table != table0).sum()))
    out["table_sample"] = t.reshape(-1)[::TABLE_STRIDE].copy()
    K = int(m.last_covered)
    for name, x in (("pts", eng.pts[:K]), ("x01", eng.x01[:K]), ("rgba", eng.rgba), ("aa", eng.aa)):
        out[name + "_sha256"] = _sha(x.detach().cpu().numpy())
    return out


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
