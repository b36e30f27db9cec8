"""Both stage-0 drivers with opt.enable_dense_depth on a COLMAP capture: 9 views of the box scene at 24 x 20 px (7 of them train) with the
scene's lattice points as the reconstruction's sparse points, and per-view depth maps computed from the scene's boxes (ray-box depth
along the camera axis) written beside them.  lambda_depth = 10: with the reference's 0.1 and its 1000-step ramp the term would be too
small to be seen in 30 steps."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dense_depth_case as DC   # noqa: E402

pytestmark = pytest.mark.gpu

STEPS = 30
H, W = 20, 24


@pytest.fixture(scope="module")
def recon(tmp_path_factory):
    from nerf2mesh_amd import synthetic
    from nerf2mesh_amd.capture import Capture
    tiny = Capture.load_colmap(DC.TINY, split="trainval", scale=1.0)
    fx, fy, cx, cy = tiny.intrinsics
    intr = (2 * fx, 2 * fy, 2 * cx, 2 * cy)
    big = Capture.synthetic(tiny.poses, H=H, W=W, intrinsics=intr, alpha=True)
    root = str(tmp_path_factory.mktemp("colmap24dd"))
    big.save_colmap(root, synthetic.scene_points().numpy(), depths=DC.box_depth_maps(tiny.poses, H, W, intr))
    return root


def _load(recon, dense=True, **kw):
    from nerf2mesh_amd.capture import Capture
    return Capture.load_colmap(recon, split="train", scale=1.0, device="cuda", dense_depth=dense, **kw)


def _run(cls, cap, steps=STEPS, **over):
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    torch.manual_seed(0)
    over.setdefault("lambda_depth", 10.0)
    opt = make_options(O=True, bound=1, dt_gamma=0, iters=30000, fused_mlp=True, diffuse_step=12, enable_cam_near_far=True, **over)
    opt.num_rays, opt.num_points = 1024, 1 << 14
    model = NeRFNetwork(opt).to("cuda")
    model.update_aabb(cap.pts_aabb.cuda())
    tr = cls(model, opt, None, torch.device("cuda", 0), seed=0, capture=cap)
    tr.mark_untrained()
    losses, rays = [], []
    for _ in range(steps):
        losses.append(float(tr.train_step().detach()))
        rays.append(int(tr.num_rays))
    torch.cuda.synchronize()
    return tr, losses, rays


def _drivers():
    from nerf2mesh_amd.engine import Stage0Engine
    from nerf2mesh_amd.trainer import Stage0Trainer
    return Stage0Engine, Stage0Trainer


def _same_parameters(a, b):
    for (n, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(p, q), n


@pytest.fixture(scope="module")
def runs(recon):
    """The engine runs several tests look at, made once: option on, option off (same capture), option on with lambda_depth = 0."""
    Engine, _ = _drivers()
    cap = _load(recon)
    sb = cap.dense_depth_scale_bias
    print("fitted (scale, bias) per training view:", np.round(sb, 4).tolist())
    assert cap.dense_depth.shape == (7, H * W) and cap.dense_depth.is_cuda and (sb[:, 0] > 0).all()
    return {"cap": cap, "on": _run(Engine, cap, enable_dense_depth=True), "off": _run(Engine, cap),
            "zero": _run(Engine, cap, enable_dense_depth=True, lambda_depth=0.0)}


def test_engine_against_trainer_on_every_step(runs):
    Engine, Trainer = _drivers()
    b, lb, rb = runs["on"]
    assert Engine.supported(b.model, b.opt) and b.dense_depth is not None and b.depth_schedule is None
    a, la, ra = _run(Trainer, runs["cap"], enable_dense_depth=True)
    print("engine :", [f"{x:.5f}" for x in lb])
    print("trainer:", [f"{x:.5f}" for x in la])
    # every one of the 30 batches had the same rays and samples in both drivers (num_rays itself is not compared: it belongs to the batch
    # each driver has prepared last, and the executor prepares further ahead)
    assert a.samples_seen == b.samples_seen and a.rays_seen == b.rays_seen
    np.testing.assert_allclose(la, lb, rtol=2e-4, atol=1e-7)             # tests/test_colmap_engine_gpu.py's bound for the same head
    # N stays num_rays and these steps steer it: the ray count moved as in the run without the option, whose batches have the same rays
    assert len(set(rb)) > 1 and rb[0] == runs["off"][2][0]


def test_two_engine_runs_are_bit_identical(runs):
    Engine, _ = _drivers()
    a, la, ra = runs["on"]
    b, lb, rb = _run(Engine, runs["cap"], enable_dense_depth=True)
    assert la == lb and ra == rb and a.samples_seen == b.samples_seen
    _same_parameters(a, b)


def test_the_term_is_present_from_step_two_on(runs):
    """lambda_depth * min(1, step / 1000) is positive from step 1 on; the first loss already carries the term, and from step 2 on the
    parameters have moved under it too."""
    on, off = runs["on"][1], runs["off"][1]
    print("on :", [f"{x:.5f}" for x in on[:6]], "\noff:", [f"{x:.5f}" for x in off[:6]])
    assert all(x != y for x, y in zip(on[1:], off[1:]))
    assert all(np.isfinite(on))


def test_lambda_zero_equals_the_option_off_bit_for_bit(runs):
    """The head's documented + 0: with lambda_depth = 0 the depth head reproduces the entropy head's bits."""
    z, lz, rz = runs["zero"]
    o, lo, ro = runs["off"]
    assert z.dense_depth is not None and o.dense_depth is None
    assert lz == lo and rz == ro and z.samples_seen == o.samples_seen
    _same_parameters(z, o)


def test_a_bank_that_is_not_asked_for_changes_nothing(recon, runs):
    Engine, _ = _drivers()
    bare = _load(recon, dense=False)
    assert bare.dense_depth is None and torch.equal(bare.bank, runs["cap"].bank)
    b, lb, rb = _run(Engine, bare)
    o, lo, ro = runs["off"]
    assert lb == lo and rb == ro
    _same_parameters(b, o)


def test_value_errors_and_sdf(recon, runs):
    from nerf2mesh_amd import synthetic
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    dev = torch.device("cuda", 0)
    for cls in _drivers():
        mk = lambda **kw: make_options(O=True, bound=1, dt_gamma=0, fused_mlp=True, enable_dense_depth=True, **kw)
        with pytest.raises(ValueError, match="needs a capture"):
            cls(NeRFNetwork(mk()), mk(), synthetic.make_cameras(4), dev, seed=0)
        with pytest.raises(ValueError, match="no dense-depth bank"):
            cls(NeRFNetwork(mk()), mk(), None, dev, seed=0, capture=_load(recon, dense=False))
        with pytest.raises(ValueError, match="exclude each other"):
            cls(NeRFNetwork(mk()), mk(enable_sparse_depth=True), None, dev, seed=0, capture=_load(recon, sparse_depth=True))
    Engine, _ = _drivers()
    for depth, want in ((False, True), (True, False)):                   # SDF with depth goes to the trainer
        opt = make_options(O=True, bound=1, dt_gamma=0, fused_mlp=True, sdf=True, enable_dense_depth=depth)
        assert Engine.supported(NeRFNetwork(opt), opt) == want
