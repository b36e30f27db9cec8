"""Per-image appearance codes (--ind_dim), host side: which configurations the drivers accept, the parameter names and shapes (the
reference's: `individual_codes [ind_num, D]`, `color_net.net.0.weight [64, 35 + D]`), and the view ids of the CPU batch path.

The view ids are checked against a bank in which view v is the constant colour v: the decoded `rgba` of a ray then says which view the
batch read its pixel from, whatever expression picked it."""
import os

import numpy as np
import pytest
import torch

from nerf2mesh_amd.capture import Capture, batch_views

TINY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colmap_tiny")
V, H, W = 11, 6, 8


def constant_colour_capture(device="cpu", alpha=True, views=V):
    """View v of the bank is the colour (v, v, v) everywhere, alpha 255: round(rgba * 255) is the view a ray read."""
    from nerf2mesh_amd import synthetic
    img = torch.arange(views, dtype=torch.uint8).view(views, 1, 1, 1).expand(views, H, W, 4 if alpha else 3).clone()
    if alpha:
        img[..., 3] = 255
    return Capture.from_arrays(synthetic.make_cameras(views, seed=0), img, (9.0, 9.0, W / 2, H / 2), device=device)


def _options(**over):
    from nerf2mesh_amd.options import make_options
    kw = dict(O=True, bound=1, dt_gamma=0, fused_mlp=True)
    kw.update(over)
    return make_options(**kw)


def _model(opt):
    from nerf2mesh_amd.network import NeRFNetwork
    torch.manual_seed(0)
    return NeRFNetwork(opt)


@pytest.mark.parametrize("ind_dim", [0, 8])
@pytest.mark.parametrize("with_capture", [False, True])
@pytest.mark.parametrize("sdf", [False, True])
@pytest.mark.parametrize("world_size", [1, 2])
def test_executor_accepts_codes_on_a_capture_in_density_mode_on_one_rank(ind_dim, with_capture, sdf, world_size):
    from nerf2mesh_amd.engine import Stage0Engine
    opt = _options(ind_dim=ind_dim, ind_num=16, sdf=sdf)
    model = _model(opt)
    cap = constant_colour_capture() if with_capture else None
    want = ind_dim == 0 or (with_capture and not sdf and world_size == 1)
    assert Stage0Engine.supported(model, opt, capture=cap, world_size=world_size) == want
    if ind_dim == 0:       # the two new arguments do not change what was accepted before
        assert Stage0Engine.supported(model, opt) == want


def test_executor_leaves_codes_wider_than_the_kernels_to_the_trainer():
    from nerf2mesh_amd.engine import Stage0Engine
    from nerf2mesh_amd.fused import ind_max_dim
    cap = constant_colour_capture()
    assert ind_max_dim() == 16
    for d, want in ((1, True), (16, True), (17, False)):
        opt = _options(ind_dim=d, ind_num=16)
        assert Stage0Engine.supported(_model(opt), opt, capture=cap) == want


def test_fused_field_is_off_without_device_tensors():
    """_can_fuse needs the tables on the GPU: on the host every form of `c` runs the unfused network."""
    from nerf2mesh_amd.fused import IndCode
    opt = _options(ind_dim=8, ind_num=16)
    model = _model(opt)
    assert not model._can_fuse() and not model._can_fuse(IndCode(model.individual_codes))
    assert torch.is_tensor(model.ind_code()) and model.ind_code().shape == (1, 8)
    assert torch.equal(model.ind_code(torch.tensor([2, 0], dtype=torch.int32)), model.individual_codes[[2, 0]])
    assert _model(_options()).ind_code() is None


def test_state_dict_has_the_reference_names_and_shapes():
    opt = _options(ind_dim=8, ind_num=23)
    sd = _model(opt).state_dict()
    assert tuple(sd["individual_codes"].shape) == (23, 8)
    assert tuple(sd["color_net.net.0.weight"].shape) == (64, 35 + 8)
    sd0 = _model(_options()).state_dict()
    assert "individual_codes" not in sd0 and tuple(sd0["color_net.net.0.weight"].shape) == (64, 35)


def test_trainer_names_both_numbers_when_the_capture_has_more_views_than_codes():
    from nerf2mesh_amd.trainer import Stage0Trainer
    cap = constant_colour_capture()
    opt = _options(ind_dim=8, ind_num=V - 1)
    with pytest.raises(ValueError, match=rf"{V} views.*ind_num is {V - 1}"):
        Stage0Trainer(_model(opt), opt, None, torch.device("cpu"), capture=cap)
    opt = _options(ind_dim=8, ind_num=V)
    Stage0Trainer(_model(opt), opt, None, torch.device("cpu"), capture=cap)
    with pytest.raises(ValueError, match="captured image set"):
        from nerf2mesh_amd import synthetic
        Stage0Trainer(_model(opt), opt, synthetic.make_cameras(4, seed=0), torch.device("cpu"))


def test_cpu_batch_view_ids_are_the_views_the_pixels_were_read_from():
    from nerf2mesh_amd.trainer import Stage0Trainer
    cap = constant_colour_capture()
    opt = _options(ind_dim=8, ind_num=V, fused_mlp=False)
    opt.num_rays = 257
    tr = Stage0Trainer(_model(opt), opt, None, torch.device("cpu"), seed=3, capture=cap)
    seen = set()
    for _ in range(4):
        _, _, rgba, _, _ = tr.batch()
        ids = tr._index
        assert ids.dtype == torch.int32 and ids.shape == (257,)
        read = torch.round(rgba[:, 0] * 255).to(torch.int32)
        assert torch.equal(ids, read)
        seen.update(ids.tolist())
    assert seen == set(range(V)), seen
    # the edges of the expression: u = 0 is view 0, the largest fp32 below 1 is the last view, and a product that rounds up to V stays inside
    u = torch.zeros(3, 6)
    u[1, 0] = float(np.nextafter(np.float32(1), np.float32(0)))
    u[2, 0] = 1.0
    assert batch_views(u, V).tolist() == [0, V - 1, V - 1]
    # without codes no ids are made
    opt0 = _options(fused_mlp=False)
    tr0 = Stage0Trainer(_model(opt0), opt0, None, torch.device("cpu"), seed=3, capture=cap)
    tr0.batch()
    assert tr0._index is None


def test_cpu_sparse_depth_batch_has_the_batch_view_for_every_ray():
    from nerf2mesh_amd.trainer import Stage0Trainer
    cap = Capture.load_colmap(TINY, split="train", sparse_depth=True)
    opt = _options(ind_dim=4, ind_num=len(cap), fused_mlp=False, enable_sparse_depth=True, iters=1000)
    opt.num_rays = 64
    tr = Stage0Trainer(_model(opt), opt, None, torch.device("cpu"), seed=5, capture=cap)
    depth_batches = 0
    for _ in range(40):
        o, _, _, _, _ = tr.batch()
        view = tr.depth_schedule.log[-1]
        assert tr._index.shape == (o.shape[0],)
        if view is not None:
            depth_batches += 1
            assert (tr._index == view).all()
    assert depth_batches >= 2
