"""CPU side of dense-depth supervision: the torch statements the kernels are compared against (capture.batch_from_uniforms_u8 with a depth
bank, capture.resize_linear_at / dense_depth_fill), the option's error cases, and the trainer's batches on CPU tensors."""
import numpy as np
import pytest
import torch

from nerf2mesh_amd import capture as C
from nerf2mesh_amd import synthetic

H, W, V, N = 10, 12, 5, 70
INTR = (14.0, 13.0, 6.5, 4.25)


def _case(channels=4, cnf=True):
    g = torch.Generator().manual_seed(3)
    images = torch.randint(0, 256, (V, H, W, channels), generator=g, dtype=torch.uint8)
    poses = synthetic.make_cameras(V, seed=1)
    near_far = synthetic.cam_near_far(poses, "lego", H, W, INTR[0]) if cnf else None
    cap = C.Capture.from_arrays(poses, images, INTR, cam_near_far=near_far)
    cap.dense_depth = torch.rand(V, H * W, generator=g) * 4
    u = torch.rand(N, 6, generator=g)
    u[0, :2] = 0.0                                        # first view, first pixel
    u[1, 0], u[1, 1] = 0.999999, 0.999999                 # last view, last pixel
    u[2, 0], u[2, 1] = 1.0, 1.0                           # a uniform of exactly 1 is clamped to the last view and pixel
    u[3, 0], u[3, 1] = 0.0, 0.999999                      # first view, last pixel
    return cap, u


@pytest.mark.parametrize("channels,cnf", [(4, True), (3, False)])
def test_depth_batch_statement_equals_the_plain_one_and_gathers_the_bank(channels, cnf):
    cap, u = _case(channels, cnf)
    aabb = torch.tensor([-1.0, -1, -1, 1, 1, 1])
    plain = C.batch_from_uniforms_u8(cap.poses, cap.bank, cap.lut, u, aabb, 0.05, H, W, INTR, cam_near_far=cap.cam_near_far)
    got = C.batch_from_uniforms_u8(cap.poses, cap.bank, cap.lut, u, aabb, 0.05, H, W, INTR, cam_near_far=cap.cam_near_far, dense_depth=cap.dense_depth)
    assert len(plain) == 7 and len(got) == 8
    for a, b in zip(plain, got):
        assert a.dtype == b.dtype and torch.equal(a, b)
    # the (view, pixel) the statement chose, restated in float32 as the kernel casts it
    cam = np.minimum((u[:, 0].numpy() * np.float32(V)).astype(np.int64), V - 1)
    pix = np.minimum((u[:, 1].numpy() * np.float32(H * W)).astype(np.int64), H * W - 1)
    assert (cam[:4] == [0, V - 1, V - 1, 0]).all() and (pix[:4] == [0, H * W - 1, H * W - 1, H * W - 1]).all()
    assert got[7].shape == (N,) and got[7].dtype == torch.float32
    assert np.array_equal(got[7].numpy(), cap.dense_depth.numpy()[cam, pix])
    # ... which is where the colour came from
    assert torch.equal(got[2], C.decode_words(cap.bank[torch.from_numpy(cam), torch.from_numpy(pix)], cap.lut))
    with pytest.raises(ValueError, match="depth bank"):
        C.batch_from_uniforms_u8(cap.poses, cap.bank, cap.lut, u, aabb, 0.05, H, W, INTR, dense_depth=cap.dense_depth[:, :-1])


def test_resize_identity_at_equal_size():
    m = torch.rand(H, W, generator=torch.Generator().manual_seed(0)) * 9 - 2
    assert torch.equal(C.dense_depth_fill(m, H, W).view(H, W), m)
    assert torch.equal(C.dense_depth_fill(m, H, W, 2.5, -0.75).view(H, W), m * torch.tensor(2.5) + torch.tensor(-0.75))
    out = torch.empty(H * W)
    assert C.dense_depth_fill(m, H, W, out=out) is out and torch.equal(out.view(H, W), m)
    with pytest.raises(ValueError, match="2-D fp32"):
        C.dense_depth_fill(m.double(), H, W)


def test_resize_reproduces_the_corners_of_a_two_by_two_source():
    """The output's corner pixels have source coordinates below 0 or above 1 on both axes ((0 + 0.5) * 2 / 12 - 0.5 < 0): both taps of either
    axis are clamped onto the same source pixel, and a + (a - a) * t is a."""
    m = torch.tensor([[1.25, -3.5], [7.0, 0.1]])
    out = C.dense_depth_fill(m, H, W).view(H, W)
    assert out[0, 0] == m[0, 0] and out[0, W - 1] == m[0, 1] and out[H - 1, 0] == m[1, 0] and out[H - 1, W - 1] == m[1, 1]
    # a 1 x 1 source fills the image
    assert torch.equal(C.dense_depth_fill(torch.tensor([[4.5]]), 3, 2), torch.full((6,), 4.5))
    # between the corners the values stay inside the source's range and the rows in between are monotone in x
    assert out.min() >= m.min() and out.max() <= m.max()
    assert (out[0, 1:] <= out[0, :-1]).all() and (out[H - 1, 1:] <= out[H - 1, :-1]).all()


@pytest.mark.parametrize("h,w", [(5, 7), (20, 24), (10, 12)])
def test_resize_keeps_a_linear_ramp(h, w):
    """src(y, x) = 3 + 0.5 x - 0.25 y sampled at the source pixel centres.  Where no tap is clamped the bilinear value is the ramp at the
    source coordinate (sx, sy) = ((X + 0.5) w / W - 0.5, (Y + 0.5) h / H - 0.5).  Error: the coordinate carries the fp32 rounding of the
    ratio and of two operations (3 x 2^-24 relative of a coordinate below 24), the weight one more, each lerp two roundings of values
    below 16, three lerps: below (4 x 24 x 0.5 + 6 x 16) x 2^-24 < 1e-5 absolute."""
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    src = (3 + 0.5 * xs - 0.25 * ys).float()
    out = C.dense_depth_fill(src, H, W).view(H, W).double()
    sy = (torch.arange(H, dtype=torch.float64) + 0.5) * h / H - 0.5
    sx = (torch.arange(W, dtype=torch.float64) + 0.5) * w / W - 0.5
    inside = ((sy >= 0) & (sy <= h - 1))[:, None] & ((sx >= 0) & (sx <= w - 1))[None, :]
    assert inside.sum() >= (H - 2) * (W - 2)
    want = 3 + 0.5 * sx[None, :] - 0.25 * sy[:, None]
    err = (out - want).abs()[inside].max().item()
    print(f"{h} x {w} -> {H} x {W}: ramp error {err:.3g}")
    assert err < 1e-5
    # outside, the clamped taps hold the edge's value: the ramp at the clamped coordinate
    wantc = 3 + 0.5 * sx.clamp(0, w - 1)[None, :] - 0.25 * sy.clamp(0, h - 1)[:, None]
    assert (out - wantc).abs().max().item() < 1e-5


def test_option_and_its_error_cases():
    from nerf2mesh_amd.options import make_options
    assert make_options().enable_dense_depth is False
    cap, _ = _case()
    on = make_options(enable_dense_depth=True)
    assert C.dense_depth_for(cap, make_options()) is None
    assert C.dense_depth_for(cap, on) is cap.dense_depth
    with pytest.raises(ValueError, match="needs a capture"):
        C.dense_depth_for(None, on)
    bare = C.Capture.from_arrays(cap.poses, cap.bank_bytes(), INTR)
    with pytest.raises(ValueError, match="no dense-depth bank"):
        C.dense_depth_for(bare, on)
    with pytest.raises(ValueError, match="exclude each other"):
        C.dense_depth_for(cap, make_options(enable_dense_depth=True, enable_sparse_depth=True))


def test_trainer_batches_carry_the_bank_on_every_step():
    """Stage0Trainer.batch() on CPU tensors: every batch has num_rays rays and a depth target, weight None (1), from the same draw a run
    without the option makes its batch of."""
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    from nerf2mesh_amd.trainer import Stage0Trainer
    cap, _ = _case()

    def trainer(**over):
        torch.manual_seed(0)
        opt = make_options(bound=1, dt_gamma=0, iters=1000, **over)
        opt.num_rays = 64
        return Stage0Trainer(NeRFNetwork(opt), opt, None, torch.device("cpu"), seed=5, capture=cap)
    on, off = trainer(enable_dense_depth=True), trainer()
    assert on.depth_schedule is None and off.dense_depth is None
    for _ in range(5):
        a, b = on.batch(), off.batch()
        assert off._depth is None
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        gtd, dw = on._depth
        assert dw is None and gtd.shape == (64,)
        # the target belongs to the ray: its colour is at the same (view, pixel)
        hit = (cap.decode().view(-1, 4)[:, None] == a[2][None]).all(-1)          # [V*H*W, 64]
        assert all((cap.dense_depth.view(-1)[hit[:, n]] == gtd[n]).any() for n in range(64))
    with pytest.raises(ValueError, match="needs a capture"):
        torch.manual_seed(0)
        opt = make_options(bound=1, dt_gamma=0, enable_dense_depth=True)
        Stage0Trainer(NeRFNetwork(opt), opt, synthetic.make_cameras(4), torch.device("cpu"), seed=5)
