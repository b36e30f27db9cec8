"""capture.Capture on the host: loading a nerf-format set by the rules of nerf/provider.py:150-263 (sizes, focal lengths, principal point,
extension-less file names, nerf_matrix_to_ngp), the packed bank against the PNG bytes, the save / load round trip, the integer box
downscale, and the agreement of the rays with the model-view-projection built from the same intrinsics."""
import json
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

from nerf2mesh_amd import synthetic
from nerf2mesh_amd.capture import Capture, box_downscale, pack_rgba8

V, H, W = 3, 6, 10


def _ngp(pose, scale, offset):
    """nerf_matrix_to_ngp (nerf/provider.py:16-19) restated."""
    pose = np.array(pose, dtype=np.float32)
    pose[:3, 3] = pose[:3, 3] * scale + np.array(offset)
    return pose.astype(np.float32)


def _write_set(root, channels, how, h=H, w=W):
    rng = np.random.default_rng(channels * 10 + (how == "angle"))
    images = rng.integers(0, 256, (V, h, w, channels), dtype=np.uint8)
    images[0, 0, 0] = 255
    images[0, 0, 1] = 0
    poses = synthetic.make_cameras(V, seed=5).double().numpy()
    frames = []
    os.makedirs(os.path.join(root, "train"), exist_ok=True)
    for v in range(V):
        Image.fromarray(images[v]).save(os.path.join(root, "train", f"r_{v}.png"))
        frames.append({"file_path": f"./train/r_{v}" + ("" if how == "angle" else ".png"), "transform_matrix": poses[v].tolist()})
    meta = {"frames": frames}
    if how == "angle":
        meta["camera_angle_x"] = 0.6911112070083618
    else:
        meta.update(fl_x=11.25, fl_y=12.5, cx=4.75, cy=3.25, h=h, w=w)
    with open(os.path.join(root, "transforms_train.json"), "w") as f:
        json.dump(meta, f)
    return images, poses


@pytest.mark.parametrize("channels", [4, 3])
@pytest.mark.parametrize("how", ["fl", "angle"])
def test_load_nerf_follows_the_provider_rules(tmp_path, channels, how):
    images, poses = _write_set(str(tmp_path), channels, how)
    scale, offset = 0.8, (0.1, -0.2, 0.05)
    cap = Capture.load_nerf(str(tmp_path), split="train", scale=scale, offset=offset)
    assert (len(cap), cap.H, cap.W) == (V, H, W)
    want = np.stack([_ngp(p, scale, offset) for p in poses])
    assert np.array_equal(cap.poses.numpy(), want)
    if how == "fl":
        assert cap.intrinsics == (11.25, 12.5, 4.75, 3.25)
    else:
        f = W / (2 * math.tan(0.6911112070083618 / 2))
        assert cap.intrinsics == (f, f, W / 2.0, H / 2.0)
    by = cap.bank_bytes().numpy()
    assert np.array_equal(by[..., :channels], images)
    assert cap.has_alpha == (channels == 4)
    if channels == 3:
        assert (by[..., 3] == 255).all()
    # R in the low byte of the packed word
    word = cap.bank[0, 1].item() & 0xFFFFFFFF
    assert word & 255 == images[0, 0, 1, 0] and (word >> 8) & 255 == images[0, 0, 1, 1] and (word >> 16) & 255 == images[0, 0, 1, 2]


def test_transforms_json_is_the_fallback(tmp_path):
    _write_set(str(tmp_path), 4, "fl")
    os.rename(tmp_path / "transforms_train.json", tmp_path / "transforms.json")
    assert len(Capture.load_nerf(str(tmp_path), split="train")) == V
    with pytest.raises(FileNotFoundError):
        Capture.load_nerf(str(tmp_path / "train"))


@pytest.mark.parametrize("channels", [4, 3])
def test_save_then_load_is_the_identity(tmp_path, channels):
    _write_set(str(tmp_path / "a"), channels, "fl")
    a = Capture.load_nerf(str(tmp_path / "a"), scale=0.8, offset=(0.1, -0.2, 0.05))
    a.save_nerf(str(tmp_path / "b"), split="test")
    b = Capture.load_nerf(str(tmp_path / "b"), split="test", scale=1.0)
    assert torch.equal(a.poses, b.poses) and torch.equal(a.bank, b.bank) and torch.equal(a.mvps, b.mvps)
    assert (a.H, a.W, a.intrinsics, a.has_alpha) == (b.H, b.W, b.intrinsics, b.has_alpha)
    im = Image.open(tmp_path / "b" / "test" / "r_0.png")
    assert im.mode == ("RGBA" if channels == 4 else "RGB")


def test_downscale_is_the_integer_block_mean(tmp_path):
    images, _ = _write_set(str(tmp_path), 4, "fl", h=7, w=10)
    cap = Capture.load_nerf(str(tmp_path), downscale=2)
    assert (cap.H, cap.W) == (3, 5)
    blocks = images[:, :6, :10].astype(np.int64).reshape(V, 3, 2, 5, 2, 4)
    want = (blocks.sum((2, 4)) + 2) // 4
    assert np.array_equal(cap.bank_bytes().numpy(), want.astype(np.uint8))
    assert cap.intrinsics == (11.25 / 2, 12.5 / 2, 4.75 / 2, 3.25 / 2)
    # k = 3: two columns and one row are dropped
    bank, _ = pack_rgba8(images)
    got = box_downscale(bank, 7, 10, 3).view(torch.uint8).view(V, 2, 3, 4).numpy()
    b3 = images[:, :6, :9].astype(np.int64).reshape(V, 2, 3, 3, 3, 4)
    assert np.array_equal(got, ((b3.sum((2, 4)) + 4) // 9).astype(np.uint8))


def test_rays_and_raster_agree_off_centre():
    """For every pixel of a 5 x 7 view the point o + 3 d of its ray, pushed through mvps[v], lands on window coordinates (i + 0.5, j + 0.5).
    Bound: 1e-3 px -- fp32 arithmetic on coordinates below 10 (a few ulp of 10 = 1e-6 relative, times the image size)."""
    h, w = 5, 7
    poses = synthetic.make_cameras(3, seed=2)
    cap = Capture.from_arrays(poses, np.zeros((3, h, w, 3), np.uint8), (9.5, 7.25, 3.3, 2.85))
    for v in range(3):
        o, d, _, _ = cap.view(v)
        p = torch.cat([o + 3 * d, torch.ones(h * w, 1)], -1) @ cap.mvps[v].T
        ndc = p[:, :2] / p[:, 3:]
        wx, wy = (ndc[:, 0] * 0.5 + 0.5) * w, (ndc[:, 1] * 0.5 + 0.5) * h
        jj, ii = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        assert (wx - (ii.reshape(-1) + 0.5)).abs().max() < 1e-3
        assert (wy - (jj.reshape(-1) + 0.5)).abs().max() < 1e-3
        assert (p[:, 3] > 0).all()


def test_centred_square_intrinsics_give_the_synthetic_mvp():
    poses = synthetic.make_cameras(4, seed=0)
    cap = Capture.from_arrays(poses, np.zeros((4, 8, 8, 4), np.uint8), (synthetic.LEGO_FOCAL * 8 / 800, synthetic.LEGO_FOCAL * 8 / 800, 4.0, 4.0))
    want = torch.stack([synthetic.mvp_matrix(p, 8, 8, synthetic.LEGO_FOCAL * 8 / 800) for p in poses])
    assert torch.equal(cap.mvps, want)
    lego = Capture.from_arrays(poses[:1], np.zeros((1, 2, 2, 4), np.uint8), (1.0, 1.0, 1.0, 1.0))
    assert lego.mvps.shape == (1, 4, 4)


def test_synthetic_quantises_render_gt():
    poses = synthetic.make_cameras(2, seed=0)
    intr = (70.0, 60.0, 30.5, 25.25)
    cap = Capture.synthetic(poses, H=48, W=64, intrinsics=intr)
    o, d, rgba, _ = cap.view(1)
    want = (synthetic.render_gt(o, d) * 255 + 0.5).to(torch.uint8)
    assert torch.equal(cap.bank_bytes()[1].view(-1, 4), want)
    assert torch.equal(rgba, want.float() / 255)
    assert cap.has_alpha and 0 < (want[:, 3] == 255).float().mean() < 1
    rgb = Capture.synthetic(poses, H=48, W=64, intrinsics=intr, alpha=False)
    assert not rgb.has_alpha and (rgb.bank_bytes()[..., 3] == 255).all()
