"""nerf2mesh_amd/camera_path.py on the host: the paths against tests/golden/camera_path.npz (scipy's Slerp in float64, written by
tests/golden/make_golden_camera_path.py), CameraPath's Capture interface, the torch statement of n2m_frame_pack against a float64 numpy
restatement of nerf/utils.py:978-986, and save_frames read back through PIL.

Pose bound: 1e-6 on every entry.  The rotation entries are <= 1 in magnitude and both sides compute in float64 from the same fp32 key
poses (the product casts to fp32 once), so the bound is 16 fp32 ulps of 1.

frame_pack bound: bytes equal, except where the float64 value of 255 x lies within 1e-3 of an integer; there one level of difference is
allowed (fp32 against float64 may fall on either side of the truncation).  At most 1 % of the elements may use that excuse: for uniform
inputs the bands cover 0.2 % of the range.  Measured when the test was written (seed 3, 20000 pixels): none of the 60000 RGB bytes in
either colour space, and 1 of the 20000 depth bytes (0.005 %), used it."""
import os

import numpy as np
import pytest
import torch

from nerf2mesh_amd import camera_path as CP
from nerf2mesh_amd.camera_path import CameraPath
from nerf2mesh_amd.capture import Capture, proj_matrix

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "camera_path.npz")
H, W = 5, 7
INTR = (9.5, 7.25, 3.3, 2.85)


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _capture(poses, intrinsics=INTR, per_view=None):
    V = len(poses)
    images = torch.randint(0, 256, (V, H, W, 4), generator=torch.Generator().manual_seed(V), dtype=torch.uint8)
    return Capture.from_arrays(torch.from_numpy(np.asarray(poses, dtype=np.float32)), images, intrinsics, per_view=per_view)


CASES = [("poses", "keys_a", "n_test_a", "between_a"), ("poses", "keys_b", "n_test_b", "between_b"),
         ("poses_far", None, "n_test_far", "between_far"), ("poses", (2, 2), "n_test_same", "between_same")]


def _case(gold, case):
    src, keys, n_test, want = case
    keys = [0, 1] if keys is None else [int(k) for k in (gold[keys] if isinstance(keys, str) else keys)]
    return gold[src], keys, int(gold[n_test]), gold[want]


@pytest.mark.parametrize("case", CASES, ids=[c[3] for c in CASES])
def test_between_against_scipy(gold, case):
    poses, keys, n_test, want = _case(gold, case)
    path = CameraPath.between(_capture(poses), n_test=n_test, keys=keys)
    got = path.poses.numpy()
    assert got.dtype == np.float32 and got.shape == want.shape == ((len(keys) - 1) * (n_test + 1), 4, 4) and len(path) == got.shape[0]
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"{case[3]}: max |delta| = {err:.3e}")
    assert err <= 1e-6
    # the key poses themselves, bit for bit, at both ends of every segment
    for s, (a, b) in enumerate(zip(keys[:-1], keys[1:])):
        assert np.array_equal(got[s * (n_test + 1)].view(np.int32), poses[a].view(np.int32))
        assert np.array_equal(got[s * (n_test + 1) + n_test].view(np.int32), poses[b].view(np.int32))
    R = got[:, :3, :3].astype(np.float64)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-6
    assert (np.linalg.det(R) > 0).all() and np.abs(np.linalg.det(R) - 1).max() <= 1e-6
    assert np.array_equal(got[:, 3], np.tile(np.float32([0, 0, 0, 1]), (len(got), 1)))


def test_the_far_pair_takes_the_shortest_arc(gold):
    """179 degrees apart: the middle frame is 89.5 degrees from both keys (the long way round it would be 90.5)."""
    poses, keys, n_test, _ = _case(gold, CASES[2])
    got = CameraPath.between(_capture(poses), n_test=n_test, keys=keys).poses.numpy().astype(np.float64)
    assert n_test % 2 == 0
    mid = got[n_test // 2, :3, :3]
    for k in (0, 1):
        cos = (np.trace(mid @ poses[k, :3, :3].astype(np.float64).T) - 1) / 2
        assert abs(np.rad2deg(np.arccos(cos)) - 89.5) < 1e-3


def test_circle_against_the_reference_construction(gold):
    path = CameraPath.circle((H, W, INTR), n=8)
    assert len(path) == 8 and (path.H, path.W, path.intrinsics) == (H, W, INTR) and path.device.type == "cpu"
    assert np.abs(path.poses.numpy().astype(np.float64) - gold["circle"]).max() <= 1e-6
    cap = _capture(gold["poses"])
    full = CameraPath.circle(cap)
    assert len(full) == 100 and (full.H, full.W) == (cap.H, cap.W) and full.intrinsics == cap.intrinsics
    assert np.abs(np.linalg.norm(full.poses[:, :3, 3].numpy(), axis=-1) - 0.1).max() < 1e-7


def test_seeded_keys_and_frame_count(gold):
    cap = _capture(gold["poses"])
    for seed, n_keys, n_test in ((0, 5, 3), (7, 3, 2), (1, 50, 1)):
        path = CameraPath.between(cap, n_test=n_test, n_keys=n_keys, seed=seed)
        want = np.random.RandomState(seed).choice(7, min(n_keys, 7), replace=False)
        assert path.keys == [int(k) for k in want]
        assert len(path) == (len(want) - 1) * (n_test + 1)
    assert len(CameraPath.between(cap)) == 4 * 25                                   # the defaults: 5 keys, n_test = 24
    two = CameraPath.between(_capture(gold["poses"][:2]))
    assert sorted(two.keys) == [0, 1] and len(two) == 25


def test_fewer_than_two_views_raise(gold):
    with pytest.raises(ValueError, match="at least 2 views"):
        CameraPath.between(_capture(gold["poses"][:1]))
    with pytest.raises(ValueError, match="at least 2 keys"):
        CameraPath.between(_capture(gold["poses"]), keys=[3])
    with pytest.raises(ValueError, match="at least 2 keys"):
        CameraPath.between(_capture(gold["poses"]), keys=[3, 7])
    with pytest.raises(ValueError, match=r"\[F,4,4\]"):
        CameraPath(np.eye(4), H, W, INTR)


def test_a_per_view_capture_hands_row_zero(gold):
    rows = np.array([[9.5 + v, 7.25 - 0.125 * v, 3.3 + 0.0625 * v, 2.85] for v in range(7)])
    cap = _capture(gold["poses"], intrinsics=rows)
    assert cap.per_view_intrinsics
    path = CameraPath.between(cap, n_test=2, keys=[4, 1])
    assert path.intrinsics == tuple(float(x) for x in rows[0]) and path.intrinsics_of(2) == path.intrinsics
    assert CameraPath.circle(cap, n=4).intrinsics == path.intrinsics


def test_the_capture_interface(gold):
    cap = _capture(gold["poses"])
    keys, n_test = [3, 0, 5], 4
    path = CameraPath.between(cap, n_test=n_test, keys=keys)
    assert (path.H, path.W, path.device, path.cam_near_far) == (cap.H, cap.W, cap.device, None)
    assert path.poses.dtype == torch.float32 and tuple(path.poses.shape) == (10, 4, 4) and tuple(path.mvps.shape) == (10, 4, 4)
    proj = proj_matrix(H, W, *INTR)
    for f in range(len(path)):
        assert torch.equal(path.mvps[f], proj @ torch.inverse(path.poses[f]))
    for f, v in ((0, 3), (4, 0), (5, 0), (9, 5)):
        assert torch.equal(path.mvps[f], cap.mvps[v])
        for stride, ssaa in ((1, 0), (1, 2), (2, 1)):
            o, d, rgba, dirs = path.view(f, stride=stride, dirs_ssaa=ssaa)
            wo, wd, _, wdirs = cap.view(v, stride=stride, dirs_ssaa=ssaa)
            assert rgba is None and torch.equal(o, wo) and torch.equal(d, wd)
            assert (dirs is None and wdirs is None) if ssaa == 0 else torch.equal(dirs, wdirs)
    # explicit poses
    own = CameraPath(gold["poses"][1:3], H, W, INTR)
    assert len(own) == 2 and torch.equal(own.view(1)[1], cap.view(2)[1])


# ------------------------------------------------------------------------------------------------------ frames as bytes
def _model64(image, depth, linear):
    """nerf/utils.py:978-986 in float64 numpy on the fp32 inputs (with the stated clamp): the values whose truncation is the byte."""
    x = np.clip(image.astype(np.float64), 0, 1)
    if linear:
        with np.errstate(invalid="ignore"):
            x = np.clip(np.where(x < 0.0031308, 12.92 * x, 1.055 * x ** 0.41666 - 0.055), 0, 1)
    d = depth.astype(np.float64)
    return x * 255, (d - d.min()) / (d.max() - d.min() + 1e-6) * 255


def check_bytes(got, value64, cap=0.01, what=""):
    """got == floor(value64), except within 1e-3 of an integer, where one level either way is allowed; returns the share that used it."""
    got, want = np.asarray(got).astype(np.int64).reshape(-1), np.floor(value64).astype(np.int64).reshape(-1)
    off = got != want
    near = np.abs(value64.reshape(-1) - np.rint(value64.reshape(-1))) <= 1e-3
    share = float(off.mean()) if off.size else 0.0
    print(f"{what}: {int(off.sum())} of {off.size} bytes differ from the float64 model ({100 * share:.4f} %)")
    assert (near | ~off).all(), f"{what}: a byte differs away from a truncation boundary"
    assert np.abs(got - want)[off].max(initial=0) <= 1
    assert share <= cap
    return share


@pytest.mark.parametrize("linear", [False, True])
def test_frame_pack_torch_against_float64(linear):
    g = torch.Generator().manual_seed(3)
    n = 20000
    image = torch.rand(n, 3, generator=g) * 1.2 - 0.1                  # some below 0 and above 1
    depth = torch.rand(n, generator=g) * 4.5 + 0.25
    image[0] = torch.tensor([0.0, 1.0, -0.0])
    image[1] = torch.tensor([0.0031308, 0.5, 2.0])
    rgb, dep = CP.frame_pack_torch(image, depth, linear)
    assert rgb.dtype == torch.uint8 and dep.dtype == torch.uint8 and rgb.shape == image.shape and dep.shape == depth.shape
    v_rgb, v_dep = _model64(image.numpy(), depth.numpy(), linear)
    check_bytes(rgb.numpy(), v_rgb, what=f"rgb linear={linear}")
    check_bytes(dep.numpy(), v_dep, what="depth")
    assert int(dep.min()) == 0 and int(dep.max()) in (254, 255)
    assert rgb[0].tolist() == ([0, 254, 0] if linear else [0, 255, 0]) and int(rgb[1, 2]) == (254 if linear else 255)


def test_frame_pack_edges_on_the_host():
    k = torch.arange(256, dtype=torch.float32)
    image = (k / 255).view(-1, 1).expand(-1, 3).contiguous()
    rgb, dep = CP.frame_pack(image, torch.full((256,), 2.5))
    want = (image * 255).to(torch.uint8)
    assert torch.equal(rgb, want) and (rgb[:, 0].long() - k.long()).abs().max() <= 1      # k / 255 * 255 may land just below k
    assert torch.equal(dep, torch.zeros(256, dtype=torch.uint8))                          # a constant frame
    out = (torch.zeros(16, 16, 3, dtype=torch.uint8), torch.zeros(16, 16, dtype=torch.uint8))
    depth = torch.linspace(1, 3, 256)
    assert CP.frame_pack(image, depth, out=out) is out
    assert torch.equal(out[0].view(-1, 3), want) and torch.equal(out[1].view(-1), CP.frame_pack_torch(image, depth)[1])
    assert int(out[1].view(-1)[0]) == 0 and int(out[1].view(-1)[-1]) == 254              # (2 / (2 + 1e-6)) * 255 is below 255
    with pytest.raises(ValueError, match="not one frame"):
        CP.frame_pack(image, depth[:-1])


def test_render_path_on_the_host(gold):
    path = CameraPath.between(_capture(gold["poses"]), n_test=2, keys=[1, 4])
    frames = {f: (torch.rand(H * W, 3, generator=torch.Generator().manual_seed(f)), torch.rand(H * W, generator=torch.Generator().manual_seed(9 + f)))
              for f in range(3)}
    seen = []

    def render(f):
        seen.append(f)
        return {"image": frames[f][0], "depth": frames[f][1].view(H, W)}
    rgb, dep = CP.render_path(render, path)
    assert seen == [0, 1, 2] and rgb.shape == (3, H, W, 3) and dep.shape == (3, H, W) and rgb.dtype == dep.dtype == torch.uint8
    for f in range(3):
        wr, wd = CP.frame_pack_torch(*frames[f])
        assert torch.equal(rgb[f].view(-1, 3), wr) and torch.equal(dep[f].view(-1), wd)
    sub, _ = CP.render_path(render, path, frames=[2, 0])
    assert torch.equal(sub[0], rgb[2]) and torch.equal(sub[1], rgb[0])


def test_save_frames_reads_back(tmp_path):
    from PIL import Image
    g = torch.Generator().manual_seed(4)
    F, h, w = 4, 5, 7                                                                     # odd sizes: nothing is padded
    rgb = torch.randint(0, 256, (F, h, w, 3), generator=g, dtype=torch.uint8)
    dep = torch.randint(0, 256, (F, h, w), generator=g, dtype=torch.uint8)
    files = CP.save_frames(rgb, dep, str(tmp_path / "results"), "ngp_ep0001")
    assert sorted(os.listdir(tmp_path / "results")) == sorted(os.path.basename(f) for f in files) and len(files) == 2 * F
    for i in range(F):
        with Image.open(tmp_path / "results" / f"ngp_ep0001_{i:04d}_rgb.png") as im:
            assert im.mode == "RGB" and np.array_equal(np.asarray(im), rgb[i].numpy())
        with Image.open(tmp_path / "results" / f"ngp_ep0001_{i:04d}_depth.png") as im:
            assert im.mode == "L" and np.array_equal(np.asarray(im), dep[i].numpy())
    files = CP.save_frames(rgb, dep, str(tmp_path / "video"), "run", video="apng")
    assert len(files) == 2 * F + 2
    for kind, stack, mode in (("rgb", rgb, "RGB"), ("depth", dep, "L")):
        with Image.open(tmp_path / "video" / f"run_{kind}.apng") as im:
            assert im.n_frames == F
            for k in range(F):
                im.seek(k)
                assert np.array_equal(np.asarray(im.convert(mode)), stack[k].numpy()), (kind, k)
    with pytest.raises(ValueError, match="video"):
        CP.save_frames(rgb, dep, str(tmp_path / "x"), "run", video="mp4")


def test_options_and_the_front_end_path(gold):
    from nerf2mesh_amd.options import make_options
    assert make_options().camera_traj == ""
    cap = _capture(gold["poses"])
    assert len(CP.path_for(cap, make_options(camera_traj="circle"))) == 100
    assert len(CP.path_for(cap, make_options(), n_test=3)) == 4 * 4
    with pytest.raises(ValueError, match="camera_traj"):
        CP.path_for(cap, make_options(camera_traj="spiral"))


def test_no_scipy_in_the_product():
    import glob
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name in glob.glob(os.path.join(root, "nerf2mesh_amd", "**", "*.py"), recursive=True):
        assert not re.search(r"^\s*(from|import)\s+scipy\b", open(name).read(), flags=re.M), name
