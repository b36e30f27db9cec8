"""csrc/campath.hip and nerf2mesh_amd/camera_path.py on the device.

n2m_path_view against n2m_capture_view on the same pose, intrinsics and size: the same bits.  n2m_frame_pack against the torch statement
(camera_path.frame_pack_torch) evaluated on the same device tensors: exact byte equality for the depth and for sRGB-space RGB (clamp,
multiply, subtract, add, divide and truncate are correctly rounded fp32 operations on both sides); under linear=1 the device's powf and
torch's pow are different approximations, so those bytes are compared against the float64 model of tests/test_camera_path_cpu.py with its
one-level excuse within 1e-3 of a truncation boundary and its 1 % cap.  Then the three renderers on a CameraPath whose keys are training
views, and tools/render_path.py in a fresh process."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_camera_path_cpu import _model64, check_bytes   # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTR = (9.5, 7.25, 3.3, 2.85)          # fx != fy, principal point off-centre by a non-integer amount
BLOCK = 256                            # the workgroup size of both frame_pack kernels
COUNTS = [1, 63, 64, 65, 480, 2 * BLOCK + 3, 256 * BLOCK + 259]      # the last: more than 256 workgroups' worth, where the reduction strides


# ------------------------------------------------------------------------------------------------------ n2m_path_view
@pytest.mark.parametrize("H,W", [(20, 24), (1, 1), (3, 65)])
def test_path_view_has_the_bits_of_capture_view(H, W):
    from nerf2mesh_amd import synthetic
    from nerf2mesh_amd.camera_path import CameraPath
    from nerf2mesh_amd.capture import Capture
    V = 3
    poses = synthetic.make_cameras(V, seed=1)
    images = torch.randint(0, 256, (V, H, W, 4), generator=torch.Generator().manual_seed(H), dtype=torch.uint8)
    cap = Capture.from_arrays(poses, images, INTR, device="cuda")
    gpu, cpu = CameraPath(poses, H, W, INTR, device="cuda"), CameraPath(poses, H, W, INTR)
    assert gpu.device == cap.device and torch.equal(gpu.mvps, cap.mvps) and torch.equal(gpu.poses, cap.poses)
    for stride in (1, 2):
        h, w = H // stride, W // stride
        for ssaa in (0, 1, 2):
            for f in range(V):
                got = gpu.view(f, stride=stride, dirs_ssaa=ssaa)
                host = cpu.view(f, stride=stride, dirs_ssaa=ssaa)
                torch.cuda.synchronize()
                assert got[2] is None and got[0].shape == (h * w, 3) and got[1].shape == (h * w, 3)
                assert (got[3] is None) if ssaa == 0 else got[3].shape == (h * ssaa * w * ssaa, 3)
                want = cap.view(f, stride=stride, dirs_ssaa=ssaa) if h * w else host          # (an empty grid launches nothing)
                for k, name in ((0, "rays_o"), (1, "rays_d"), (3, "dirs")):
                    if got[k] is None:
                        assert want[k] is None and host[k] is None
                        continue
                    assert torch.equal(got[k], want[k].to(got[k].device)), (stride, ssaa, f, name)
                    assert torch.equal(got[k].cpu(), host[k]), (stride, ssaa, f, name, "against the torch statement")


def test_path_view_refuses_bad_arguments():
    from nerf2mesh_amd import _lib as L
    with pytest.raises(RuntimeError, match="frame < F"):
        L.call("n2m_path_view", 16, 2, 2, 4, 4, 1, 1.0, 1.0, 2.0, 2.0, 16, 16, None, 1, None)
    with pytest.raises(RuntimeError, match="ssaa must be 1..8"):
        L.call("n2m_path_view", 16, 2, 0, 4, 4, 1, 1.0, 1.0, 2.0, 2.0, 16, 16, 16, 9, None)
    with pytest.raises(RuntimeError, match="NULL"):
        L.call("n2m_frame_pack", 16, 16, 4, 0, 16, None, 16, None)


# ------------------------------------------------------------------------------------------------------ n2m_frame_pack
def _frame(n, lo_at, hi_at, seed=0):
    """n pixels: colours in [-0.1, 1.1) with the special values in front, depth in [1, 2) with its minimum 0.5 at lo_at and its maximum
    3 at hi_at."""
    g = torch.Generator().manual_seed(seed + n)
    image = torch.rand(n, 3, generator=g) * 1.2 - 0.1
    special = torch.tensor([0.0, -0.0, 1.0, -0.5, 1.5, 0.0031308, 0.5, 1e-30, 0.999999])
    flat = image.view(-1)
    flat[:min(len(special), 3 * n)] = special[:3 * n]
    depth = torch.rand(n, generator=g) + 1.0
    depth[lo_at], depth[hi_at] = 0.5, 3.0
    return image.cuda(), depth.cuda()


def _placements(n):
    """(index of the minimum, index of the maximum): first / last element both ways round, and either side of a workgroup boundary."""
    if n == 1:
        return [(0, 0)]
    out = [(0, n - 1), (n - 1, 0)]
    if n > BLOCK:
        out += [(BLOCK - 1, BLOCK), (BLOCK, BLOCK - 1)]
    return out


@pytest.mark.parametrize("n", COUNTS)
def test_frame_pack_equals_the_torch_statement(n):
    from nerf2mesh_amd.camera_path import frame_pack, frame_pack_torch
    for lo_at, hi_at in _placements(n):
        image, depth = _frame(n, lo_at, hi_at)
        guard = torch.full((4 * n + 16,), 77, dtype=torch.uint8, device="cuda")            # both outputs inside one buffer, rgb at an odd offset
        out = (guard[1:1 + 3 * n].view(n, 3), guard[3 * n + 9:4 * n + 9])
        got = frame_pack(image, depth, out=out)
        want = frame_pack_torch(image, depth)
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]), (n, lo_at, hi_at, "rgb")
        assert torch.equal(got[1], want[1]), (n, lo_at, hi_at, "depth")
        assert (guard[:1] == 77).all() and (guard[1 + 3 * n:3 * n + 9] == 77).all() and (guard[4 * n + 9:] == 77).all(), "wrote outside its outputs"
        if n > 1:
            assert int(got[1][lo_at]) == 0 and int(got[1][hi_at]) == 254 and int(got[1].max()) == 254      # 2.5 / (2.5 + 1e-6) * 255 < 255
            assert got[0].view(-1)[:5].tolist() == [0, 0, 255, 0, 255]
        again = frame_pack(image, depth)
        assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])            # two runs, bit for bit


def test_frame_pack_special_frames():
    from nerf2mesh_amd.camera_path import frame_pack, frame_pack_torch
    k = torch.arange(256, dtype=torch.float32, device="cuda")
    image = (k / 255).view(-1, 1).expand(-1, 3).contiguous()                               # k / 255 exactly as fp32 divides it, every k
    const = torch.full((256,), 2.5, device="cuda")
    rgb, dep = frame_pack(image, const)
    want = frame_pack_torch(image, const)
    assert torch.equal(rgb, want[0]) and torch.equal(rgb.cpu(), frame_pack_torch(image.cpu(), const.cpu())[0])
    assert torch.equal(dep, torch.zeros_like(dep)) and torch.equal(dep, want[1])           # a constant frame gives zeros
    # a wide range: max - min + 1e-6 rounds to max - min, the ratio reaches 1 and the byte 255
    depth = torch.linspace(0, 1000, 256, device="cuda")
    dep = frame_pack(image, depth)[1]
    assert torch.equal(dep, frame_pack_torch(image, depth)[1]) and int(dep[0]) == 0 and int(dep[-1]) == 255
    # shaped inputs [H,W,3] / [H,W] give shaped outputs
    rgb2, dep2 = frame_pack(image.view(16, 16, 3), depth.view(16, 16))
    assert rgb2.shape == (16, 16, 3) and dep2.shape == (16, 16) and torch.equal(dep2.view(-1), dep)


def test_frame_pack_linear_against_float64():
    from nerf2mesh_amd.camera_path import frame_pack
    n = 20000
    image, depth = _frame(n, 7, 11, seed=3)
    rgb, dep = frame_pack(image, depth, linear=True)
    v_rgb, v_dep = _model64(image.cpu().numpy(), depth.cpu().numpy(), True)
    check_bytes(rgb.cpu().numpy(), v_rgb, what="device rgb, linear")
    check_bytes(dep.cpu().numpy(), v_dep, what="device depth")
    # exact on 0, the branch point of linear_to_srgb and its fp32 neighbours, and 1
    t = torch.tensor(0.0031308)
    x = torch.stack([torch.tensor(0.0), torch.nextafter(t, torch.tensor(0.0)), t, torch.nextafter(t, torch.tensor(1.0)), torch.tensor(1.0),
                     torch.tensor(0.25)]).view(2, 3)
    got = frame_pack(x.cuda(), torch.tensor([1.0, 2.0], device="cuda"), linear=True)[0].cpu().numpy()
    want = np.floor(_model64(x.numpy(), np.float32([1, 2]), True)[0]).astype(np.uint8)
    print("linear edge bytes:", got.reshape(-1).tolist(), "float64 model:", want.reshape(-1).tolist())
    assert np.array_equal(got.reshape(-1)[:5], want.reshape(-1)[:5])
    again = frame_pack(image, depth, linear=True)
    assert torch.equal(again[0], rgb) and torch.equal(again[1], dep)


# ------------------------------------------------------------------------------------------------------ end to end
H, W, V, STEPS = 20, 24, 7, 30
KEYS, N_TEST = [2, 5, 0], 2


@pytest.fixture(scope="module")
def trained():
    from nerf2mesh_amd import synthetic
    from nerf2mesh_amd.camera_path import CameraPath
    from nerf2mesh_amd.capture import Capture
    from nerf2mesh_amd.engine import Stage0Engine
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    f = synthetic.LEGO_FOCAL * H / synthetic.LEGO_HW
    cap = Capture.synthetic(synthetic.make_cameras(V, seed=0), H=H, W=W, intrinsics=(f, f, W / 2, H / 2), device="cuda")
    torch.manual_seed(0)
    opt = make_options(O=True, bound=1, dt_gamma=0, iters=30000, fused_mlp=True)
    opt.num_rays, opt.num_points = 1024, 1 << 14
    eng = Stage0Engine(NeRFNetwork(opt), opt, None, torch.device("cuda", 0), seed=0, capture=cap)
    eng.mark_untrained()
    for _ in range(STEPS):
        eng.train_step()
    torch.cuda.synchronize()
    path = CameraPath.between(cap, n_test=N_TEST, keys=KEYS)
    return {"cap": cap, "eng": eng, "model": eng.model.eval(), "path": path, "opt": opt}


KEY_FRAMES = [(0, 2), (2, 5), (3, 5), (5, 0)]          # (frame, the training view whose pose it is)


def _same_at_the_keys(on_path, on_capture):
    for f, v in KEY_FRAMES:
        a, b = on_path(f), on_capture(v)
        for k in ("image", "depth"):
            assert torch.equal(a[k], b[k]), (f, v, k)
    return on_path


def test_field_frames(trained):
    from nerf2mesh_amd import metrics
    from nerf2mesh_amd.camera_path import render_path
    cap, path, model = trained["cap"], trained["path"], trained["model"]
    assert len(path) == 6 and path.cam_near_far is None and cap.cam_near_far is None
    render = _same_at_the_keys(metrics.field_renderer(model, path), metrics.field_renderer(model, cap))
    rgb, depth = render_path(render, path)
    torch.cuda.synchronize()
    assert rgb.shape == (6, H, W, 3) and depth.shape == (6, H, W) and rgb.dtype == depth.dtype == torch.uint8 and rgb.is_cuda and depth.is_cuda
    confirmed = 0
    for f in range(len(path)):
        res = render(f)
        v_rgb, v_dep = _model64(res["image"].cpu().numpy(), res["depth"].cpu().numpy(), False)
        check_bytes(rgb[f].cpu().numpy(), v_rgb, what=f"frame {f} rgb")
        check_bytes(depth[f].cpu().numpy(), v_dep, what=f"frame {f} depth")
        print(f"frame {f}: depth {float(res['depth'].min()):.4f} .. {float(res['depth'].max()):.4f}, bytes {int(depth[f].min())} .. {int(depth[f].max())}")
        assert int(depth[f].min()) == 0
        assert float(res["depth"].max()) > float(res["depth"].min()), "the field rendered a constant depth"
        if np.floor(v_dep).max() == 255:                          # (only a range wide enough for max - min + 1e-6 to round to max - min gets there)
            confirmed += 1
            assert int(depth[f].max()) == 255
        else:
            assert int(depth[f].max()) in (int(np.floor(v_dep).max()), int(np.floor(v_dep).max()) + 1)
    print("frames whose float64 model reaches 255:", confirmed)
    # an in-between frame is neither of its keys
    for f, keys in ((1, (0, 2)), (4, (3, 5))):
        for k in keys:
            assert not torch.equal(rgb[f], rgb[k]) and not torch.equal(path.poses[f], path.poses[k])
    sub = render_path(render, path, frames=[4, 1])
    assert torch.equal(sub[0][0], rgb[4]) and torch.equal(sub[1][1], depth[1])


@pytest.fixture(scope="module")
def stage1(trained):
    from nerf2mesh_amd import synthetic
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    from nerf2mesh_amd.trainer import Stage1Trainer
    torch.manual_seed(0)
    opt = make_options(O=True, bound=1, dt_gamma=0, iters=30000, fused_mlp=True, stage=1, ssaa=2)
    v, f = synthetic.scene_mesh(6000)
    tr = Stage1Trainer(NeRFNetwork(opt), opt, None, v, f, torch.device("cuda", 0), capture=trained["cap"])
    return tr.model.eval()


def test_mesh_frames(trained, stage1):
    from nerf2mesh_amd import metrics
    from nerf2mesh_amd.camera_path import render_path
    cap, path = trained["cap"], trained["path"]
    render = _same_at_the_keys(metrics.mesh_renderer(stage1, path), metrics.mesh_renderer(stage1, cap))
    assert stage1.last_covered > 0, "the mesh is in front of the path's cameras"
    rgb, depth = render_path(render, path)
    assert rgb.shape == (6, H, W, 3) and depth.shape == (6, H, W)
    assert all(int(depth[f].min()) == 0 for f in range(6)) and not torch.equal(rgb[1], rgb[0]) and not torch.equal(rgb[1], rgb[2])


def test_asset_frames(trained, stage1, tmp_path):
    from nerf2mesh_amd import metrics
    from nerf2mesh_amd.asset import ExportedAsset
    from nerf2mesh_amd.camera_path import render_path
    cap, path = trained["cap"], trained["path"]
    stage1.export_stage1(str(tmp_path), 512, 512)
    asset = ExportedAsset.load(str(tmp_path))
    render = _same_at_the_keys(metrics.asset_renderer(asset, path, ssaa=2), metrics.asset_renderer(asset, cap, ssaa=2))
    rgb, depth = render_path(render, path)
    assert rgb.shape == (6, H, W, 3) and depth.shape == (6, H, W) and not torch.equal(rgb[4], rgb[3]) and not torch.equal(rgb[4], rgb[5])


def test_render_path_tool_in_a_fresh_process(tmp_path):
    from PIL import Image
    work = str(tmp_path / "work")
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "render_path.py"), work, "--source", "field", "--views", str(V),
           "--size", str(H), "--width", str(W), "--iters0", str(STEPS), "--n_test", "2", "--name", "run"]
    run = subprocess.run(cmd, capture_output=True, text=True)
    print(run.stdout[-3000:])
    print(run.stderr[-3000:])
    assert run.returncode == 0
    F = 4 * 3                                                       # 5 keys of the 7 views, n_test + 1 frames per segment
    names = sorted(os.listdir(os.path.join(work, "results")))
    assert names == sorted([f"run_{i:04d}_rgb.png" for i in range(F)] + [f"run_{i:04d}_depth.png" for i in range(F)])
    for name in names:
        with Image.open(os.path.join(work, "results", name)) as im:
            assert im.size == (W, H) and im.mode == ("RGB" if name.endswith("_rgb.png") else "L")
