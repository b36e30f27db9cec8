"""CPU: the pose-refinement entry points are declared, bound and refuse bad arguments on the host (no GPU needed); the option, the
combinations the trainer refuses, the checkpoint rule, and the tools' flags."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("n2m_pose_apply", "n2m_pose_ray_grad", "n2m_pose_view_grad")


@pytest.fixture(scope="module")
def L():
    from nerf2mesh_amd import _lib, build
    build.build(verbose=False)
    return _lib


def test_symbols_are_declared_and_bound_with_matching_argument_lists(L):
    import ctypes
    src = open(os.path.join(ROOT, "include", "n2m_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    kinds = {"uint32_t": ctypes.c_uint32, "int": ctypes.c_int, "float": ctypes.c_float}
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in include/n2m_hip.h"
        want = []
        for arg in m.group(1).split(","):
            arg = arg.strip()
            want.append(ctypes.c_void_p if "*" in arg else kinds[arg.replace("const ", "").split()[0]])
        assert L.SIGNATURES[name] == want, name
        assert hasattr(L.lib(), name)
    assert os.path.exists(os.path.join(ROOT, "nerf2mesh_amd", "csrc", "posegrad.hip"))
    from nerf2mesh_amd import pose_refine
    assert float(re.search(r"#define\s+N2M_POSE_SERIES_THETA\s+(\S+)", src).group(1)) == pose_refine.SERIES_THETA


p = 16                                                                     # a stand-in for a device pointer: nothing is dereferenced


def test_null_pointers_and_empty_tensors_are_refused_before_any_launch(L):
    EINVAL = r"\(-1\)"
    calls = {"n2m_pose_apply": ([p, p, 4, p], (0, 1, 3), (2,)),
             "n2m_pose_ray_grad": ([p, p, p, p, p, p, 8, 2, p], (0, 3, 4, 5, 8), (6, 7)),
             "n2m_pose_view_grad": ([p, p, p, 8, 2, p], (0, 1, 2, 5), (3, 4))}
    for name, (args, pointers, sizes) in calls.items():
        for hole in pointers:
            a = list(args)
            a[hole] = None
            with pytest.raises(RuntimeError, match=name + r" failed " + EINVAL + ".*NULL"):
                L.call(name, *a, None)
        for hole in sizes:
            a = list(args)
            a[hole] = 0
            with pytest.raises(RuntimeError, match=name + r" failed " + EINVAL):
                L.call(name, *a, None)


def test_the_options():
    from nerf2mesh_amd.options import make_options
    opt = make_options()
    assert opt.optimize_poses is False and opt.lr_pose == 1e-3
    assert make_options(optimize_poses=True, lr_pose=5e-4).lr_pose == 5e-4
    for wrong in ("optimise_poses", "optimize_pose", "pose_lr"):
        with pytest.raises(TypeError, match="unknown option"):
            make_options(**{wrong: True})


def _capture(V=3, HW=8):
    from nerf2mesh_amd import synthetic
    from nerf2mesh_amd.capture import Capture, pack_rgba8
    images = torch.full((V, HW, HW, 4), 128, dtype=torch.uint8)
    bank, alpha = pack_rgba8(images)
    return Capture(synthetic.make_cameras(V, seed=0), bank, HW, HW, (10.0, 10.0, HW / 2, HW / 2), has_alpha=alpha, device="cpu")


def _trainer(capture, world_size=1, **over):
    from nerf2mesh_amd import synthetic
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    from nerf2mesh_amd.trainer import Stage0Trainer
    opt = make_options(bound=1, dt_gamma=0, **over)
    poses = None if capture is not None else synthetic.make_cameras(2, seed=0)
    return Stage0Trainer(NeRFNetwork(opt), opt, poses, torch.device("cpu"), capture=capture, world_size=world_size)


def test_unsupported_combinations_raise():
    cap = _capture()
    with pytest.raises(ValueError, match="needs a captured image set"):
        _trainer(None, optimize_poses=True)
    with pytest.raises(ValueError, match="fused_mlp=False"):
        _trainer(cap, optimize_poses=True, fused_mlp=True)
    with pytest.raises(ValueError, match="sdf=True"):
        _trainer(cap, optimize_poses=True, sdf=True)
    with pytest.raises(ValueError, match="more than one rank"):
        _trainer(cap, optimize_poses=True, world_size=2)


def test_the_trainer_with_the_option_on():
    cap = _capture()
    off = _trainer(cap)
    assert off.refiner is None and off.model.ray_attach is None and off.pipeline is True and off._stepper is off.optimizer
    tr = _trainer(cap, optimize_poses=True, lr_pose=2e-3)
    assert tr.pipeline is False and tr.model.ray_attach == tr.refiner.attach
    assert tr.poses is tr.refiner.poses() and torch.equal(tr.poses, cap.poses)
    assert tr.refiner.delta.shape == (3, 6) and float(tr.refiner.delta.detach().abs().max()) == 0
    assert tr.refiner.optimizer.param_groups[0]["initial_lr"] == 2e-3
    assert tr.refiner.optimizer.param_groups[0]["lr"] == pytest.approx(2e-3 * 0.01)          # the trainer's schedule: the warm-up starts at 1 %
    groups = tr._stepper.param_groups
    assert groups[-1]["params"][0] is tr.refiner.delta and len(groups) == len(tr.optimizer.param_groups) + 1


def test_the_refiner_uses_the_trainers_schedule():
    from nerf2mesh_amd import trainer
    from nerf2mesh_amd.pose_refine import PoseRefiner
    ref = PoseRefiner(_capture().poses, lr=1.0, iters=2000)
    f = trainer.lr_schedule(2000)
    for step in (0, 1, 499, 500, 501, 1999):
        ref.scheduler.last_epoch = step
        ref.scheduler._apply()
        assert ref.optimizer.param_groups[0]["lr"] == f(step)


def test_refined_capture_and_the_pose_table_on_the_cpu():
    from nerf2mesh_amd.pose_refine import PoseRefiner
    cap = _capture()
    ref = PoseRefiner(cap.poses, lr=1e-3, iters=1000)
    same = ref.refined(cap)
    assert torch.equal(same.poses, cap.poses) and torch.allclose(same.mvps, cap.mvps) and same.bank is cap.bank
    with torch.no_grad():
        ref.delta[1] = torch.tensor([0.0, 0.0, 0.1, 0.5, 0.0, 0.0])
    buf = ref.poses()
    assert buf is ref.poses() and torch.equal(buf[0], cap.poses[0]) and not torch.equal(buf[1], cap.poses[1])
    moved = ref.refined(cap)
    assert float(moved.poses[1, 0, 3] - cap.poses[1, 0, 3]) == pytest.approx(0.5, abs=1e-6)
    assert not torch.allclose(moved.mvps[1], cap.mvps[1]) and torch.equal(cap.poses, ref.poses0)


def test_state_dict_round_trip_and_the_checkpoint_rule():
    from nerf2mesh_amd import checkpoint
    cap = _capture()
    a = _trainer(cap, optimize_poses=True)
    with torch.no_grad():
        a.refiner.delta.normal_(generator=torch.Generator().manual_seed(1)).mul_(0.01)
    a.refiner.delta.grad = torch.ones_like(a.refiner.delta)
    a.refiner.optimizer.step()
    sd = a.state_dict()
    assert set(sd["n2m"]["pose_refine"]) == {"delta", "poses0_checksum", "optimizer", "last_epoch"}
    b = _trainer(cap, optimize_poses=True)
    b.load_state_dict(sd)
    assert torch.equal(b.refiner.delta, a.refiner.delta) and torch.equal(b.poses, a.refiner.poses()) and b.poses is b.refiner.poses()
    sa, sb = a.refiner.optimizer.state_dict()["state"][0], b.refiner.optimizer.state_dict()["state"][0]
    assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]) and float(sa["step"]) == float(sb["step"]) == 1
    plain = _trainer(cap)
    assert "pose_refine" not in plain.state_dict()["n2m"]
    with pytest.raises(ValueError, match="disagree on optimize_poses"):
        plain.load_state_dict(sd)                                          # a file with the feature, a run without
    with pytest.raises(ValueError, match="disagree on optimize_poses"):
        b.load_state_dict(plain.state_dict())
    plain.load_state_dict(sd, model_only=True)                             # the model alone is always welcome
    other = _capture()
    other.poses[0, 0, 3] += 1.0
    with pytest.raises(ValueError, match="checksum"):
        _trainer(other, optimize_poses=True).load_state_dict(sd)
    assert checkpoint.FORMAT == 1


@pytest.mark.parametrize("tool", ["train_capture.py", "evaluate.py"])
def test_the_tools_take_the_flags(tool):
    src = open(os.path.join(ROOT, "tools", tool)).read()
    assert 'add_argument("--optimize_poses", action="store_true"' in src and 'add_argument("--lr_pose", type=float, default=1e-3' in src
    assert "optimize_poses=args.optimize_poses" in src and "lr_pose=args.lr_pose" in src and "poses_refined.npy" in src
    assert "refiner.refined(cap)" in src and "stored poses" in src


def test_the_flags_parse():
    """The tools run as scripts; their parser is built by the lines in front of parse_args(): run exactly those."""
    src = open(os.path.join(ROOT, "tools", "train_capture.py")).read()
    head = src[src.index("ap = argparse.ArgumentParser"):src.index("args = ap.parse_args()")]
    ns = {"argparse": __import__("argparse"), "__doc__": ""}
    exec(compile(head, "train_capture_parser", "exec"), ns)
    args = ns["ap"].parse_args(["PATH", "--workspace", "W", "--optimize_poses", "--lr_pose", "5e-4"])
    assert args.optimize_poses is True and args.lr_pose == 5e-4
    assert ns["ap"].parse_args(["PATH", "--workspace", "W"]).optimize_poses is False
