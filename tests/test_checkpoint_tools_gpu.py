"""The front ends on checkpoints: tools/train_capture.py saves as it goes and, started again, trains only what is left; tools/render_path.py
then renders from the workspace without training.  The tiny set of tests/test_capture_pipeline_gpu.py; every tool runs in a fresh process
under its own time limit."""
import glob
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(limit, name, *args):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.join(ROOT, "tools", name), *args]
    run = subprocess.run(cmd, capture_output=True, text=True)
    print(run.stdout[-3000:])
    print(run.stderr[-3000:])
    assert run.returncode == 0, name
    return run.stdout


@pytest.mark.gpu
def test_train_capture_resumes_and_render_path_loads(tmp_path):
    from nerf2mesh_amd import synthetic
    from nerf2mesh_amd.capture import Capture
    intr = (70.0, 60.0, 30.5, 25.25)
    data, work = str(tmp_path / "set"), str(tmp_path / "work")
    Capture.synthetic(synthetic.make_cameras(6, seed=0), H=48, W=64, intrinsics=intr).save_nerf(data, split="train")
    common = [data, "--workspace", work, "--scale", "1", "--texture", "256", "--decimate_target", "20000", "--n_ckpt", "20"]
    out = _tool(240, "train_capture.py", *common, "--iters0", "60", "--iters1", "12")
    res = json.loads(out.strip().splitlines()[-1])
    assert res["trained0"] == 60 and res["trained1"] == 12 and res["resumed0"] is None and res["resumed1"] is None
    assert "[ckpt] stage 0: from scratch, 60 steps to train" in out
    ckpts = sorted(os.path.basename(f) for f in glob.glob(os.path.join(work, "checkpoints", "*.pth")))
    assert [c for c in ckpts if "_stage0_" in c] == ["ngp_stage0_ep0006.pth", "ngp_stage0_ep0010.pth"], ckpts      # steps 40 and 60; step 20's rotated out
    assert [c for c in ckpts if "_stage1_" in c] == ["ngp_stage1_ep0002.pth"], ckpts

    # again, with more steps asked for: the default --ckpt latest trains only what is left of either stage
    out = _tool(240, "train_capture.py", *common, "--iters0", "80", "--iters1", "20")
    res = json.loads(out.strip().splitlines()[-1])
    assert res["trained0"] == 20 and res["trained1"] == 8, res
    assert res["resumed0"].endswith("ngp_stage0_ep0010.pth") and res["resumed1"].endswith("ngp_stage1_ep0002.pth")
    assert re.search(r"\[ckpt\] stage 0: .*ngp_stage0_ep0010\.pth \(full\) at step 60, 20 steps to train", out)
    assert re.search(r"\[ckpt\] stage 1: .*ngp_stage1_ep0002\.pth \(full\) at step 12, 8 steps to train", out)
    assert "export_stage0" not in out.split("[ckpt] stage 1")[0].split("[stage 0]")[1], "the stage-1 file brings its mesh: no second extraction"

    # a camera path from the trained field: nothing is trained
    out = _tool(240, "render_path.py", work, "--data", data, "--source", "field", "--iters0", "0", "--n_test", "1")
    res = json.loads(out.strip().splitlines()[-1])
    assert re.search(r"\[stage 0\] loaded .*ngp_stage0_ep0013\.pth \(step 80\), 0 steps trained", out)
    assert res["frames"] > 0 and res["files"] >= 2 * res["frames"]
    assert len(glob.glob(os.path.join(work, "results", "*_rgb.png"))) == res["frames"]

    # without a checkpoint, --iters0 0 stays an error
    empty = str(tmp_path / "empty")
    cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.join(ROOT, "tools", "render_path.py"), empty, "--data", data, "--iters0", "0"]
    run = subprocess.run(cmd, capture_output=True, text=True)
    assert run.returncode != 0 and "needs a stage-0 checkpoint" in run.stderr
