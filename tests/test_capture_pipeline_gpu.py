"""tools/train_capture.py end to end on a set written with Capture.save_nerf: load -> stage 0 -> export_stage0 -> stage 1 -> export_stage1,
in a fresh process.  No quality threshold: a 48 x 64 set and a few hundred steps say nothing about quality."""
import json
import math
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_train_capture_runs_both_stages(tmp_path):
    from nerf2mesh_amd import synthetic
    from nerf2mesh_amd.capture import Capture
    intr = (70.0, 60.0, 30.5, 25.25)
    data, work = str(tmp_path / "set"), str(tmp_path / "work")
    Capture.synthetic(synthetic.make_cameras(6, seed=0), H=48, W=64, intrinsics=intr).save_nerf(data, split="train")
    Capture.synthetic(synthetic.make_cameras(2, seed=1), H=48, W=64, intrinsics=intr).save_nerf(data, split="test")
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "train_capture.py"), data, "--workspace", work, "--scale", "1",
           "--iters0", "400", "--iters1", "30", "--texture", "512", "--decimate_target", "20000"]
    run = subprocess.run(cmd, capture_output=True, text=True)
    print(run.stdout[-4000:])
    print(run.stderr[-4000:])
    assert run.returncode == 0
    assert os.path.exists(os.path.join(work, "mesh_stage0", "mesh_0.ply"))
    for name in ("mesh_0.obj", "feat0_0.jpg", "feat1_0.jpg", "mlp.json"):
        assert os.path.exists(os.path.join(work, "mesh_stage1", name)), name
    res = json.loads(run.stdout.strip().splitlines()[-1])
    assert res["held_out_is_test_split"] and res["held_out_views"] == 2 and (res["H"], res["W"]) == (48, 64)
    assert math.isfinite(res["psnr_stage0"]) and math.isfinite(res["psnr_stage1"])
    assert res["faces"] > 0
