"""bench.py's own contract on one GPU: a plain run times exactly `--steps` steps and measures nothing beyond the headline (the extras
are behind --full), and `--dump-outputs DIR` writes the last timed step's outputs as float32 .npy files of bounded size."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_step(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2", "--pretrain", "24",
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, r.stdout[-1500:] + r.stderr[-1500:]
    d = json.loads(lines[0])
    assert d["metric"] == "train_samples_per_sec" and d["value"] > 0 and d["higher_is_better"] is True and d["dtype"]
    assert d["steps"] == 6 and d["ms_per_step"] > 0
    assert d["config"]["timed_steps"] == [d["config"]["pretrain_steps"] + 2 + 1, d["config"]["pretrain_steps"] + 2 + 6]
    # nothing of --full in a plain run
    assert not d["kernels"] and d["roofline"] is None and d["long_run"] is None and d["other_configs"] is None
    assert d["cpu_baseline"] is None and d["psnr_view0_quarter_res"] is None

    files = sorted(glob.glob(str(out / "*.npy")))
    names = {os.path.basename(f)[:-4] for f in files}
    assert {"loss", "num_points", "encoder.embeddings.sample", "encoder_color.embeddings.sample", "sigma_net.net.0.weight",
            "density_grid.sample"} <= names, names
    assert sum(os.path.getsize(f) for f in files) <= 64 << 20
    arrays = {os.path.basename(f)[:-4]: np.load(f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert np.isfinite(arrays["loss"]).all() and arrays["loss"][0] > 0 and arrays["num_points"][0] > 0
    assert np.abs(arrays["encoder.embeddings.sample"]).max() > 0
