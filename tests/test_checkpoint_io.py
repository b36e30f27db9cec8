"""nerf2mesh_amd/checkpoint.py without a device: the file, the folder (names, "latest", rotation, a save that dies), the format version, the
two forms of the optimizer state, and the learning-rate schedule."""
import glob
import os
import types

import pytest
import torch

from nerf2mesh_amd import checkpoint as C


class FakeDriver:
    """The least a driver is to checkpoint.py: opt.stage / opt.workspace, global_step, epoch_len, state_dict() / load_state_dict()."""

    def __init__(self, workspace, stage=0, epoch_len=4):
        self.opt = types.SimpleNamespace(stage=stage, workspace=str(workspace))
        self.global_step, self.epoch_len, self.world = 0, epoch_len, 1
        self.weight = torch.arange(6, dtype=torch.float32).reshape(2, 3)
        self.loaded = None

    def state_dict(self):
        return {"epoch": self.global_step // self.epoch_len, "global_step": self.global_step, "stats": self.stats, "stage": self.opt.stage,
                "mean_density": 0.25, "model": {"w": self.weight + self.global_step}, "optimizer": {"state": {}, "param_groups": []},
                "lr_scheduler": {"last_epoch": self.global_step}, "scaler": {}, "ema": {"decay": 0.95, "num_updates": 3, "shadow_params": [self.weight * 2],
                                                                                        "collected_params": None},
                "n2m": {"options": {"bound": 1, "name": "x"}, "samples_seen": 7 * self.global_step, "gen": torch.arange(16, dtype=torch.uint8)}}

    def load_state_dict(self, sd, model_only=False):
        self.loaded = (sd, model_only)
        if not model_only:
            self.global_step = sd["global_step"]


def _driver(tmp_path, **kw):
    d = FakeDriver(tmp_path, **kw)
    d.stats = C.new_stats()
    return d


def test_round_trip_holds_tensors_and_plain_values_only(tmp_path):
    d = _driver(tmp_path)
    d.global_step = 9
    path = C.save_checkpoint(d, str(tmp_path))
    assert path == os.path.join(str(tmp_path), "checkpoints", "ngp_stage0_ep0002.pth")
    sd = torch.load(path, weights_only=True)                       # no pickled class: the restricted loader reads it
    for k in ("epoch", "global_step", "stats", "stage", "mean_density", "model", "optimizer", "lr_scheduler", "scaler", "ema", "n2m"):
        assert k in sd, k
    assert sd["epoch"] == 2 and sd["global_step"] == 9 and sd["stage"] == 0 and sd["mean_density"] == 0.25
    assert torch.equal(sd["model"]["w"], d.weight + 9) and torch.equal(sd["ema"]["shadow_params"][0], d.weight * 2)
    assert sd["n2m"]["n2m_format"] == C.FORMAT and sd["n2m"]["samples_seen"] == 63 and sd["n2m"]["options"] == {"bound": 1, "name": "x"}
    assert torch.equal(sd["n2m"]["gen"], torch.arange(16, dtype=torch.uint8))
    assert sd["stats"]["checkpoints"] == ["ngp_stage0_ep0002.pth"]
    assert set(sd) == {"epoch", "global_step", "stats", "stage", "mean_density", "model", "optimizer", "lr_scheduler", "scaler", "ema", "n2m"}
    # full=False: the model and the counters alone
    slim = torch.load(C.save_checkpoint(d, str(tmp_path / "slim.pth"), full=False), weights_only=True)
    assert "model" in slim and not {"optimizer", "lr_scheduler", "scaler", "ema"} & set(slim)
    e = _driver(tmp_path)
    assert C.load_checkpoint(e) == path and e.global_step == 9 and e.loaded[1] is False
    assert C.load_checkpoint(e, path, model_only=True) == path and e.loaded[1] is True


def test_names_latest_and_rotation(tmp_path):
    ws = str(tmp_path)
    assert C.latest_checkpoint(ws, 0) is None and C.load_checkpoint(_driver(tmp_path)) is None
    d = _driver(tmp_path)
    written = []
    for step in (4, 8, 12):
        d.global_step = step
        written.append(C.save_checkpoint(d, ws, max_keep=2))
    names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(ws, "checkpoints", "*")))
    assert names == ["ngp_stage0_ep0002.pth", "ngp_stage0_ep0003.pth"], "at most max_keep, the oldest removed first"
    assert d.stats["checkpoints"] == names
    assert C.latest_checkpoint(ws, 0) == written[-1]
    # the same epoch again: the file is replaced, not listed twice
    d.global_step = 13
    C.save_checkpoint(d, ws, max_keep=2)
    assert d.stats["checkpoints"] == names
    assert torch.load(C.latest_checkpoint(ws, 0), weights_only=True)["global_step"] == 13
    # a best file is no candidate for "latest", however it sorts
    d.stats["results"].append(0.5)
    best = C.save_checkpoint(d, ws, best=True)
    assert os.path.basename(best) == "ngp_stage0.pth" and C.latest_checkpoint(ws, 0) == written[-1]
    assert C.best_checkpoint(ws, 0) == best
    d.stats["results"].append(0.7)                                  # not better (lower is better): nothing written
    assert C.save_checkpoint(d, ws, best=True) is None and d.stats["best_result"] == 0.5
    d.stats["results"].append(0.25)
    assert C.save_checkpoint(d, ws, best=True) == best and d.stats["best_result"] == 0.25
    assert C.save_checkpoint(_driver(tmp_path), ws, best=True) is None, "no evaluated result: no best file"
    # stage 1 asked for while only stage-0 files are there
    assert C.latest_checkpoint(ws, 1) is None
    s1 = _driver(tmp_path, stage=1)
    assert C.restore_or_init(s1, ws, "latest") == (written[-1], "model_only") and s1.loaded[1] is True and s1.global_step == 0
    s1.global_step = 5
    p1 = C.save_checkpoint(s1, ws)
    assert os.path.basename(p1) == "ngp_stage1_ep0001.pth" and C.latest_checkpoint(ws, 1) == p1 and C.latest_checkpoint(ws, 0) == written[-1]
    s1b = _driver(tmp_path, stage=1)
    assert C.restore_or_init(s1b, ws, "latest") == (p1, "full") and s1b.global_step == 5
    assert C.restore_or_init(_driver(tmp_path, stage=1), ws, "scratch") == (None, None)
    assert C.restore_or_init(_driver(tmp_path, stage=1), ws, written[-1]) == (written[-1], "model_only"), "a stage-0 path handed to stage 1"
    assert C.restore_or_init(_driver(tmp_path), ws, "best") == (best, "model_only")
    empty = str(tmp_path / "empty")
    assert C.restore_or_init(_driver(empty), empty, "latest") == (None, None)


def test_interrupted_save_leaves_the_previous_file(tmp_path, monkeypatch):
    ws = str(tmp_path)
    d = _driver(tmp_path)
    d.global_step = 4
    first = C.save_checkpoint(d, ws)
    d.global_step = 8

    def dies(src, dst):
        assert os.path.exists(src), "the temporary file is complete when the save dies"
        raise OSError("power cut")
    monkeypatch.setattr(os, "replace", dies)
    with pytest.raises(OSError):
        C.save_checkpoint(d, ws)
    monkeypatch.undo()
    assert glob.glob(os.path.join(ws, "checkpoints", "*.pth")) == [first], "the glob sees no partial file"
    assert os.listdir(os.path.join(ws, "checkpoints")) == [os.path.basename(first)], "and the temporary file is gone"
    assert d.stats["checkpoints"] == [os.path.basename(first)]
    assert C.latest_checkpoint(ws, 0) == first and torch.load(first, weights_only=True)["global_step"] == 4
    # the same epoch: the file that was there stays whole
    d.global_step = 5
    monkeypatch.setattr(os, "replace", dies)
    with pytest.raises(OSError):
        C.save_checkpoint(d, ws)
    monkeypatch.undo()
    assert torch.load(first, weights_only=True)["global_step"] == 4


def test_newer_format_raises(tmp_path):
    d = _driver(tmp_path)
    path = C.save_checkpoint(d, str(tmp_path))
    sd = torch.load(path, weights_only=True)
    sd["n2m"]["n2m_format"] = C.FORMAT + 1
    torch.save(sd, path)
    with pytest.raises(ValueError, match="newer"):
        C.load_checkpoint(_driver(tmp_path), path)
    with pytest.raises(ValueError, match="newer"):
        C.restore_or_init(_driver(tmp_path), str(tmp_path))
    with pytest.raises(NotImplementedError):
        two = _driver(tmp_path)
        two.world = 2
        C.save_checkpoint(two, str(tmp_path))


def _torch_forms():
    g = torch.Generator().manual_seed(3)
    shapes = [(5, 1), (5, 2), (4, 3), (1,)]
    state = {i: {"step": torch.tensor(float(s)), "exp_avg": torch.randn(sh, generator=g), "exp_avg_sq": torch.rand(sh, generator=g)}
             for i, (sh, s) in enumerate(zip(shapes, (40, 40, 17, 0)))}       # parameter 2 joined late, parameter 3 never stepped
    groups = [{"lr": 1e-2, "betas": (0.9, 0.99), "eps": 1e-15, "weight_decay": 0, "amsgrad": False, "maximize": False, "foreach": None,
               "capturable": False, "differentiable": False, "fused": None, "decoupled_weight_decay": False, "initial_lr": 2e-2, "params": [0, 1]},
              {"lr": 1e-3, "betas": (0.9, 0.99), "eps": 1e-15, "weight_decay": 0, "amsgrad": False, "maximize": False, "foreach": None,
               "capturable": False, "differentiable": False, "fused": None, "decoupled_weight_decay": False, "initial_lr": 2e-3, "params": [2, 3]}]
    scaler = {"scale": 8192.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000, "_growth_tracker": 731}
    return {"state": state, "param_groups": groups}, scaler


def test_optimizer_forms_convert_without_loss():
    opt_sd, scaler = _torch_forms()
    fused = C.adam_from_torch(opt_sd, scaler, n_slots=16)
    amp = fused["n2m_amp"]
    assert amp["steps"].shape == (17,) and amp["steps"].tolist()[:5] == [40.0, 40.0, 40.0, 17.0, 0.0] and float(amp["steps"][5:].abs().sum()) == 0
    assert amp["scale"] == 8192.0 and amp["growth_tracker"] == 731.0 and amp["growth"] == (2.0, 0.5, 2000.0)
    assert all("step" not in st for st in fused["state"].values())
    back, scaler_back, extra = C.adam_to_torch(fused)
    assert scaler_back == scaler and type(scaler_back["_growth_tracker"]) is int and type(scaler_back["growth_interval"]) is int
    assert extra["steps_all"] == 40.0
    assert back["param_groups"] == opt_sd["param_groups"]
    for i, st in opt_sd["state"].items():
        assert float(back["state"][i]["step"]) == float(st["step"])
        assert torch.equal(back["state"][i]["exp_avg"], st["exp_avg"]) and torch.equal(back["state"][i]["exp_avg_sq"], st["exp_avg_sq"])
    # the count of all steps travels in n2m["adam"] where the per-parameter counts do not say it (every tensor joined late)
    again = C.adam_from_torch(back, scaler_back, {"steps_all": 45.0, "amp": True})
    assert again["n2m_amp"]["steps"].tolist()[:4] == [45.0, 40.0, 40.0, 17.0]
    # a state that already is FusedAdamAMP's passes through
    assert C.adam_from_torch(fused) is fused
    # torch's own classes take the converted forms
    params = [torch.nn.Parameter(torch.zeros(st["exp_avg"].shape)) for st in opt_sd["state"].values()]
    adam = torch.optim.Adam([{"params": params[:2], "lr": 1.0}, {"params": params[2:], "lr": 1.0}], eps=1e-15)
    adam.load_state_dict(back)
    assert [float(adam.state[p]["step"]) for p in params] == [40.0, 40.0, 17.0, 0.0] and adam.param_groups[1]["initial_lr"] == 2e-3
    assert torch.equal(adam.state[params[2]]["exp_avg_sq"], opt_sd["state"][2]["exp_avg_sq"])
    with pytest.raises(ValueError, match=r"optimizer.state\[3\]"):
        C.adam_from_torch(opt_sd, scaler, n_slots=3)


def test_lambda_lr_resumes_with_the_same_rates():
    from nerf2mesh_amd.engine_adam import lr_lambda
    from nerf2mesh_amd.trainer import LambdaLR
    f = lambda it: lr_lambda(it, 3000)

    def make():
        p = [torch.nn.Parameter(torch.zeros(2)), torch.nn.Parameter(torch.zeros(3))]
        o = torch.optim.Adam([{"params": p[:1], "lr": 1e-2}, {"params": p[1:], "lr": 1e-3}])
        return o, LambdaLR(o, f)
    oa, sa = make()
    for _ in range(700):                                             # across the warm-up's end at 500
        sa.step()
    saved_opt, saved_sched = oa.state_dict(), sa.state_dict()
    assert saved_sched == {"last_epoch": 700} and [g["initial_lr"] for g in saved_opt["param_groups"]] == [1e-2, 1e-3]
    ob, sb = make()
    ob.load_state_dict(saved_opt)
    sb.load_state_dict(saved_sched)
    assert sb.get_last_lr() == sa.get_last_lr()
    for _ in range(50):
        sa.step()
        sb.step()
        assert sb.get_last_lr() == sa.get_last_lr()
    assert sa.get_last_lr() == [1e-2 * f(750), 1e-3 * f(750)]
