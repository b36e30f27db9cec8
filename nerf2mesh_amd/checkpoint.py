"""Checkpoints of both stages: the file, the folder, and the rule that resumes a run.

The layout is the reference's (nerf/utils.py:1345-1473): WORKSPACE/checkpoints/{name}_stage{S}_ep{E:04d}.pth, at most `max_keep` of them, the
newest one is "latest"; {name}_stage{S}.pth holds the best evaluated model with the averaged weights.  A file carries the reference's keys --
epoch, global_step, stats, stage, mean_density, model and, with full=True, optimizer, lr_scheduler, scaler, ema -- written in the forms an
unchanged reference Trainer reads and writes (torch.optim.Adam's and torch.amp.GradScaler's state), and everything of this project under one
more key, "n2m": the format version, the options as plain values, the step counts of optim.FusedAdamAMP, and what each driver keeps outside
those objects (its counters, the batch pipeline's generator in front of the next batch, the depth schedule's position, the device generator,
the stage-1 mesh).  Tensors and plain Python values only: torch.load(..., weights_only=True) reads every file written here.

What a driver saves is decided by the driver: engine.Stage0Engine, trainer.Stage0Trainer, trainer.Stage1Trainer and engine_stage1.Stage1Engine
each have state_dict() / load_state_dict(); this module moves that state to and from disk and converts the optimizer's two forms."""
import glob
import os
import re

import torch

FORMAT = 1
ADAM_GROUP_DEFAULTS = dict(weight_decay=0, amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                           decoupled_weight_decay=False)
SCALER_DEFAULTS = dict(scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, _growth_tracker=0)


def new_stats():
    """The reference Trainer's `stats` (nerf/utils.py:530-536)."""
    return {"loss": [], "valid_loss": [], "results": [], "checkpoints": [], "best_result": None}


# ---------------------------------------------------------------------------------------------------------- optimizer forms
def adam_to_torch(fused_sd):
    """optim.FusedAdamAMP.state_dict() -> (torch.optim.Adam's state_dict, torch.amp.GradScaler's state_dict, what neither holds).
    Parameter i of the optimizer's order is slot 1 + i of `steps`; its count becomes that parameter's `step`."""
    amp = fused_sd["n2m_amp"]
    steps = amp["steps"].detach().float().cpu().reshape(-1)
    state = {}
    for i, st in fused_sd["state"].items():
        state[i] = {"step": steps[1 + int(i)].clone(), "exp_avg": st["exp_avg"], "exp_avg_sq": st["exp_avg_sq"]}
    groups = []
    for g in fused_sd["param_groups"]:
        g = dict(g)
        for k, v in ADAM_GROUP_DEFAULTS.items():
            g.setdefault(k, v)
        g["betas"] = tuple(float(b) for b in g["betas"])
        groups.append(g)
    gf, bf, gi = amp.get("growth", (2.0, 0.5, 2000.0))
    scaler = {"scale": float(amp["scale"]), "growth_factor": float(gf), "backoff_factor": float(bf), "growth_interval": int(gi),
              "_growth_tracker": int(amp["growth_tracker"])}
    return {"state": state, "param_groups": groups}, scaler, {"steps_all": float(steps[0]), "amp": bool(amp.get("amp", True))}


def adam_from_torch(opt_sd, scaler_sd=None, extra=None, n_slots=16):
    """The inverse: torch.optim.Adam's state_dict [+ GradScaler's] -> what optim.FusedAdamAMP.load_state_dict takes.  A state that already
    carries "n2m_amp" (a file of this project from before the reference forms) passes through.  Without `extra` (a file the reference
    wrote) the count of all steps is the largest per-parameter count."""
    if "n2m_amp" in opt_sd:
        return opt_sd
    scaler = dict(SCALER_DEFAULTS)
    scaler.update(scaler_sd or {})
    steps = torch.zeros(1 + n_slots, dtype=torch.float32)
    state = {}
    for i, st in opt_sd["state"].items():
        if int(i) >= n_slots:
            raise ValueError(f"optimizer.state[{i}]: optim.FusedAdamAMP holds {n_slots} tensors")
        steps[1 + int(i)] = float(st["step"]) if "step" in st else 0.0
        state[i] = {k: v for k, v in st.items() if k != "step"}
    steps[0] = float(extra["steps_all"]) if extra is not None and "steps_all" in extra else float(steps[1:].max())
    amp = {"steps": steps, "scale": float(scaler["scale"]), "growth_tracker": float(scaler["_growth_tracker"]),
           "amp": bool(extra["amp"]) if extra is not None and "amp" in extra else True,
           "growth": (float(scaler["growth_factor"]), float(scaler["backoff_factor"]), float(scaler["growth_interval"]))}
    return {"state": state, "param_groups": [dict(g) for g in opt_sd["param_groups"]], "n2m_amp": amp}


def optimizer_state(driver):
    """(optimizer, scaler, n2m["adam"]) entries of a driver's state: FusedAdamAMP in the reference's two forms, torch's own pair as it is."""
    o = driver.optimizer
    if hasattr(o, "found_inf"):          # optim.FusedAdamAMP
        return adam_to_torch(o.state_dict())
    scaler = getattr(driver, "scaler", None)
    return o.state_dict(), (scaler.state_dict() if scaler is not None else {}), None


def load_optimizer_state(driver, sd):
    o = driver.optimizer
    if "optimizer" not in sd:
        return
    if hasattr(o, "found_inf"):
        o.load_state_dict(adam_from_torch(sd["optimizer"], sd.get("scaler"), sd.get("n2m", {}).get("adam"), n_slots=o.steps.numel() - 1))
        return
    opt_sd = sd["optimizer"]
    if "n2m_amp" in opt_sd:
        opt_sd, scaler_sd, _ = adam_to_torch(opt_sd)
    else:
        scaler_sd = sd.get("scaler")
    o.load_state_dict(opt_sd)
    scaler = getattr(driver, "scaler", None)
    if scaler is not None and scaler.is_enabled() and scaler_sd:
        scaler.load_state_dict(scaler_sd)


# ------------------------------------------------------------------------------------------------ what the stage-0 drivers share
def plain_options(opt):
    """The options as a dict of plain values (what a file may hold)."""
    out = {}
    for k, v in sorted(vars(opt).items()):
        if isinstance(v, (bool, int, float, str)) or v is None:
            out[k] = v
        elif isinstance(v, (list, tuple)) and all(isinstance(x, (bool, int, float, str)) for x in v):
            out[k] = list(v)
    return out


def _device_rng(device):
    device = torch.device(device)
    return torch.cuda.get_rng_state(device) if device.type == "cuda" else torch.get_rng_state()


def _set_device_rng(device, state):
    device = torch.device(device)
    if device.type == "cuda":
        torch.cuda.set_rng_state(state.cpu(), device)
    else:
        torch.set_rng_state(state.cpu())


def _load_model(model, state, model_only):
    """A size mismatch raises and names the key (torch's message); so does, outside model_only, a key one side lacks."""
    missing, unexpected = model.load_state_dict(state, strict=False)
    if not model_only and (missing or unexpected):
        raise KeyError(f"model: the checkpoint lacks {list(missing)} and holds {list(unexpected)} this model does not have")


def stage0_state(d):
    """The part of a stage-0 driver's state both drivers hold alike (engine.Stage0Engine, trainer.Stage0Trainer): a file of either loads
    into the other."""
    model = d.model
    optimizer, scaler, adam = optimizer_state(d)
    sd = {"epoch": d.global_step // d.epoch_len, "global_step": int(d.global_step), "stats": getattr(d, "stats", None) or new_stats(),
          "stage": int(d.opt.stage), "mean_density": float(model.mean_density), "model": model.state_dict(), "optimizer": optimizer,
          "lr_scheduler": {"last_epoch": int(d.global_step)}, "scaler": scaler}
    if d.ema is not None:
        sd["ema"] = d.ema.state_dict()
    sd["n2m"] = {"options": plain_options(d.opt), "adam": adam, "samples_seen": int(d.samples_seen), "rays_seen": int(d.rays_seen),
                 "loss_sum": d.loss_acc.detach().reshape(1).clone(), "iter_density": int(model.iter_density), "max_level": int(model.max_level),
                 "device_rng": _device_rng(d.device)}
    if getattr(d, "refiner", None) is not None:          # optimize_poses: the corrections, their Adam, the stored poses' checksum
        sd["n2m"]["pose_refine"] = d.refiner.state_dict()
    return sd


def load_stage0_state(d, sd, model_only=False):
    model = d.model
    if "model" not in sd:                       # a bare model state_dict, as the reference accepts one (nerf/utils.py:1423-1426)
        _load_model(model, sd, True)
        return
    refiner = getattr(d, "refiner", None)
    if not model_only and (refiner is None) != (sd.get("n2m", {}).get("pose_refine") is None):
        raise ValueError("pose_refine: the checkpoint and this driver disagree on optimize_poses -- a run with refined poses continues only "
                         "as one (its field was trained on them); model_only=True takes the model alone")
    _load_model(model, sd["model"], model_only)
    if d.ema is not None and sd.get("ema") is not None:
        d.ema.load_state_dict(sd["ema"])
    if "mean_density" in sd:
        model.mean_density = float(sd["mean_density"])
    if model_only:
        return
    n2m = sd.get("n2m", {})
    d.global_step = int(sd["global_step"])
    d.stats = sd.get("stats") or new_stats()
    load_optimizer_state(d, sd)
    if getattr(d, "scheduler", None) is not None:
        d.scheduler.load_state_dict(sd.get("lr_scheduler") or {"last_epoch": d.global_step})
    d.samples_seen, d.rays_seen = int(n2m.get("samples_seen", 0)), int(n2m.get("rays_seen", 0))
    if "loss_sum" in n2m:
        d._loss_sum.copy_(n2m["loss_sum"].to(d._loss_sum.device).reshape(d._loss_sum.shape))
    model.iter_density = int(n2m.get("iter_density", model.iter_density))
    model.max_level = int(n2m.get("max_level", model.max_level))
    if "device_rng" in n2m:
        _set_device_rng(d.device, n2m["device_rng"])
    if refiner is not None:
        refiner.load_state_dict(n2m["pose_refine"])      # (refreshes the pose table the driver reads)


def batch_state(sd):
    """n2m["batches"] of a stage-0 state; a file the reference wrote has none: the run goes on with this driver's generator as it is."""
    b = sd.get("n2m", {}).get("batches")
    if b is None:
        raise KeyError("n2m.batches: the checkpoint holds no batch-pipeline state (written by the reference?); load it with model_only=True")
    return b


# --------------------------------------------------------------------------------------------------------------- the folder
def _stage(driver):
    return int(driver.opt.stage)


def _world(driver):
    return int(getattr(driver, "world", 1) or 1)


def checkpoint_dir(workspace):
    return os.path.join(workspace, "checkpoints")


def _candidates(workspace, stage):
    """sorted(glob('*_stage{S}*.pth')) of the reference, without the best-model files ({name}_stage{S}.pth)."""
    files = sorted(glob.glob(os.path.join(glob.escape(checkpoint_dir(workspace)), f"*_stage{int(stage)}*.pth")))
    return [f for f in files if not re.search(rf"_stage{int(stage)}\.pth$", os.path.basename(f))]


def latest_checkpoint(workspace, stage):
    """Path of the newest rotating checkpoint of `stage` in WORKSPACE/checkpoints, or None."""
    files = _candidates(workspace, stage)
    return files[-1] if files else None


def best_checkpoint(workspace, stage, name="ngp"):
    path = os.path.join(checkpoint_dir(workspace), f"{name}_stage{int(stage)}.pth")
    return path if os.path.exists(path) else None


def _write(state, path):
    """Temporary file in the same directory (a name no glob for *.pth matches), then os.replace: a save that dies leaves what was there."""
    tmp = f"{path}.tmp{os.getpid()}"
    try:
        torch.save(state, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def save_checkpoint(driver, path_or_workspace, full=True, best=False, name=None, max_keep=2):
    """Writes the driver's state.  path_or_workspace: a workspace directory -- the file goes to its checkpoints/ folder under the
    reference's name and the folder is rotated -- or a path that ends in .pth, written as it is.  best=True: the model with the averaged
    weights, and only when the newest entry of stats["results"] beats stats["best_result"] (lower is better).  Returns the path written,
    or None when a best save had nothing to write."""
    if _world(driver) > 1:
        raise NotImplementedError("checkpoints of a multi-rank run: every rank would write its own shard (not implemented: train on one rank, or gather first)")
    name = name or "ngp"
    stats = getattr(driver, "stats", None)
    if stats is None:
        stats = driver.stats = new_stats()
    stage = _stage(driver)
    explicit = str(path_or_workspace).endswith(".pth")
    folder = os.path.dirname(os.path.abspath(path_or_workspace)) if explicit else checkpoint_dir(path_or_workspace)
    os.makedirs(folder, exist_ok=True)
    if best:
        if not stats["results"]:
            return None
        if stats["best_result"] is not None and not stats["results"][-1] < stats["best_result"]:
            return None
    before = (list(stats["checkpoints"]), stats["best_result"])
    if best:
        stats["best_result"] = stats["results"][-1]
    removed = []
    if not best and not explicit:
        state_epoch = _epoch(driver)
        file = f"{name}_stage{stage}_ep{state_epoch:04d}.pth"
        if file in stats["checkpoints"]:
            stats["checkpoints"].remove(file)
        stats["checkpoints"].append(file)
        while len(stats["checkpoints"]) > max_keep:
            removed.append(stats["checkpoints"].pop(0))
        path = os.path.join(folder, file)
    elif explicit:
        path = str(path_or_workspace)
    else:
        path = os.path.join(folder, f"{name}_stage{stage}.pth")
    ema = getattr(driver, "ema", None)
    if best and ema is not None:
        if hasattr(driver, "sync_parameters"):
            driver.sync_parameters()
        with ema.average_parameters():          # store(); copy_to() ... restore(), nerf/utils.py:1389-1401
            state = _file_state(driver, full)
            state["model"] = {k: v.detach().clone() for k, v in state["model"].items()}
    else:
        state = _file_state(driver, full)
    try:
        _write(state, path)
    except BaseException:
        stats["checkpoints"][:], stats["best_result"] = before      # the folder is as it was: so is the list of what it holds
        raise
    for old in removed:
        old = os.path.join(folder, old)
        if os.path.exists(old):
            os.remove(old)
    return path


def _epoch(driver):
    tr = getattr(driver, "tr", driver)
    per = getattr(tr, "epoch_len", None) or max(1, len(getattr(tr, "views", [0])))
    return int(tr.global_step) // int(per)


def _file_state(driver, full):
    state = dict(driver.state_dict())
    state["n2m"] = dict(state.get("n2m", {}), n2m_format=FORMAT)
    if not full:
        for k in ("optimizer", "lr_scheduler", "scaler", "ema"):
            state.pop(k, None)
    return state


def read_checkpoint(path, device="cpu"):
    """The file's state; a newer format raises."""
    state = torch.load(path, map_location=device, weights_only=True)
    version = state.get("n2m", {}).get("n2m_format", 0) if isinstance(state, dict) else 0
    if int(version) > FORMAT:
        raise ValueError(f"{path}: checkpoint format {int(version)} is newer than this package reads ({FORMAT})")
    return state


def load_checkpoint(driver, checkpoint=None, model_only=False):
    """Loads `checkpoint` (a path; None: the latest one of the driver's stage in opt.workspace) into the driver.  model_only: the model, the
    averaged weights and mean_density alone -- how stage 1 starts from a stage-0 file.  Returns the path, or None when there was no file."""
    if _world(driver) > 1:
        raise NotImplementedError("loading a checkpoint into a multi-rank run is not implemented")
    if checkpoint is None:
        checkpoint = latest_checkpoint(driver.opt.workspace, _stage(driver))
        if checkpoint is None:
            return None
    state = read_checkpoint(checkpoint, getattr(driver, "device", "cpu"))
    driver.load_state_dict(state, model_only=model_only)
    return checkpoint


def restore_or_init(driver, workspace, ckpt="latest", name="ngp"):
    """The rule of the reference's Trainer.__init__ (nerf/utils.py:573-600) in one place.  ckpt: "scratch" (load nothing), "latest" (the
    newest file of the driver's stage; none: a stage-1 driver starts from the newest stage-0 file with model_only, a stage-0 driver from
    scratch), "best" (the best model if there is one, else latest), or a path.  Returns (path loaded or None, "full" | "model_only" | None)."""
    stage = _stage(driver)
    if ckpt == "scratch":
        path, mode = None, None
    elif ckpt in ("latest", "best"):
        path = (best_checkpoint(workspace, stage, name) if ckpt == "best" else None) or latest_checkpoint(workspace, stage)
        mode = "full" if path is not None else None
        if path is not None and ckpt == "best" and path == best_checkpoint(workspace, stage, name):
            mode = "model_only"                  # the reference loads the best file for evaluation; it holds the averaged weights
    else:
        # a path: a file of another stage (a stage-0 file handed to stage 1) gives the model alone
        state = read_checkpoint(ckpt, getattr(driver, "device", "cpu"))
        mode = "full" if int(state.get("stage", stage)) == stage else "model_only"
        driver.load_state_dict(state, model_only=mode == "model_only")
        return ckpt, mode
    if path is None and stage > 0 and ckpt != "scratch":
        path = latest_checkpoint(workspace, 0)
        mode = "model_only" if path is not None else None
    if path is not None:
        load_checkpoint(driver, path, model_only=mode == "model_only")
    return path, mode


def stage1_mesh(workspace, ckpt="latest"):
    """(vertices, triangles, v_cumsum, f_cumsum) held by the stage-1 checkpoint restore_or_init() would load in full -- what a front end
    builds its Stage1Trainer on instead of extracting the stage-0 mesh again -- or None when there is no such file."""
    if ckpt == "scratch":
        return None
    path = latest_checkpoint(workspace, 1) if ckpt in ("latest", "best") else ckpt
    if path is None:
        return None
    state = read_checkpoint(path)
    mesh = state.get("n2m", {}).get("mesh") if int(state.get("stage", 0)) == 1 else None
    return None if mesh is None else (mesh["vertices"], mesh["triangles"], mesh["v_cumsum"], mesh["f_cumsum"])
