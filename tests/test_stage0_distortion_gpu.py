"""GPU: the opt-in distortion term (options.lambda_distort / distort_space) of trainer.Stage0Trainer on a synthetic capture of
4 views at 48 x 48, num_rays 1024, the fused field.

Step 1 of a trainer with lambda_distort = 0.01 against step 1 of identically seeded trainers without the term: the loss gains
0.01 * last_distortion, last_distortion is the float64 model's value on the step's own weights / ts / rays / nears / fars
(tests/distortion_ref.py, under the kernel's bound of tests/test_distortion_gpu.py), and the density-table gradient equals the one a step
with the torch statement of the term produces."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import distortion_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu

LAM, HW, RAYS = 0.01, 48, 1024


def _capture():
    from nerf2mesh_amd import synthetic
    from nerf2mesh_amd.capture import Capture
    f = synthetic.LEGO_FOCAL * HW / synthetic.LEGO_HW                      # the whole scene in the frame
    return Capture.synthetic(synthetic.make_cameras(4, seed=0), H=HW, W=HW, intrinsics=(f, f, HW / 2, HW / 2), alpha=True, device="cuda")


def _trainer(cap, torch_term=False, **over):
    import torch
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    from nerf2mesh_amd.trainer import Stage0Trainer
    torch.manual_seed(0)
    opt = make_options(O=True, bound=1, dt_gamma=0, iters=30000, fused_mlp=True, num_rays=RAYS, **over)
    tr = Stage0Trainer(NeRFNetwork(opt), opt, None, torch.device("cuda", 0), seed=0, capture=cap)
    if torch_term:                                                         # the torch statement of the term, on the device, in the kernels' place
        from nerf2mesh_amd.losses import distortion_loss_torch
        tr.distortion_fn = lambda w, ts, rays, nears, fars, space, rays_tile_samples: distortion_loss_torch(w, ts, rays, nears, fars, space)
    tr.mark_untrained()
    return tr


def _step(tr):
    """One step: the loss, the term, and the density-table gradient the optimizer was handed (it carries the loss scale)."""
    seen, model = {}, tr.model
    step = tr.optimizer.step

    def spy_step(flagged=()):
        seen["density"] = model.encoder.embeddings.grad.detach().float().clone()
        return step(flagged=flagged)
    tr.optimizer.step = spy_step
    seen["scale"] = float(tr.optimizer.scale)
    seen["loss"] = float(tr.train_step().detach())
    tr.optimizer.step = step
    seen["term"] = None if tr.last_distortion is None else float(tr.last_distortion)
    seen["inputs"] = tr.last_distortion_inputs
    return seen


def _params(tr):
    return [p.detach().clone() for p in tr.model.parameters()]


@pytest.fixture(scope="module")
def runs():
    cap = _capture()
    on = _trainer(cap, lambda_distort=LAM)
    assert on.lambda_distort == LAM and on.distort_space == "linear" and on.fused_loss is True
    first = _step(on)
    later = [float(on.train_step().detach()) for _ in range(2)]
    return {"cap": cap, "on": first, "later": later, "later_term": float(on.last_distortion), "off": _step(_trainer(cap)),
            "off2": _step(_trainer(cap)), "torch": _step(_trainer(cap, torch_term=True, lambda_distort=LAM))}


def test_the_executor_steps_aside():
    from nerf2mesh_amd.engine import Stage0Engine
    cap = _capture()
    off, on = _trainer(cap), _trainer(cap, lambda_distort=LAM)
    assert off.opt.lambda_distort == 0 and off.lambda_distort == 0 and off.last_distortion is None
    assert Stage0Engine.supported(off.model, off.opt, capture=cap)
    assert not Stage0Engine.supported(on.model, on.opt, capture=cap)


def test_three_steps_are_finite_and_the_term_is_positive(runs):
    import math
    on = runs["on"]
    assert all(math.isfinite(v) for v in [on["loss"]] + runs["later"])
    assert on["term"] is not None and on["term"] > 0 and runs["later_term"] > 0
    assert runs["off"]["term"] is None and runs["off"]["inputs"] is None
    weights, ts, rays, nears, fars = on["inputs"]
    M = weights.shape[0]
    assert not weights.requires_grad and ts.shape == (M, 2) and rays.shape == (RAYS, 2) and nears.shape == fars.shape == (RAYS,)
    assert int((rays[:, 1] > 0).sum()) >= RAYS // 2


def test_last_distortion_is_the_float64_model_on_the_steps_own_tensors(runs):
    """Under the kernel's bound: 4 x the fp32 yardstick's per-ray loss error, plus what the fp32 mean over 1024 rays adds (a tree sum of
    ten levels and one division of values <= 4/3)."""
    on = runs["on"]
    ref_loss, ref_mean, _ = R.model_f64(*on["inputs"], space="linear")
    tol = 4.0 * R.yardstick()["loss"] + 11 * 2.0 ** -24 * 4 / 3
    print(f"last_distortion {on['term']:.8g}, float64 model {float(ref_mean):.8g}, error {abs(on['term'] - float(ref_mean)):.3g}, allowed {tol:.3g}")
    assert float(ref_mean) > 0 and abs(on["term"] - float(ref_mean)) <= tol


def test_loss_gains_lambda_times_the_term(runs):
    """loss(lambda_distort = 0.01) = loss(0) of the same state + 0.01 * last_distortion to the fp32 rounding of one addition (an ulp of the
    sum covers it together with the product's own rounding), plus the distance two runs without the term show."""
    on, off, off2 = runs["on"], runs["off"], runs["off2"]
    assert on["scale"] == off["scale"]
    want = LAM * on["term"]
    tol = 2.0 ** -23 * abs(on["loss"]) + abs(off["loss"] - off2["loss"])
    print(f"loss with the term {on['loss']:.9g}, without {off['loss']:.9g} (a second run {off2['loss']:.9g}); term {on['term']:.8g}, "
          f"lambda * term {want:.6g}, difference {on['loss'] - off['loss']:.6g}, allowed {tol:.3g}")
    assert want > 100 * tol                                               # the term is far above what the comparison resolves
    assert abs((on["loss"] - off["loss"]) - want) <= tol


def test_the_gradient_reaches_the_density_table(runs):
    """One step with the kernels against one step from the same state and seeds with the torch statement of the term (float64 inside) in
    their place: both hand grad_weights to the same compositing backward, which is linear in it, so the density-table gradients differ by
    the kernels' gradient error carried through -- held to 4 x the fp32 yardstick's gradient error, as max |a - b| / max |b|."""
    import torch
    on, ref, off = runs["on"], runs["torch"], runs["off"]
    assert on["scale"] == ref["scale"] == off["scale"]
    a, b = on["density"], ref["density"]
    assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
    err = float((a - b).abs().max()) / float(b.abs().max())
    moved = float((a - off["density"]).abs().max()) / float(b.abs().max())
    noise = float((off["density"] - runs["off2"]["density"]).abs().max()) / float(b.abs().max())
    bound = 4.0 * R.yardstick()["grad"]
    print(f"density-table gradient: kernels vs torch statement {err:.3g} (bound {bound:.3g}); the term moves it by {moved:.3g}; "
          f"two runs without the term differ by {noise:.3g}")
    assert moved > 0                                                       # the term's gradient is there at all
    assert err <= bound


def test_disparity_space_runs(runs):
    import math
    tr = _trainer(runs["cap"], lambda_distort=LAM, distort_space="disparity")
    loss = float(tr.train_step().detach())
    assert math.isfinite(loss) and tr.distort_space == "disparity" and float(tr.last_distortion) > 0
    assert float(tr.last_distortion) != runs["on"]["term"]                 # the same batch in the other coordinate


def test_one_sdf_step_runs(runs):
    """SDF mode composites in alpha mode; the weights are weights either way."""
    import math
    tr = _trainer(runs["cap"], lambda_distort=LAM, sdf=True)
    loss = float(tr.train_step().detach())
    assert math.isfinite(loss) and float(tr.last_distortion) > 0


def test_one_patch_batch_runs(runs):
    import math
    tr = _trainer(runs["cap"], lambda_distort=LAM, patch_size=16)
    loss = float(tr.train_step().detach())
    assert math.isfinite(loss) and tr.last_patches[0].shape == (4, 16, 16, 3) and float(tr.last_distortion) > 0
    assert tr.last_distortion_inputs[2].shape == (RAYS, 2)


def test_a_resumed_run_continues(runs):
    """The term has no state of its own: the options travel with the driver, the file brings the rest."""
    import math
    a = _trainer(runs["cap"], lambda_distort=LAM)
    a.train_step()
    sd = a.state_dict()
    b = _trainer(runs["cap"], lambda_distort=LAM)
    b.load_state_dict(sd)
    assert b.global_step == 1
    loss = float(b.train_step().detach())
    assert math.isfinite(loss) and b.global_step == 2 and float(b.last_distortion) > 0


def test_two_runs_from_one_seed_end_in_identical_bits(runs):
    """The density recipe of this file (not SDF), three steps with the term on."""
    import torch
    ends = []
    for _ in range(2):
        tr = _trainer(runs["cap"], lambda_distort=LAM)
        for _ in range(3):
            tr.train_step()
        ends.append(_params(tr))
    for p, q in zip(*ends):
        assert torch.equal(p, q)
