"""GPU: the normal-consistency / edge-length kernels (n2m_mesh_losses_forward / _backward / _backward_acc, csrc/meshloss.hip) against the float64
yardstick of tests/mesh_loss_case.py, and the two losses inside the stage-1 step (trainer.Stage1Trainer and engine_stage1.Stage1Engine).

Tolerances: tests/mesh_loss_case.py measures how far the plain float32 torch form is from the yardstick (value: absolute; gradient: over the
largest |gradient| of the mesh) and gives every float32 evaluation 8 x the largest distance -- VALUE_BOUND 1.04e-06 (measured 1.3e-07),
GRAD_BOUND 1.04e-04 (measured 1.3e-05)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mesh_loss_case as MC   # noqa: E402

pytestmark = pytest.mark.gpu


def _terms(v, f):
    import torch
    from nerf2mesh_amd.trainer import MeshEdgeTerms
    return MeshEdgeTerms(torch.from_numpy(f).cuda(), v.shape[0])


@pytest.mark.parametrize("name", list(MC.cases()))
def test_kernels_against_the_float64_yardstick_and_bitwise_repeatable(name):
    """Value and gradient (non-unit weights, non-unit upstream gradient) of the kernels on the same float32 vertices; a second run gives the same
    bits.  The grid cases have V = 441, E = 1240, P = 1160 -- no multiple of 64 or 256, several workgroups each way."""
    import torch
    v, f, settings = MC.cases()[name]
    t = _terms(v, f)
    for w in settings:
        runs = []
        for _ in range(2):
            x = torch.from_numpy(v).cuda().requires_grad_()
            val = t(x, *w)
            (val * MC.UPSTREAM).backward()
            runs.append((val.detach().clone(), x.grad.clone()))
        dv, dg = MC.distances(name, w, runs[0][0], runs[0][1])
        print(f"{name:18s} weights {w}: value {float(runs[0][0]):.6g}  |diff| {dv:.3g}   gradient diff / max {dg:.3g}")
        assert dv <= MC.VALUE_BOUND and dg <= MC.GRAD_BOUND, (name, w, dv, dg)
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_zero_area_face_on_the_device():
    """The pair with a collinear face: the value is within the bound of the yardstick's (1: the clamped cosine is 0) and the gradient, of order
    1e8 by the clamped expression, is finite -- the one case left out of the gradient comparison."""
    import torch
    v, f = MC.zero_area()
    t = _terms(v, f)
    x = torch.from_numpy(v).cuda().requires_grad_()
    val = t(x, 1.0, 0.0)
    val.backward()
    assert abs(float(val) - 1.0) <= MC.VALUE_BOUND
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 1e6


@pytest.mark.parametrize("name", ["book", "grid noise 0.01", "two cascades"])
def test_accumulating_backward_equals_base_plus_the_plain_backward(name):
    """n2m_mesh_losses_backward_acc == base + n2m_mesh_losses_backward's output, bit for bit."""
    import torch
    from nerf2mesh_amd import _lib as L
    v, f, _ = MC.cases()[name]
    t = _terms(v, f)
    x = torch.from_numpy(v).cuda()
    V, P, E, s = v.shape[0], t.n_pairs, t.n_edges, L.stream()
    w_n, w_e = t.weights(0.37, 2.5)
    seed = torch.tensor(1024.0, device="cuda")
    args = (L.ptr(x), L.ptr(t.pairs), L.ptr(t.pair_ptr), L.ptr(t.pair_ref), P, L.ptr(t.edges), L.ptr(t.edge_ptr), L.ptr(t.edge_ref), E, V, L.ptr(seed),
            w_n, w_e)
    d = torch.empty(V, 3, device="cuda")
    L.call("n2m_mesh_losses_backward", *args, L.ptr(d), s)
    base = torch.randn(V, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    acc = base.clone()
    L.call("n2m_mesh_losses_backward_acc", *args, L.ptr(acc), s)
    assert float(d.abs().max()) > 0 and torch.equal(acc, base + d)


def test_calls_without_terms_return_zero_and_write_nothing():
    """P = 0 and E = 0 (and V = 0): status 0, no launch, the output buffers keep their bytes; a mesh without pairs runs its edges alone; through
    autograd a loss without terms is 0 with a gradient of zeros."""
    import torch
    from nerf2mesh_amd import _lib as L
    v, f = MC.triangle()
    t = _terms(v, f)
    assert (t.n_pairs, t.n_edges) == (0, 3)
    x = torch.from_numpy(v).cuda()
    s, seed = L.stream(), torch.ones((), device="cuda")
    partial, d = torch.full((4,), -7.0, device="cuda"), torch.full((3, 3), -7.0, device="cuda")
    L.call("n2m_mesh_losses_forward", L.ptr(x), None, 0, None, 0, 1.0, 1.0, L.ptr(partial), s)
    for entry in ("n2m_mesh_losses_backward", "n2m_mesh_losses_backward_acc"):
        L.call(entry, L.ptr(x), None, None, None, 0, None, None, None, 0, 3, L.ptr(seed), 1.0, 1.0, L.ptr(d), s)
        L.call(entry, L.ptr(x), L.ptr(t.pairs), L.ptr(t.pair_ptr), L.ptr(t.pair_ref), 0, L.ptr(t.edges), L.ptr(t.edge_ptr), L.ptr(t.edge_ref), 3, 0,
               L.ptr(seed), 1.0, 1.0, L.ptr(d), s)
    assert bool((partial == -7.0).all()) and bool((d == -7.0).all())
    with pytest.raises(RuntimeError, match="P > 0 needs pairs"):
        L.call("n2m_mesh_losses_forward", L.ptr(x), None, 5, None, 0, 1.0, 1.0, L.ptr(partial), s)
    # no pair, three edges: one workgroup's sum is written, the rest of the buffer is not
    L.call("n2m_mesh_losses_forward", L.ptr(x), None, 0, L.ptr(t.edges), 3, 1.0, 1.0 / 3, L.ptr(partial), s)
    want = MC.yardstick("triangle")[(0.0, 1.0)][0]
    assert abs(float(partial[0]) - want) <= MC.VALUE_BOUND and bool((partial[1:] == -7.0).all())
    y = torch.from_numpy(v).cuda().requires_grad_()
    val = t(y, 1.0, 0.0)                                        # the normal loss of a mesh without pairs
    val.backward()
    assert float(val) == 0.0 and float(y.grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ inside the stage-1 step

LAM_NORMAL, LAM_EDGE = 1e-2, 0.1
HW = 64


def _trainer(lam_n, lam_e, fused_head=True):
    import torch
    from nerf2mesh_amd import synthetic as S
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    from nerf2mesh_amd.trainer import Stage1Trainer
    torch.manual_seed(0)
    opt = make_options(O=True, bound=1, dt_gamma=0, stage=1, fused_mlp=True, lambda_normal=lam_n, lambda_edgelen=lam_e)
    v, f = S.scene_mesh(2000)
    tr = Stage1Trainer(NeRFNetwork(opt), opt, S.make_cameras(4, seed=0), v, f, torch.device("cuda"), H=HW, W=HW)
    tr.fused_head = fused_head
    for _ in range(500):
        tr.scheduler.step()               # past the warm-up of the schedule: the step moves the parameters
    return tr


def _params(tr):
    m = tr.model
    return {"colour table": m.encoder_color.embeddings.detach().float().clone(), "offsets": m.vertices_offsets.detach().clone(),
            **{f"mlp{i}": p.detach().clone() for i, p in enumerate(list(m.color_net.parameters()) + list(m.specular_net.parameters()))}}


def _trainer_step(tr):
    scale = float(tr.optimizer.scale)
    loss = float(tr.train_step().detach())
    table = tr._amp["color"].get("grad_half")                  # (the fused head's path: the fp16 gradient the optimizer read)
    return dict(loss=loss, scale=scale, grad=tr.model.vertices_offsets.grad.clone(), table=None if table is None else table.float().clone(),
                params=_params(tr), covered=getattr(tr.model, "last_covered", 0))


def _engine_step(tr):
    from nerf2mesh_amd.engine_stage1 import Stage1Engine
    assert Stage1Engine.supported(tr)
    eng = Stage1Engine(tr)
    seen, step = {}, tr.optimizer.step

    def spy(flagged=()):
        seen["grad"], seen["table"] = tr.model.vertices_offsets.grad.clone(), eng.g2.float().clone()
        return step(flagged=flagged)
    tr.optimizer.step = spy
    scale = float(tr.optimizer.scale)
    loss = float(eng.train_step())
    tr.optimizer.step = step
    return dict(loss=loss, scale=scale, params=_params(tr), covered=tr.model.last_covered, engine=eng, **seen)


@pytest.fixture(scope="module")
def steps():
    """One step each, computed once: two autograd trainers with both weights 0, two with them on, the executor with them on; and the float64 value
    and gradient of the two terms on the step's vertices (the offsets start at 0, so these are the mesh's own vertices)."""
    import torch
    from nerf2mesh_amd import synthetic as S
    out = {"off": _trainer_step(_trainer(0, 0)), "off2": _trainer_step(_trainer(0, 0)),
           "on": _trainer_step(_trainer(LAM_NORMAL, LAM_EDGE)), "on2": _trainer_step(_trainer(LAM_NORMAL, LAM_EDGE)),
           "engine": _engine_step(_trainer(LAM_NORMAL, LAM_EDGE))}
    v, f = S.scene_mesh(2000)
    edges, pairs = MC.brute_topology(np.asarray(f))
    x = torch.as_tensor(v, dtype=torch.float32).double().requires_grad_()
    n, e = MC.defined_losses(x, edges, pairs)
    val = LAM_NORMAL * n + LAM_EDGE * e
    val.backward()
    out["terms"] = (float(val.detach()), x.grad.clone())
    return out


def _ulp(x):
    return float(np.spacing(np.float32(abs(x))))


@pytest.mark.parametrize("fused_head", [True, False])
def test_trainer_loss_gains_exactly_the_two_terms(steps, fused_head):
    """Stage1Trainer with lambda_normal = 1e-2, lambda_edgelen = 0.1 against the same step with both at 0 (same view, same background): the loss
    differs by lambda_normal * normal + lambda_edgelen * edge of the step's vertices -- to the kernels' VALUE_BOUND, the float32 roundings of
    the two losses and of the sum (one ulp of the loss each) and 10 x what two runs of the weights-off step differ by (the margin
    tests/test_stage1.py gives that distance).  Both branches of the step: the fused image head and the torch graph."""
    if fused_head:
        on, off, off2 = steps["on"]["loss"], steps["off"]["loss"], steps["off2"]["loss"]
    else:
        on, off, off2 = (_trainer_step(_trainer(*lam, False))["loss"] for lam in ((LAM_NORMAL, LAM_EDGE), (0, 0), (0, 0)))
    want = steps["terms"][0]
    tol = MC.VALUE_BOUND + 3 * _ulp(on) + 10 * abs(off - off2)
    print(f"loss with the terms {on:.8g}, without {off:.8g} (a second run {off2:.8g}), difference {on - off:.6g}, the two terms {want:.6g}, "
          f"allowed {tol:.3g}")
    assert want > 100 * tol                                             # the terms are far above what the comparison resolves
    assert abs((on - off) - want) <= tol


def _render_noise(a, b):
    return float((a["grad"] - b["grad"]).abs().max())


@pytest.mark.parametrize("who", ["on", "engine"])
def test_offset_gradient_is_rendering_plus_regularisers_plus_the_new_terms(steps, who):
    """The vertex offsets' gradient with the weights on = the gradient with both at 0 (rendering + Laplacian + offset penalty) + loss scale x the
    gradient of the two terms -- for the autograd trainer and for the executor.  Allowed: the kernels' GRAD_BOUND on the terms' part, the float32
    roundings of the sum (three adds: 3 ulp of the largest entry) and what two runs of the SAME weights-off step differ by (float atomics in the
    raster / antialias backward), times the margin tests/test_stage1.py gives that distance (10)."""
    got, off = steps[who], steps["off"]
    assert got["scale"] == off["scale"] and got["covered"] == off["covered"] > 0
    want = (got["scale"] * steps["terms"][1]).float().cuda()
    noise = _render_noise(steps["off"], steps["off2"])
    err = float(((got["grad"] - off["grad"]) - want).abs().max())
    tol = MC.GRAD_BOUND * float(want.abs().max()) + 3 * _ulp(float(got["grad"].abs().max())) + 10 * noise
    print(f"{who}: max |terms' gradient| {float(want.abs().max()):.4g}, max |gradient| {float(got['grad'].abs().max()):.4g}, error {err:.3g}, "
          f"two weights-off runs differ by {noise:.3g}, allowed {tol:.3g}")
    assert float(want.abs().max()) > 100 * tol                          # the terms' gradient is far above what the comparison resolves
    assert err <= tol


def test_executor_reproduces_the_trainer_with_the_terms_on(steps):
    """Stage1Engine against Stage1Trainer for one step with lambda_normal / lambda_edgelen on, by the criterion of
    tests/test_stage1.py::test_stage1_executor_reproduces_the_autograd_trainer: loss to 1e-5, first-step gradients to 1e-3 (2e-3 for the fp16
    colour-table gradient) of their maximum, parameters after the step within 10 x the distance between two runs of the autograd trainer + 2e-3."""
    a, a2, b = steps["on"], steps["on2"], steps["engine"]
    assert abs(a["loss"] - b["loss"]) <= 1e-5 * abs(a["loss"]), (a["loss"], b["loss"])
    for k, tol in (("grad", 1e-3), ("table", 2e-3)):
        d = float((a[k] - b[k]).abs().max()) / float(a[k].abs().max())
        print(f"first-step gradient, {k}: max |diff| / max = {d:.3g}")
        assert d <= tol, k
    assert a["covered"] == b["covered"] > 0
    rel = lambda x, y: float((x - y).norm() / x.norm().clamp_min(1e-30))
    for k in a["params"]:
        d_te, d_tt = rel(a["params"][k], b["params"][k]), rel(a["params"][k], a2["params"][k])
        print(f"{k:14s} trainer-vs-executor {d_te:.3g}   trainer-vs-trainer {d_tt:.3g}")
        assert d_te <= 10 * d_tt + 2e-3, k
    eng = b["engine"]
    assert eng.mesh_partial is not None and eng.mesh_partial.numel() == (eng.mesh.n_pairs + 255) // 256 + (eng.mesh.n_edges + 255) // 256


def test_weights_zero_leave_the_executor_step_as_it_was(monkeypatch):
    """Both weights 0 (the defaults): no topology, no buffer, no launch of the new kernels; the loss is the one reduction over the image head's
    and the regularisers' sums, and the offsets' gradient is what n2m_laplacian_backward_acc makes of the rendering gradient -- bit for bit."""
    import torch
    from nerf2mesh_amd import _lib as L
    from nerf2mesh_amd.engine_stage1 import Stage1Engine
    tr = _trainer(0, 0)
    eng = Stage1Engine(tr)
    assert tr.mesh_terms is None and eng.mesh is None and eng.mesh_partial is None
    V, N = tr.model.vertices.shape[0], HW * HW
    assert eng.partials.numel() == (N + 255) // 256 + (V + 255) // 256
    assert eng.reg_partial.data_ptr() + eng.reg_partial.numel() * 4 == eng.partials.data_ptr() + eng.partials.numel() * 4
    calls, kept, real = [], {}, L.call

    def spy(name, *args):
        calls.append(name)
        if name == "n2m_laplacian_backward_acc":
            # d_verts here: the rendering gradient, straight from n2m_to_clip_backward; the offsets as they are before the optimizer moves them
            kept["args"], kept["base"], kept["off"] = args, eng.d_verts.clone(), tr.model.vertices_offsets.detach().clone()
        return real(name, *args)
    monkeypatch.setattr(L, "call", spy)
    loss = eng.train_step()
    monkeypatch.undo()
    assert not [c for c in calls if c.startswith("n2m_mesh_losses")]
    i = calls.index("n2m_to_clip_backward")
    assert calls[i:i + 3] == ["n2m_to_clip_backward", "n2m_laplacian_forward", "n2m_laplacian_backward_acc"]
    assert torch.equal(loss, eng.partials.sum() / float(N))
    redo, flag = kept["base"].clone(), torch.zeros(1, device="cuda")
    args = list(kept["args"])
    args[7], args[11], args[12] = L.ptr(kept["off"]), L.ptr(redo), L.ptr(flag)
    L.call("n2m_laplacian_backward_acc", *args)
    assert torch.equal(redo, eng.d_verts) and tr.model.vertices_offsets.grad is eng.d_verts
