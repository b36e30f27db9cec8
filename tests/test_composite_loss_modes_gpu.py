"""n2m_composite_loss_train in every mode and at its edges: the alpha-mode instantiation bit for bit against the four-kernel chain, every mode per ray
against the float64 model of tests/composite_loss_ref.py, stops placed on lane 0 / lane 63 / the first lane of a later chunk / a ray's last
sample, a ray cut off by M, vanishing loss weights, and the loss reduction over more than 1024 workgroups (ticketed and ticketless).

Yardstick of the float comparisons: E_ref(mode), the per-ray normalised error of the CPU oracle's serial fp32 chain against the same model,
recomputed here on the same inputs (composite_loss_ref.oracle_chain / ray_errors).  The fused kernel sums in another order (wave scans, the
ray totals as per-lane sums) and may show 4 x E_ref, the margin tests/test_depth_loss_gpu.py gives a different summation order; the loss
value 4 x max(the chain's error, 2^-24).  Measured values: DESIGN 4.24."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import composite_loss_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu

POISON = -7.0
PAD = 64                                         # gradient buffers hold M + PAD samples: nothing may be written at or behind M
HALF_ULP = 2.0 ** -24


_DEVICE = {}


def _dev(case):
    """The case's arrays on the GPU, uploaded once per case."""
    d = _DEVICE.get(id(case))
    if d is None:
        d = _DEVICE[id(case)] = {k: torch.from_numpy(v).cuda() for k, v in case.items() if isinstance(v, np.ndarray)}
    return d


def _fused(case, mode, lam_rgb=R.LAM_RGB, lam_mask=R.LAM_MASK, bg="tensor", outputs=True, ticket=True):
    from nerf2mesh_amd import _lib as L
    d, M, N, p = _dev(case), case["M"], case["N"], L.ptr
    full = lambda shape, v, dt=torch.float32: torch.full(shape, v, dtype=dt, device="cuda")
    B = (N + 15) // 16
    gs, gr = full((M + PAD,), POISON), full((M + PAD, 3), POISON)
    ws, im = (full((N,), POISON), full((N, 3), POISON)) if outputs else (None, None)
    depth = full((N,), POISON) if mode == "depth" else None
    live, block_live = full((N,), -7, torch.int32), full((B,), -7, torch.int32)
    partial = full((B,), POISON)
    tk = full((1,), 0, torch.int32) if ticket else None
    lv, lsum = (full((1,), POISON), full((1,), 2.0)) if ticket else (None, None)
    scale = full((1,), R.SCALE)
    head = L.CompositeLoss(sigmas=p(d["sig"]), rgbs=p(d["rgb"]), ts=p(d["ts"]), rays=p(d["rays"]), M=M, N=N, T_thresh=R.T_THRESH, gt_rgba=p(d["gt"]),
                           bg=p(d["bg"]) if bg == "tensor" else None, bg_scalar=0.0 if bg == "tensor" else float(bg), lambda_rgb=lam_rgb,
                           lambda_mask=lam_mask, grad_loss=p(scale), weights_sum=p(ws), image=p(im), grad_sigmas=p(gs), grad_rgbs=p(gr),
                           partial=p(partial), ticket=p(tk), loss=p(lv), loss_sum=p(lsum), live=p(live), block_live=p(block_live))
    if mode == "alpha":
        head.alpha_mode = 1
    elif mode == "entropy":
        head.lambda_entropy = R.LAM_ENT
    elif mode == "depth":
        head.depth, head.gt_depth, head.depth_weight, head.lambda_depth = p(depth), p(d["gtd"]), p(d["dw"]), R.LAM_DEPTH
    L.call("n2m_composite_loss_train", ctypes.addressof(head), L.stream())
    torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.cpu().numpy()
    out = dict(gs=cpu(gs), gr=cpu(gr), ws=cpu(ws), image=cpu(im), depth=cpu(depth), live=cpu(live), block_live=cpu(block_live), partial=cpu(partial))
    if ticket:
        assert int(tk) == 0                       # left zero
        out["loss"], out["loss_sum"] = lv.item(), lsum.item()
    return out


_RUNS = {}


def _run(mode):
    """The default call of a mode on its edge case, made once."""
    if mode not in _RUNS:
        _RUNS[mode] = _fused(R.edge_case(mode), mode)
    return _RUNS[mode]


def _written(case, got):
    """Every sample in [0, M) was written, nothing at or behind M."""
    M = case["M"]
    assert not (got["gs"][:M] == POISON).any() and not (got["gr"][:M] == POISON).any()
    assert (got["gs"][M:] == POISON).all() and (got["gr"][M:] == POISON).all()


def _against_model(case, mode, oracle, got, **kw):
    """The per-ray bound, the loss bound, the ray outputs and the stop positions of one call against the model; returns the figures."""
    ref = case["ref"] if not kw else R.model(case, mode, **kw)
    chain = R.oracle_chain(case, mode, oracle, **kw)
    M = case["M"]
    E_gs, E_gr = R.ray_errors(case, ref, chain["gs"], chain["gr"])
    e_gs, e_gr = R.ray_errors(case, ref, got["gs"][:M], got["gr"][:M])
    l_chain, l_fused = R.loss_error(chain["loss"], ref), R.loss_error(got["loss"], ref)
    print(f"{mode} {kw or ''}: grad_sigmas kernel {e_gs:.3e} / yardstick {E_gs:.3e}, grad_rgbs kernel {e_gr:.3e} / yardstick {E_gr:.3e}, "
          f"loss kernel {l_fused:.3e} / yardstick {l_chain:.3e}")
    assert e_gs <= 4 * E_gs and e_gr <= 4 * E_gr, (mode, kw, e_gs, E_gs, e_gr, E_gr)
    assert l_fused <= 4 * max(l_chain, HALF_ULP), (mode, kw, l_fused, l_chain)
    tol = dict(rtol=2e-5, atol=2e-6)             # the bar of test_composite_train
    np.testing.assert_allclose(got["ws"], ref["ws"], **tol)
    np.testing.assert_allclose(got["image"], ref["image"], **tol)
    if mode == "depth":
        np.testing.assert_allclose(got["depth"], ref["depth"], **tol)
    assert np.array_equal(got["live"], ref["live"])
    assert np.array_equal(got["block_live"], np.add.reduceat(ref["live"], np.arange(0, case["N"], 16)))
    _written(case, got)
    return e_gs, e_gr


@pytest.mark.parametrize("bg", ["tensor", 1.0, 0.5])
def test_alpha_mode_equals_the_four_kernel_chain_bit_for_bit(bg):
    """What the header of n2m_composite_loss_train promises, in the instantiation the SDF recipe runs: gradients, opacities and colours are the
    bits of composite forward -> photo loss forward / backward -> composite backward with alpha_mode; the loss up to its summation order."""
    from nerf2mesh_amd import raymarching
    from nerf2mesh_amd.losses import photo_loss
    case = R.edge_case("alpha")
    d, M, ref = _dev(case), case["M"], case["ref"]
    sig, rgb = d["sig"].clone().requires_grad_(), d["rgb"].clone().requires_grad_()
    w, ws, dp, im = raymarching.composite_rays_train(sig, rgb, d["ts"], d["rays"], R.T_THRESH, True)
    loss = photo_loss(im, ws, d["gt"], d["bg"] if bg == "tensor" else bg, R.LAM_RGB, R.LAM_MASK)
    loss.backward(gradient=torch.tensor(R.SCALE, device="cuda"))
    got = _fused(case, "alpha", bg=bg)
    assert np.array_equal(got["gs"][:M], sig.grad.cpu().numpy()) and np.array_equal(got["gr"][:M], rgb.grad.cpu().numpy())
    assert np.array_equal(got["ws"], ws.detach().cpu().numpy()) and np.array_equal(got["image"], im.detach().cpu().numpy())
    assert np.abs(got["gs"][:M]).max() > 0 and np.abs(got["gr"][:M]).max() > 0
    np.testing.assert_allclose(got["loss"], loss.item(), rtol=5e-6)
    assert got["loss_sum"] == np.float32(2.0) + np.float32(got["loss"])
    assert np.array_equal(got["live"], ref["live"])
    assert np.array_equal(got["block_live"], np.add.reduceat(ref["live"], np.arange(0, case["N"], 16)))
    _written(case, got)


@pytest.mark.parametrize("mode", R.MODES)
def test_every_mode_against_float64_per_ray(oracle, mode):
    _against_model(R.edge_case(mode), mode, oracle, _run(mode))


@pytest.mark.parametrize("mode", R.MODES)
def test_placed_stops(mode):
    """The sample a stop falls on keeps its gradient, every later sample of the ray gets exact zeros; the long ray carries gradients through its
    third chunk."""
    case, got = R.edge_case(mode), _run(mode)
    for n, idx in case["placed"]:
        a, c = case["rays"][n].tolist()
        assert got["live"][n] == idx + 1
        assert got["gs"][a + idx] != 0 and got["gr"][a + idx].all(), (n, idx)
        assert np.abs(got["gs"][a:a + idx + 1]).min() > 0                               # and every sample before it
        assert not got["gs"][a + idx + 1:a + c].any() and not got["gr"][a + idx + 1:a + c].any(), (n, idx)
    a, c = case["rays"][case["long"]].tolist()
    assert c == R.LONG and got["live"][case["long"]] == R.LONG
    assert np.abs(got["gs"][a + 128:a + 193]).min() > 0 and np.abs(got["gr"][a + 128:a + 193]).min() > 0


@pytest.mark.parametrize("mode", R.MODES)
def test_ray_cut_off_by_M(oracle, mode):
    """The last ray's range overruns M: exact zeros over the poison inside [off, M), nothing at or behind M, no live samples, no opacity or colour;
    empty rays likewise.  In entropy mode its M - off samples still count as H(1e-5) each in the loss."""
    case, got = R.edge_case(mode), _run(mode)
    M, (a, c) = case["M"], case["rays"][-1].tolist()
    assert a < M < a + c
    assert not got["gs"][a:M].any() and not got["gr"][a:M].any()
    assert (got["gs"][M:] == POISON).all() and (got["gr"][M:] == POISON).all()
    for n in [case["N"] - 1] + [n for n in range(case["N"]) if case["rays"][n, 1] == 0]:
        assert got["live"][n] == 0 and got["ws"][n] == 0 and not got["image"][n].any()
        assert mode != "depth" or got["depth"][n] == 0
    ref, chain = case["ref"], R.oracle_chain(case, mode, oracle)
    assert R.loss_error(got["loss"], ref) <= 4 * max(R.loss_error(chain["loss"], ref), HALF_ULP)
    if mode == "entropy":                         # the bound above sees the term: without the cut-off samples the loss is another one
        without = R.LAM_ENT * (M - a) * R._entropy(R.H_LO) / M
        assert without > 16 * max(R.loss_error(chain["loss"], ref), HALF_ULP) * ref["loss"]


@pytest.mark.parametrize("mode", R.MODES)
def test_same_bits_without_the_ray_outputs(mode):
    """weights_sum / image requested or NULL: the same gradients and loss."""
    got, bare = _run(mode), _fused(R.edge_case(mode), mode, outputs=False)
    assert np.array_equal(got["gs"], bare["gs"]) and np.array_equal(got["gr"], bare["gr"]) and got["loss"] == bare["loss"]
    assert np.array_equal(got["live"], bare["live"]) and bare["ws"] is None


@pytest.mark.parametrize("mode", ["density", "alpha"])
@pytest.mark.parametrize("lams", [(0.0, R.LAM_MASK), (R.LAM_RGB, 0.0)])
def test_one_loss_term_alone_against_float64(oracle, mode, lams):
    case = R.edge_case(mode)
    got = _fused(case, mode, *lams)
    e_gs, e_gr = _against_model(case, mode, oracle, got, lam_rgb=lams[0], lam_mask=lams[1])
    assert np.abs(got["gs"][:case["M"]]).max() > 0 and (e_gr > 0) == (lams[0] > 0)     # the mask term alone sends nothing to the colours


@pytest.mark.parametrize("mode", ["density", "alpha"])
def test_no_loss_term_gives_exact_zeros(mode):
    case = R.edge_case(mode)
    got = _fused(case, mode, 0.0, 0.0)
    assert not got["gs"][:case["M"]].any() and not got["gr"][:case["M"]].any() and got["loss"] == 0.0
    _written(case, got)


@pytest.fixture(scope="module")
def big():
    case = R.big_case()
    ref, f32 = R.big_loss(case, torch.float64), R.big_loss(case, torch.float32)
    return case, ref, 4 * max(abs(f32 - ref) / ref, HALF_ULP), _fused(case, "density")


def test_large_grid_with_the_ticket(big):
    """1026 workgroups: the last workgroup's 1024 threads take a second trip over the partials."""
    case, ref, bound, got = big
    err = abs(got["loss"] - ref) / ref
    print(f"large grid, ticket: loss error {err:.3e}, bound {bound:.3e}, value {ref:.6f}")
    assert len(got["partial"]) == 1026 and err <= bound
    assert got["loss_sum"] == np.float32(2.0) + np.float32(got["loss"])                # advanced by exactly the loss (and the ticket is 0: _fused)
    again = _fused(case, "density")
    assert again["loss"] == got["loss"] and np.array_equal(again["gs"], got["gs"]) and np.array_equal(again["gr"], got["gr"])
    _written(case, got)


def test_large_grid_without_the_ticket(big):
    """ticket = NULL, as the step executor calls it: only the partials are left, and their float64 sum / N is the loss."""
    case, ref, bound, got = big
    bare = _fused(case, "density", ticket=False)
    err = abs(bare["partial"].astype(np.float64).sum() / case["N"] - ref) / ref
    print(f"large grid, no ticket: loss error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert np.array_equal(bare["partial"], got["partial"])
    assert np.array_equal(bare["gs"], got["gs"]) and np.array_equal(bare["gr"], got["gr"]) and np.array_equal(bare["live"], got["live"])
