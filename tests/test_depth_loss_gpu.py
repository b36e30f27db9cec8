"""n2m_composite_loss_train with a depth target: the fused loss head with the sparse-depth term (nerf/utils.py:685-705).

Inputs: N = 70 rays whose sample counts include 0, 1, 64, 65 and 130 (the wave scan crosses a 64-sample chunk twice; the 130-sample ray keeps
T > T_thresh to its last sample, so all three chunks carry weights and gradients), one 90-sample ray that reaches T < T_thresh on its first
sample, a third of the rays with gt_depth = 0, weights in (0, 2].

Yardstick for the float comparison: the chain that existed before -- n2m_composite_rays_train_forward, the loss in fp32 torch,
n2m_composite_rays_train_backward with grad_depth (raymarching.composite_rays_train) -- measured against float64 torch autograd of the same
recurrence and loss in the same test; the fused kernel may show at most 4 x the chain's error (a different summation order).  Errors are
maximum absolute differences relative to the largest float64 magnitude of the quantity.  Measured values: DESIGN 4.19."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 70
T_THRESH = 1e-4
LAM_RGB, LAM_MASK, LAM_DEPTH = 1.0, 0.1, 0.1
SCALE = 128.0


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(3)
    counts = [0, 1, 64, 65, 130, 90] + torch.randint(2, 100, (N - 6,), generator=g).tolist()
    perm = torch.randperm(N, generator=g).tolist()
    counts = [counts[i] for i in perm]
    long, early = counts.index(130), counts.index(90)   # the 130-sample ray stays alive through its third chunk; a 90-sample ray stops at once
    offs = np.concatenate([[0], np.cumsum(counts)])
    M = int(offs[-1])
    rays = torch.tensor(np.stack([offs[:-1], counts], -1), dtype=torch.int32)
    dt = torch.rand(M, generator=g) * 0.02 + 0.005
    tmid = torch.empty(M)
    for n in range(N):
        a, c = int(offs[n]), counts[n]
        tmid[a:a + c] = 0.3 + torch.rand(1, generator=g) + torch.cumsum(dt[a:a + c], 0)
    ts = torch.stack([tmid, dt], -1).contiguous()
    sig = torch.rand(M, generator=g) * 12
    a = int(offs[long])
    sig[a:a + 130] *= 0.25                              # sum(sigma dt) ~ 130 * 1.5 * 0.015 = 2.9: T ~ 0.05 at the last sample, far above T_thresh
    a = int(offs[early])
    sig[a:a + 2] = 400.0                                # exp(-400 * 0.025) = 4.5e-5 < T_thresh after the FIRST sample
    ts[a:a + 2, 1] = 0.025
    rgb = torch.rand(M, 3, generator=g)
    gt = torch.rand(N, 4, generator=g)
    bg = torch.rand(N, 3, generator=g)
    gtd = 0.4 + torch.rand(N, generator=g) * 1.5
    gtd[::3] = 0.0
    dw = 2.0 - torch.rand(N, generator=g) * 1.9         # (0.1, 2]
    c = dict(counts=counts, early=early, long=long, M=M, rays=rays, ts=ts, sig=sig, rgb=rgb, gt=gt, bg=bg, gtd=gtd, dw=dw)
    c["cuda"] = {k: v.cuda() for k, v in c.items() if torch.is_tensor(v)}
    return c


def _f64(case, lam_rgb, lam_mask, lam_depth):
    """Float64 autograd of composite_rays_train's recurrence + the loss of nerf/utils.py:658-705, seed gradient SCALE."""
    sig = case["sig"].double().requires_grad_()
    rgb = case["rgb"].double().requires_grad_()
    ts, gt, bg, gtd, dw = (case[k].double() for k in ("ts", "gt", "bg", "gtd", "dw"))
    image, wsum, depth, live = [], [], [], []
    for n in range(N):
        a, c = int(case["rays"][n, 0]), int(case["rays"][n, 1])
        alpha = 1 - torch.exp(-sig[a:a + c] * ts[a:a + c, 1])
        T_after = torch.cumprod(1 - alpha, 0)
        T_before = torch.cat([torch.ones(1, dtype=torch.float64), T_after[:-1]])
        stop = torch.nonzero(T_after.detach() < T_THRESH)
        k = c if len(stop) == 0 else int(stop[0]) + 1
        live.append(k)
        w = (alpha * T_before)[:k]
        image.append((w.unsqueeze(-1) * rgb[a:a + k]).sum(0))
        wsum.append(w.sum())
        depth.append((w * ts[a:a + k, 0]).sum())
    image, wsum, depth = torch.stack(image), torch.stack(wsum), torch.stack(depth)
    pred = image + (1 - wsum).unsqueeze(-1) * bg
    mask = gt[:, 3:]
    target = gt[:, :3] * mask + bg * (1 - mask)
    loss = lam_rgb * ((pred - target) ** 2).mean(-1) + lam_mask * (wsum - mask.squeeze(1)) ** 2
    m = (gtd > 0).double().view(-1, 1)
    loss_depth = dw.view(-1, 1) * (depth.view(-1, 1) * m - gtd.view(-1, 1) * m) ** 2          # [N,1]
    total = (loss + lam_depth * loss_depth).mean()          # the reference's own broadcast: [N] + [N,1] -> [N,N], then the mean
    (total * SCALE).backward()
    return dict(loss=total.item(), gs=sig.grad, gr=rgb.grad, depth=depth.detach(), live=live)


def _chain(case, lam_rgb, lam_mask, lam_depth):
    """The existing kernels: forward, fp32 torch loss, backward with grad_depth."""
    from nerf2mesh_amd import raymarching
    c = case["cuda"]
    sig, rgb = c["sig"].clone().requires_grad_(), c["rgb"].clone().requires_grad_()
    w, ws, depth, im = raymarching.composite_rays_train(sig, rgb, c["ts"], c["rays"], T_THRESH, False)
    pred = im + (1 - ws).unsqueeze(-1) * c["bg"]
    mask = c["gt"][:, 3:]
    target = c["gt"][:, :3] * mask + c["bg"] * (1 - mask)
    loss = lam_rgb * ((pred - target) ** 2).mean(-1) + lam_mask * (ws - mask.squeeze(1)) ** 2
    m = (c["gtd"] > 0).float()
    loss = (loss + lam_depth * c["dw"] * (depth * m - c["gtd"] * m) ** 2).mean()
    loss.backward(gradient=torch.tensor(SCALE, device="cuda"))
    return dict(loss=loss.item(), gs=sig.grad, gr=rgb.grad, depth=depth.detach(), w=w.detach())


def _fused(case, lam_rgb, lam_mask, lam_depth, lam_ent=0.0, gtd="gtd", dw="dw", entry="depth", want_depth=True, alpha_mode=0):
    from nerf2mesh_amd import _lib as L
    c, M = case["cuda"], case["M"]
    p = L.ptr
    d_sr = torch.full((4 * M,), -7.0, device="cuda")
    partial = torch.empty((N + 15) // 16, device="cuda")
    ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
    lv = torch.zeros(1, device="cuda")
    depth = torch.full((N,), -7.0, device="cuda") if want_depth else None
    scale = torch.tensor(SCALE, device="cuda")
    head = L.CompositeLoss(sigmas=p(c["sig"]), rgbs=p(c["rgb"]), ts=p(c["ts"]), rays=p(c["rays"]), M=M, N=N, T_thresh=T_THRESH, gt_rgba=p(c["gt"]),
                           bg=p(c["bg"]), lambda_rgb=lam_rgb, lambda_mask=lam_mask, grad_loss=p(scale), grad_sigmas=p(d_sr[:M]), grad_rgbs=p(d_sr[M:]),
                           partial=p(partial), ticket=p(ticket), loss=p(lv), lambda_entropy=float(lam_ent))
    if entry != "ent":          # + the depth fields: the same entry point's other mode
        head.depth, head.gt_depth, head.depth_weight = p(depth), p(None if gtd is None else c[gtd]), p(None if dw is None else c[dw])
        head.lambda_depth, head.alpha_mode = float(lam_depth), int(alpha_mode)
    L.call("n2m_composite_loss_train", ctypes.addressof(head), L.stream())
    torch.cuda.synchronize()
    assert int(ticket) == 0
    return dict(loss=lv.item(), gs=d_sr[:M].clone(), gr=d_sr[M:].view(M, 3).clone(), depth=depth)


def _err(got, ref):
    return ((got.double().cpu() - ref).abs().max() / ref.abs().max()).item()


@pytest.mark.parametrize("lam_ent", [0.0, 1e-3])
def test_depth_off_is_the_entropy_head_bit_for_bit(case, lam_ent):
    """lambda_depth = 0, and separately gt_depth = 0 everywhere: gradients and loss bit-identical to the call without the depth fields."""
    want = _fused(case, LAM_RGB, LAM_MASK, 0.0, lam_ent, entry="ent")
    case["cuda"]["zero"] = torch.zeros(N, device="cuda")
    for kw in (dict(lam_depth=0.0), dict(lam_depth=LAM_DEPTH, gtd="zero"), dict(lam_depth=LAM_DEPTH, gtd=None, dw=None)):
        got = _fused(case, LAM_RGB, LAM_MASK, lam_ent=lam_ent, **kw)
        assert torch.equal(got["gs"], want["gs"]) and torch.equal(got["gr"], want["gr"]), kw
        assert got["loss"] == want["loss"], kw
    assert not (want["gs"] == -7.0).any() and not (want["gr"] == -7.0).any()          # every sample of every ray was written


def test_depth_term_against_float64_within_four_times_the_chain(case):
    ref = _f64(case, LAM_RGB, LAM_MASK, LAM_DEPTH)
    chain = _chain(case, LAM_RGB, LAM_MASK, LAM_DEPTH)
    got = _fused(case, LAM_RGB, LAM_MASK, LAM_DEPTH)
    # the float64 recurrence stops where the fp32 one does (no stop decision sits on the threshold), and the early ray stops at once
    live32 = [int((chain["w"][a:a + c] != 0).sum()) for a, c in case["rays"].tolist()]
    assert live32 == ref["live"] and ref["live"][case["early"]] == 1 and case["counts"][case["early"]] == 90
    # ... and the longest ray composites into its third 64-sample chunk: second carry of the running depth, gradient terms past sample 128
    assert case["counts"][case["long"]] == 130 and ref["live"][case["long"]] > 128
    a = int(case["rays"][case["long"], 0])
    assert ref["gs"][a + 128:a + 130].abs().min() > 0 and got["gs"][a + 128:a + 130].abs().min() > 0
    for k in ("gs", "gr"):
        e_chain, e_fused = _err(chain[k], ref[k]), _err(got[k], ref[k])
        print(f"{k}: chain {e_chain:.3e}, fused {e_fused:.3e}")
        assert e_fused <= 4 * e_chain, (k, e_fused, e_chain)
    l_chain, l_fused = abs(chain["loss"] - ref["loss"]) / abs(ref["loss"]), abs(got["loss"] - ref["loss"]) / abs(ref["loss"])
    print(f"loss: chain {l_chain:.3e}, fused {l_fused:.3e}, value {ref['loss']:.6f}")
    # the loss value: one fp32 number; the chain's own error can be an exact 0 by luck, so its floor is half an ulp of the value
    assert l_fused <= 4 * max(l_chain, 2.0 ** -24), (l_fused, l_chain)
    # the weights matter: without them the gradient is another one
    flat = _fused(case, LAM_RGB, LAM_MASK, LAM_DEPTH, dw=None)
    assert (flat["gs"] - got["gs"]).abs().max() > 1e-3 * got["gs"].abs().max()


def test_depth_alone_drives_the_density_gradient(case):
    """lambda_rgb = lambda_mask = 0: the only gradient is the depth term's (this is the test that needs the new entry point)."""
    ref = _f64(case, 0.0, 0.0, LAM_DEPTH)
    chain = _chain(case, 0.0, 0.0, LAM_DEPTH)
    got = _fused(case, 0.0, 0.0, LAM_DEPTH)
    assert got["gs"].abs().max() > 0 and ref["gs"].abs().max() > 0
    e_chain, e_fused = _err(chain["gs"], ref["gs"]), _err(got["gs"], ref["gs"])
    print(f"gs (depth only): chain {e_chain:.3e}, fused {e_fused:.3e}")
    assert e_fused <= 4 * e_chain, (e_fused, e_chain)
    assert not got["gr"].any() and not ref["gr"].any()                             # colours do not enter the depth
    # the 130-sample ray on its own scale (its gradients are small beside the batch's largest): three chunks, same bound
    a = int(case["rays"][case["long"], 0])
    e_chain, e_fused = _err(chain["gs"][a:a + 130], ref["gs"][a:a + 130]), _err(got["gs"][a:a + 130], ref["gs"][a:a + 130])
    print(f"gs (depth only, 130-sample ray): chain {e_chain:.3e}, fused {e_fused:.3e}")
    assert ref["gs"][a + 128:a + 130].abs().min() > 0 and e_fused <= 4 * e_chain, (e_fused, e_chain)
    # rays without a keypoint depth (gt_depth = 0) receive nothing
    for n in range(0, N, 3):
        a, c = case["rays"][n].tolist()
        assert not got["gs"][a:a + c].any()


def test_depth_output_equals_the_forward_kernel(case):
    chain = _chain(case, LAM_RGB, LAM_MASK, LAM_DEPTH)
    got = _fused(case, LAM_RGB, LAM_MASK, LAM_DEPTH)
    assert torch.equal(got["depth"], chain["depth"])
    assert _fused(case, LAM_RGB, LAM_MASK, LAM_DEPTH, want_depth=False)["depth"] is None


def test_alpha_mode_with_depth_is_refused(case):
    with pytest.raises(RuntimeError, match=r"n2m_composite_loss_train failed \(-3\)"):
        _fused(case, LAM_RGB, LAM_MASK, LAM_DEPTH, alpha_mode=1)
