"""The field kernels with a per-sample appearance code (include/n2m_mlp.h: n2m_field_*_ind, n2m_field_sample_views) and the ray -> view id
(n2m_batch_views).  Shapes: one sample, one full 32-sample tile, two tiles and a ragged tail, and a batch that spans several workgroups;
three code rows of which the last is never named; D in {1, 8, 16}; full and diffuse shading."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MS = [1, 32, 69, 4096 + 17]
DS = [1, 8, 16]
R = 3
W_SHAPES = [(32, 19), (1, 32), (64, 35), (64, 64), (6, 64), (32, 6), (3, 32)]


def _lib():
    from nerf2mesh_amd import _lib as L
    L.lib()
    return L


def make_inputs(M, D, seed=0):
    """Random field inputs in the layouts of n2m_mlp.h; w[2] is the [64, 35 + D] parameter, `w35` its first 35 columns packed."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.rand(*s, device="cuda", generator=g) * 2 - 1
    x = dict(xyz=r(M, 3) * 0.95, dirs=torch.nn.functional.normalize(r(M, 3), dim=-1), h1=r(16, M) * 0.5, h2=(r(16, M, 2) * 0.5).half())
    w = [r(o, i) * (2.0 / i ** 0.5) for o, i in W_SHAPES]
    w[2] = r(64, 35 + D) * (2.0 / 35 ** 0.5)
    x["w"], x["w35"] = w, w[2][:, :35].contiguous()
    x["codes"] = r(R, D) * 0.5
    x["view"] = torch.randint(0, R - 1, (M,), device="cuda", generator=g, dtype=torch.int32)        # row R - 1 is never named
    x["d_sigma"], x["d_rgb"] = r(M) * 64, r(M, 3) * 64
    x["seed"] = torch.full((1,), 128.0, device="cuda")
    return x


def forward(x, shading, ind, train=False, codes=None, view="given"):
    L = _lib()
    p, M = L.ptr, x["xyz"].shape[0]
    sigma, rgb = torch.empty(M, device="cuda"), torch.empty(M, 3, device="cuda")
    spec = torch.empty(M, 3, device="cuda") if shading else None
    part = torch.full((int(L.lib().n2m_field_spec_partials()),), -1.0, device="cuda") if train else None
    w = list(x["w"])
    head = (p(x["xyz"]), p(x["dirs"]) if shading else None, p(x["h1"]), p(x["h2"]))
    if ind:
        c = x["codes"] if codes is None else codes
        v = x["view"] if isinstance(view, str) else view
        tail = (p(c), p(v), R, c.shape[1], M, shading, 0, p(sigma), p(rgb), p(spec))
        if train:
            L.call("n2m_field_forward_ind_train", *head, *[p(t) for t in w], *tail, p(part), L.stream())
        else:
            L.call("n2m_field_forward_ind", *head, *[p(t) for t in w], *tail, L.stream())
    else:
        w[2] = x["w35"]
        tail = (M, shading, 0, p(sigma), p(rgb), p(spec))
        if train:
            L.call("n2m_field_forward_train", *head, *[p(t) for t in w], *tail, p(part), L.stream())
        else:
            L.call("n2m_field_forward", *head, *[p(t) for t in w], *tail, L.stream())
    return dict(sigma=sigma, rgb=rgb, spec=spec, part=part)


def backward(x, shading, ind, train=False, codes=None, view="given"):
    L = _lib()
    p, M = L.ptr, x["xyz"].shape[0]
    d_h1, d_h2 = torch.empty(16, M, device="cuda"), torch.empty(16, M, 2, device="cuda", dtype=torch.float16)
    w = list(x["w"])
    if not ind:
        w[2] = x["w35"]
    dw = [torch.zeros_like(t) for t in w]
    finf = torch.zeros(1, device="cuda")
    head = (p(x["xyz"]), p(x["dirs"]) if shading else None, p(x["h1"]), p(x["h2"]))
    grads = (p(x["d_sigma"]), p(x["d_rgb"]), None, p(d_h1), p(d_h2), *[p(t) for t in dw])
    reg = (0.25 / M, p(x["seed"])) if train else None
    d_codes = None
    if ind:
        c = x["codes"] if codes is None else codes
        v = x["view"] if isinstance(view, str) else view
        d_codes = torch.zeros_like(c)
        need = int(L.lib().n2m_field_ind_workspace_bytes(M, R))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        mid = (p(c), p(v), R, c.shape[1], M, shading, 0)
        if train:
            L.call("n2m_field_backward_ind_train", *head, *[p(t) for t in w], *mid, *grads, p(d_codes), p(ws), need, p(finf), *reg, L.stream())
        else:
            L.call("n2m_field_backward_ind", *head, *[p(t) for t in w], *mid, *grads, p(d_codes), p(ws), need, p(finf), L.stream())
    elif train:
        L.call("n2m_field_backward_train", *head, *[p(t) for t in w], M, shading, 0, *grads, p(finf), *reg, L.stream())
    else:
        L.call("n2m_field_backward", *head, *[p(t) for t in w], M, shading, 0, *grads, p(finf), L.stream())
    torch.cuda.synchronize()
    assert finf.item() == 0
    return dict(d_h1=d_h1, d_h2=d_h2, dw=dw, d_codes=d_codes)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


# ------------------------------------------------------------------------------------------------------------------ 2. zero codes
@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("shading", [1, 0])
@pytest.mark.parametrize("D", DS)
def test_zero_codes_are_the_plain_kernels_bit_for_bit(D, shading, train):
    for M in MS:
        x = make_inputs(M, D, seed=M + D)
        zero = torch.zeros(R, D, device="cuda")
        a, b = forward(x, shading, False, train), forward(x, shading, True, train, codes=zero)
        for k in ("sigma", "rgb") + (("spec",) if shading else ()) + (("part",) if train else ()):
            assert torch.equal(bits(a[k]), bits(b[k])), (M, k)
        ga, gb = backward(x, shading, False, train), backward(x, shading, True, train, codes=zero)
        assert torch.equal(bits(ga["d_h1"]), bits(gb["d_h1"])) and torch.equal(bits(ga["d_h2"]), bits(gb["d_h2"])), M
        for i, (p, q) in enumerate(zip(ga["dw"], gb["dw"])):
            if i == 2:
                q = q[:, :35].contiguous()
            assert torch.equal(bits(p), bits(q)), (M, i)
        assert not gb["dw"][2][:, 35:].any(), "zero codes: the code columns of d W0 are sums of exact zeros"


# ------------------------------------------------------------------------------------------- 4. unused row, determinism; 5. row 0
@pytest.mark.parametrize("shading", [1, 0])
@pytest.mark.parametrize("D", DS)
def test_unreferenced_row_gets_exactly_zero_and_two_calls_give_the_same_bits(D, shading):
    for M in MS:
        x = make_inputs(M, D, seed=7 * M + D)
        a, b = backward(x, shading, True), backward(x, shading, True)
        assert not a["d_codes"][R - 1].any()
        if M > 1:      # (one sample alone may sit in the clamp of `specular + diffuse`, where every gradient is zero)
            assert a["d_codes"][:R - 1].any()
            assert a["dw"][2][:, 35:].any()
        for k in ("d_h1", "d_h2", "d_codes"):
            assert torch.equal(bits(a[k]), bits(b[k])), (M, k)
        for i, (p, q) in enumerate(zip(a["dw"], b["dw"])):
            assert torch.equal(bits(p), bits(q)), (M, i)


@pytest.mark.parametrize("shading", [1, 0])
@pytest.mark.parametrize("D", DS)
def test_null_ids_are_row_zero(D, shading):
    for M in MS:
        x = make_inputs(M, D, seed=11 * M + D)
        zeros = torch.zeros(M, dtype=torch.int32, device="cuda")
        a, b = forward(x, shading, True, view=None), forward(x, shading, True, view=zeros)
        for k in ("sigma", "rgb") + (("spec",) if shading else ()):
            assert torch.equal(bits(a[k]), bits(b[k])), (M, k)
        if M > 1:
            assert not torch.equal(a["rgb"], forward(x, shading, True, view=torch.ones_like(zeros))["rgb"]), "the row matters"
        ga, gb = backward(x, shading, True, view=None), backward(x, shading, True, view=zeros)
        for k in ("d_h1", "d_h2", "d_codes"):
            assert torch.equal(bits(ga[k]), bits(gb[k])), (M, k)
        for i, (p, q) in enumerate(zip(ga["dw"], gb["dw"])):
            assert torch.equal(bits(p), bits(q)), (M, i)
        assert not ga["d_codes"][1:].any()


def test_ids_outside_the_table_are_clamped_and_wide_codes_are_refused():
    L = _lib()
    M, D = 69, 8
    x = make_inputs(M, D)
    low, high = torch.full((M,), -5, dtype=torch.int32, device="cuda"), torch.full((M,), 1 << 20, dtype=torch.int32, device="cuda")
    assert torch.equal(forward(x, 1, True, view=low)["rgb"], forward(x, 1, True, view=None)["rgb"])
    assert torch.equal(forward(x, 1, True, view=high)["rgb"], forward(x, 1, True, view=torch.full_like(low, R - 1))["rgb"])
    assert int(L.lib().n2m_field_ind_max_dim()) == 16
    wide = torch.zeros(R, 17, device="cuda")
    x["w"][2] = torch.zeros(64, 35 + 17, device="cuda")
    with pytest.raises(RuntimeError):
        forward(x, 1, True, codes=wide)


# ---------------------------------------------------------------------------------------------------------- 3. parity with the unfused graph
def _nets(D, seed=0):
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    torch.manual_seed(seed)
    ref = NeRFNetwork(make_options(O=True, bound=1, dt_gamma=0, ind_dim=D, ind_num=R)).cuda()
    with torch.no_grad():
        ref.encoder.embeddings.uniform_(-0.5, 0.5)
        ref.encoder_color.embeddings.uniform_(-0.5, 0.5)
        ref.individual_codes.uniform_(-0.5, 0.5)
    fused = NeRFNetwork(make_options(O=True, bound=1, dt_gamma=0, fused_mlp=True, ind_dim=D, ind_num=R)).cuda()
    fused.load_state_dict(ref.state_dict())
    return ref, fused


def _samples(M, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand(M, 3, device="cuda", generator=g) * 1.9 - 0.95
    d = torch.nn.functional.normalize(torch.randn(M, 3, device="cuda", generator=g), dim=-1)
    view = torch.randint(0, R - 1, (M,), device="cuda", generator=g, dtype=torch.int32)
    return x, d, view, g


def test_can_fuse_truth_table():
    from nerf2mesh_amd.fused import IndCode
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    for D, fused_mlp, sdf, want in ((8, True, False, True), (16, True, False, True), (17, True, False, False), (8, False, False, False),
                                    (8, True, True, False)):
        net = NeRFNetwork(make_options(O=True, bound=1, dt_gamma=0, fused_mlp=fused_mlp, ind_dim=D, ind_num=R, sdf=sdf)).cuda()
        assert net._can_fuse(IndCode(net.individual_codes)) == want, (D, fused_mlp, sdf)
        assert net._can_fuse(net.individual_codes[[0]]) is False, "a gathered tensor is the unfused network's form"
        assert torch.is_tensor(net.ind_code()) != want
    net0 = NeRFNetwork(make_options(O=True, bound=1, dt_gamma=0, fused_mlp=True)).cuda()
    assert net0._can_fuse() and net0.ind_code() is None


@pytest.mark.parametrize("shading", ["full", "diffuse"])
@pytest.mark.parametrize("D", DS)
def test_forward_matches_the_unfused_autocast_network(D, shading):
    """tests/test_mlp_parity.py's tolerances, unchanged."""
    from nerf2mesh_amd.fused import IndCode
    ref, fused = _nets(D)
    for M in MS:
        x, d, view, _ = _samples(M, seed=M)
        with torch.no_grad():
            with torch.autocast("cuda", dtype=torch.float16):
                s0, c0, p0 = ref(x, d, ref.individual_codes[view.long()], shading)
            s1, c1, p1 = fused(x, d, IndCode(fused.individual_codes, view), shading)
        assert (c0.float() - c1).abs().max().item() < 6e-3
        assert (c0.float() - c1).abs().mean().item() < 3e-4
        if shading != "diffuse":
            assert (p0.float() - p1).abs().max().item() < 6e-3
        rel = ((s0.float() - s1).abs() / s0.float().abs().clamp(min=1e-3))
        assert rel.max().item() < 3e-2 and rel.mean().item() < 2e-3
        # the codes are read: other rows, other colours (M = 1 may land on a saturated sample)
        if M > 1:
            with torch.no_grad():
                _, c2, _ = fused(x, d, IndCode(fused.individual_codes, torch.full_like(view, R - 1)), shading)
            assert not torch.equal(c1, c2)


CODE_GRAD_MARGIN = 2.0


@pytest.mark.parametrize("shading", ["full", "diffuse"])
@pytest.mark.parametrize("D", DS)
def test_backward_matches_the_unfused_autocast_network(D, shading):
    """Gradients tests/test_mlp_parity.py covers: its tolerances.  The two new ones (d codes, d W0[:, 35:]): both paths are measured
    against a float64 evaluation of color_net / specular_net on the features the unfused path fed them, and the fused error (relative L2)
    must stay within CODE_GRAD_MARGIN times the unfused path's.  Why 2: both paths round the same operands and the same activation
    gradients to fp16 and differ in accumulation order only -- the fused one keeps fp32 (d W0) and exact (d codes) sums where autocast
    rounds the GEMM output to fp16 -- so their errors are two draws from one distribution at worst; a factor of two covers the spread of a
    norm over 64 D and 2 D entries without admitting a systematic loss of precision."""
    from nerf2mesh_amd.fused import IndCode
    ref, fused = _nets(D)
    M = 4096 + 17
    x, d, view, g = _samples(M, seed=3)
    cs, cc, cp = (torch.randn(M, device="cuda", generator=g), torch.randn(M, 3, device="cuda", generator=g),
                  torch.randn(M, 3, device="cuda", generator=g))
    scale = 128.0

    def loss_of(s, c, p):
        k = torch.float64 if c.dtype == torch.float64 else torch.float32
        l = (c.to(k) * cc.to(k)).sum()
        if s is not None:
            l = l + (torch.log1p(s.float()) * cs).sum()
        if p is not None:
            l = l + 0.3 * (p.to(k) * cp.to(k)).sum()
        return l * scale / M

    with torch.autocast("cuda", dtype=torch.float16):
        s, c, p = ref(x, d, ref.individual_codes[view.long()], shading)
    loss_of(s, c, p).backward()
    c_unfused = c.detach().float()
    s, c, p = fused(x, d, IndCode(fused.individual_codes, view), shading)
    loss_of(s, c, p).backward()
    pr, pf = dict(ref.named_parameters()), dict(fused.named_parameters())
    names = ["sigma_net.net.0.weight", "sigma_net.net.1.weight", "color_net.net.0.weight", "color_net.net.1.weight", "color_net.net.2.weight"]
    if shading != "diffuse":
        names += ["specular_net.net.0.weight", "specular_net.net.1.weight"]
    for nme in names:
        a, b = pr[nme].grad.float(), pf[nme].grad.float()
        if nme == "color_net.net.0.weight":
            a, b = a[:, :35], b[:, :35]
        err = (a - b).abs().max().item() / (a.abs().max().item() + 1e-12)
        assert err < 2e-2, f"{nme}: rel err {err}"
    for nme in ("encoder.embeddings", "encoder_color.embeddings"):
        a, b = pr[nme].grad.float(), pf[nme].grad.float()
        assert torch.isfinite(b).all()
        assert (a - b).abs().max().item() / (a.abs().max().item() + 1e-12) < 5e-2, nme
        assert abs(a.sum().item() - b.sum().item()) <= 2e-2 * a.abs().sum().item() + 1e-6, nme

    # float64 restatement of the colour head on the unfused path's own inputs (fp16 features, fp32 points, directions and parameters)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        h2 = ref.encoder_color(x, bound=ref.bound, max_level=ref.max_level)
    W = [pr[f"color_net.net.{i}.weight"].detach().double().requires_grad_(i == 0) for i in range(3)]
    P = [pr[f"specular_net.net.{i}.weight"].detach().double() for i in range(2)]
    codes = pr["individual_codes"].detach().double().requires_grad_()
    h = torch.cat([x.double(), h2.double(), codes[view.long()]], dim=-1)
    geo = torch.sigmoid(torch.relu(torch.relu(h @ W[0].T) @ W[1].T) @ W[2].T)
    if shading == "diffuse":
        col, spec = geo[:, :3], None
    else:
        spec = torch.sigmoid(torch.relu(torch.cat([d.double(), geo[:, 3:]], dim=-1) @ P[0].T) @ P[1].T)
        col = (spec + geo[:, :3]).clamp(0, 1)
    loss_of(None, col, spec).backward()
    # the float64 restatement is the same graph: its colours are the unfused path's within that path's own fp16 rounding (the bound
    # tests/test_mlp_parity.py puts between two fp16 evaluations).  The GRADIENT errors below are not small in themselves under full
    # shading -- a sample whose `specular + diffuse` lands on the other side of the clamp at 1 in fp16 switches its whole gradient on or
    # off (6-26 % relative L2 for either path) -- which is why the fused path is measured against the unfused one and not against a number
    assert (col.detach().float() - c_unfused).abs().max().item() < 6e-3
    rel = lambda got, want: ((got.double() - want).norm() / want.norm()).item()
    for what, want, unf, fus in (("d codes", codes.grad, pr["individual_codes"].grad, pf["individual_codes"].grad),
                                 ("d W0[:, 35:]", W[0].grad[:, 35:], pr["color_net.net.0.weight"].grad[:, 35:], pf["color_net.net.0.weight"].grad[:, 35:])):
        e_unf, e_fus = rel(unf, want), rel(fus, want)
        print(f"D={D} {shading}: {what}: unfused autocast {e_unf:.3e}, fused {e_fus:.3e} (relative L2 against float64)")
        assert e_fus <= CODE_GRAD_MARGIN * e_unf, (what, e_fus, e_unf)
    assert not pf["individual_codes"].grad[R - 1].any()


# ---------------------------------------------------------------------------------------------------------------------- 1. view ids
def test_batch_views_names_the_view_each_batch_kernel_read():
    from test_ind_codes_cpu import V, H, W, constant_colour_capture
    from nerf2mesh_amd.capture import batch_from_uniforms_u8, batch_views
    cap = constant_colour_capture("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    N = 4096 + 17
    u = torch.rand(N, 6, device="cuda", generator=g)
    u[0, 0], u[1, 0], u[2, 0] = 0.0, float(np.nextafter(np.float32(1), np.float32(0))), 1.0
    aabb = torch.tensor([-1.0, -1, -1, 1, 1, 1], device="cuda")
    depth = torch.rand(V, H * W, device="cuda", generator=g)
    table = torch.tensor(cap.intrinsics, device="cuda").repeat(V, 1) * torch.linspace(1.0, 1.2, V, device="cuda").view(V, 1)
    for name, kw, intr in (("plain", {}, cap.intrinsics), ("depth", dict(dense_depth=depth), cap.intrinsics), ("per view", {}, table),
                           ("per view + depth", dict(dense_depth=depth), table)):
        alone = batch_from_uniforms_u8(cap.poses, cap.bank, cap.lut, u, aabb, 0.05, H, W, intr, **kw)
        ids = batch_views(u, V)
        again = batch_from_uniforms_u8(cap.poses, cap.bank, cap.lut, u, aabb, 0.05, H, W, intr, **kw)
        torch.cuda.synchronize()
        assert ids.dtype == torch.int32 and ids.shape == (N,)
        assert torch.equal(ids, torch.round(alone[2][:, 0] * 255).to(torch.int32)), name
        assert ids[:3].tolist() == [0, V - 1, V - 1]
        assert set(ids.tolist()) == set(range(V))
        for p, q in zip(alone, again):                       # the new launch leaves the batch kernels' outputs as they were
            assert torch.equal(bits(p), bits(q)), name
        if "depth" in name:
            assert torch.equal(alone[7], depth[ids.long(), (u[:, 1] * (H * W)).long().clamp(max=H * W - 1)])


def test_sample_views_spread_the_ray_ids_over_the_marcher_table():
    from nerf2mesh_amd.fused import sample_views
    counts = torch.tensor([3, 0, 70, 1, 130], dtype=torch.int32)
    offs = torch.cumsum(counts, 0) - counts
    rays = torch.stack([offs, counts], dim=1).int().cuda()
    ray_view = torch.tensor([4, 9, 2, 7, 1], dtype=torch.int32, device="cuda")
    M = int(counts.sum())
    got = sample_views(rays, ray_view, M)
    assert torch.equal(got.cpu(), torch.repeat_interleave(ray_view.cpu(), counts.long()))
