"""The fused field kernels (include/n2m_mlp.h) per sample and per weight-gradient entry.

C1: exact cases (tests/field_ref.py: exact_case) -- every sum of the kernels is exact in any order on these inputs, so the comparison with
    the float64 model is bit for bit.  The one inexact operation is the NeRF head's exp.  Its forward tolerance is 4 x the largest relative
    error of torch.exp in fp32 on the device against float64 exp on the same integer pre-activations in [-8, 8]; measured on the MI355X:
    4.380e-08, so the kernel's bound is 1.752e-07 (NERF_EXP_MEASURED; every run measures and prints it again).  Its backward bound is 2^-9 per element: one fp16 rounding of d_sigma exp(pre)
    may flip by an ulp (2^-10), twice that is the margin; zeros of the model are zeros of the kernel.
C2: random fp16 values (tests/test_ind_field_gpu.py: make_inputs), properties that need no tolerance: a sample's outputs do not depend on
    its position (permutation, prefix), nothing is written behind M, and the weight gradients of two orders differ by at most the
    reordering bound M 2^-23 S, S = the entry's sum of absolute terms, taken from field_model on the fp16-rounded inputs."""
import numpy as np
import pytest
import torch

import field_ref as R
from test_ind_field_gpu import _lib, bits, make_inputs

pytestmark = pytest.mark.gpu

NERF_EXP_MEASURED = 4.380e-08      # as recorded; the assertion uses the value the run itself measures
SENTINEL = -777.0


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device="cuda").to(dtype or torch.as_tensor(a).dtype).contiguous()


def to_device(case):
    """The case's inputs as device tensors in the header's dtypes."""
    x = dict(M=case["M"], variant=case["variant"], normalize_dirs=case["normalize_dirs"])
    for k in ("xyz", "dirs", "h1", "d_sigma", "d_rgb", "d_spec"):
        x[k] = _dev(case[k], torch.float32)
    x["h2"] = _dev(case["h2"], torch.float16)
    x["view"] = _dev(case["view"], torch.int32)
    x["w"] = [_dev(t, torch.float32) for t in case["w"]]
    x["codes"] = _dev(case["codes"], torch.float32)
    x["spec_reg"] = float(case["spec_reg"])
    x["seed"] = torch.full((1,), float(case["seed"]), device="cuda")
    return x


def field_forward(x, density, color, shading, train, pad=0):
    """One forward call; outputs are allocated `pad` samples longer and pre-filled with SENTINEL."""
    L = _lib()
    p, M = L.ptr, x["M"]
    full = lambda *s: torch.full(s, SENTINEL, device="cuda")
    sigma = full(M + pad) if density else None
    rgb = full(M + pad, 3) if color else None
    spec = full(M + pad, 3) if (color and shading) else None
    part = torch.full((int(L.lib().n2m_field_spec_partials()),), -1.0, device="cuda") if train else None
    head = (p(x["xyz"]), p(x["dirs"]) if (color and shading) else None, p(x["h1"]) if density else None, p(x["h2"]) if color else None)
    w = [p(t) for t in x["w"]]
    out = (p(sigma), p(rgb), p(spec))
    nd = x["normalize_dirs"]
    if x["codes"] is not None:
        mid = (p(x["codes"]), p(x["view"]), x["codes"].shape[0], x["codes"].shape[1], M, shading, nd)
        if train:
            L.call("n2m_field_forward_ind_train", *head, *w, *mid, *out, p(part), L.stream())
        else:
            L.call("n2m_field_forward_ind", *head, *w, *mid, *out, L.stream())
    elif train:
        L.call("n2m_field_forward_train", *head, *w, M, shading, nd, *out, p(part), L.stream())
    else:
        L.call("n2m_field_forward", *head, *w, M, shading, nd, *out, L.stream())
    torch.cuda.synchronize()
    return dict(sigma=sigma, rgb=rgb, spec=spec, part=part)


def field_backward(x, density, color, shading, train, pad=0, prefill=0.0):
    """One backward call.  d_h1 / d_h2 are flat, `pad` elements longer than [16, M] / [16, M, 2] and pre-filled with SENTINEL (the rows
    have stride M, so the pad lies behind the whole tensor); the weight gradients and d_codes start at `prefill`."""
    L = _lib()
    p, M = L.ptr, x["M"]
    d_h1 = torch.full((16 * M + pad,), SENTINEL, device="cuda") if density else None
    d_h2 = torch.full((32 * M + pad,), SENTINEL, device="cuda", dtype=torch.float16) if color else None
    dw = [torch.full_like(t, prefill) for t in x["w"]]
    finf = torch.zeros(1, device="cuda")
    head = (p(x["xyz"]), p(x["dirs"]) if (color and shading) else None, p(x["h1"]) if density else None, p(x["h2"]) if color else None)
    w = [p(t) for t in x["w"]]
    grads = (p(x["d_sigma"]) if density else None, p(x["d_rgb"]) if color else None, p(x["d_spec"]) if (color and shading and not train) else None,
             p(d_h1), p(d_h2), *[p(t) for t in dw])
    nd = x["normalize_dirs"]
    reg = (x["spec_reg"], p(x["seed"])) if train else ()
    d_codes = None
    if x["codes"] is not None:
        Rn, D = x["codes"].shape
        d_codes = torch.full_like(x["codes"], prefill)
        need = int(L.lib().n2m_field_ind_workspace_bytes(M, Rn))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        mid = (p(x["codes"]), p(x["view"]), Rn, D, M, shading, nd)
        name = "n2m_field_backward_ind_train" if train else "n2m_field_backward_ind"
        L.call(name, *head, *w, *mid, *grads, p(d_codes), p(ws), need, p(finf), *reg, L.stream())
    else:
        name = "n2m_field_backward_train" if train else "n2m_field_backward"
        L.call(name, *head, *w, M, shading, nd, *grads, p(finf), *reg, L.stream())
    torch.cuda.synchronize()
    return dict(d_h1=d_h1, d_h2=d_h2, dw=dw, d_codes=d_codes, found_inf=finf.item())


def same_bits(got, want, dtype, what):
    """Bit for bit against a float64 array of the model (which holds values the dtype represents exactly)."""
    w = torch.as_tensor(np.ascontiguousarray(want)).to(dtype)
    assert torch.equal(w.double(), torch.as_tensor(np.ascontiguousarray(want))), ("the model's value is not a number of the dtype", what)
    g = got.detach().cpu().reshape(w.shape)
    if not torch.equal(bits(g), bits(w)):
        bad = (bits(g) != bits(w)).nonzero()
        first = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} elements differ, first at {first}: kernel {g[first].item()!r}, model {w[first].item()!r}")


def close_rel(got, want, bound, what):
    g, w = got.detach().cpu().double().reshape(want.shape), torch.as_tensor(np.ascontiguousarray(want))
    assert not ((w == 0) & (g != 0)).any(), (what, "nonzero where the model is zero")
    nz = w != 0
    rel = ((g[nz] - w[nz]).abs() / w[nz].abs())
    worst = rel.max().item() if rel.numel() else 0.0
    assert worst <= bound, f"{what}: relative error {worst:.3e} > {bound:.3e}"
    return worst


_EXP_TOL = {}


def nerf_exp_tolerance():
    """4 x the largest relative error of the device's fp32 torch.exp on the integers -8..8 against float64 exp."""
    if "tol" not in _EXP_TOL:
        pre = torch.arange(-8, 9, dtype=torch.float32, device="cuda")
        got = torch.exp(pre).cpu().double()
        want = torch.exp(torch.arange(-8, 9, dtype=torch.float64))
        measured = ((got - want).abs() / want).max().item()
        print(f"NeRF head: torch.exp fp32 on the device vs float64 exp on -8..8: max relative error {measured:.3e}; kernel bound {4 * measured:.3e}")
        _EXP_TOL["tol"] = 4 * measured
    return _EXP_TOL["tol"]


def check_exact(M, v):
    case = R.exact_case(M, 0, v)
    m, x = case["model"], to_device(case)
    nerf = v.density and not v.sdf
    tag = (R.variant_id(v), M)
    # ---- forward
    f = field_forward(x, v.density, v.color, v.shading, v.train)
    if v.color:
        same_bits(f["rgb"], m["rgb"], torch.float32, (tag, "rgb"))
        if v.shading:
            same_bits(f["spec"], m["specular"], torch.float32, (tag, "specular"))
        if v.train:
            assert f["part"].double().sum().item() == m["spec_sq"], (tag, "sum of specular^2")
    if v.density:
        if v.sdf:
            same_bits(f["sigma"], m["sigma"], torch.float32, (tag, "sigma"))
        else:
            close_rel(f["sigma"], m["sigma"], nerf_exp_tolerance(), (tag, "sigma"))
    # ---- backward, on zeroed and on pre-filled weight gradients ("ACCUMULATED into"; 3 = an integer every exact sum can take on top)
    for prefill in (0.0, 3.0):
        b = field_backward(x, v.density, v.color, v.shading, v.train, prefill=prefill)
        assert b["found_inf"] == 0, tag
        if v.color:
            same_bits(b["d_h2"], m["d_h2"], torch.float16, (tag, "d_h2"))
        if v.density:
            if nerf:
                close_rel(b["d_h1"], m["d_h1"], 2.0 ** -9, (tag, "d_h1"))
            else:
                same_bits(b["d_h1"], m["d_h1"], torch.float32, (tag, "d_h1"))
        for i, want in enumerate(m["dw"]):
            got = b["dw"][i]
            if want is None:
                assert (got == prefill).all(), (tag, "a weight gradient of a branch that is off was written", R.W_NAMES[i])
            elif nerf and i < 2:
                if prefill == 0.0:
                    close_rel(got, want, 2.0 ** -9, (tag, "dW_" + R.W_NAMES[i]))
            else:
                same_bits(got, want + prefill, torch.float32, (tag, "dW_" + R.W_NAMES[i], prefill))
        if v.D:
            same_bits(b["d_codes"], m["d_codes"] + prefill, torch.float32, (tag, "d_codes"))      # (the unnamed row: prefill + 0, untouched)


@pytest.mark.parametrize("v", R.all_variants(), ids=R.variant_id)
def test_exact_cases_match_the_model(v):
    for M in R.SMALL_MS:
        check_exact(M, v)


@pytest.mark.parametrize("sdf", [False, True], ids=["nerf", "sdf"])
@pytest.mark.parametrize("M", R.LARGE_MS)
def test_exact_cases_where_the_persistent_grids_wrap(M, sdf):
    check_exact(M, R.FULL._replace(sdf=sdf))


# --------------------------------------------------------------------------------------------------------- C2: random values
def _random_case(M, seed=0, D=0):
    x = make_inputs(M, max(D, 1), seed=seed)
    y = dict(M=M, normalize_dirs=0, xyz=x["xyz"], dirs=x["dirs"], h1=x["h1"], h2=x["h2"], d_sigma=x["d_sigma"], d_rgb=x["d_rgb"], d_spec=None,
             w=list(x["w"]), codes=None, view=None, spec_reg=0.0, seed=x["seed"])
    y["w"][2] = x["w35"]
    return y


def _take(y, idx):
    z = dict(y)
    z["M"] = int(idx.numel())
    for k in ("xyz", "dirs", "d_sigma", "d_rgb"):
        z[k] = y[k][idx].contiguous()
    z["h1"], z["h2"] = y["h1"][:, idx].contiguous(), y["h2"][:, idx].contiguous()
    return z


def _model_of_random(y):
    c = lambda t: t.detach().cpu().double().numpy()
    return R.field_model(c(y["xyz"]), c(y["dirs"]), c(y["h1"].half()), c(y["h2"]), [c(t.half()) for t in y["w"]], shading=1, d_sigma=c(y["d_sigma"]),
                         d_rgb=c(y["d_rgb"]), detail=False)


def test_a_samples_outputs_do_not_depend_on_its_position():
    """Permutation: the second run's per-sample outputs are the first run's, permuted, bit for bit; every weight-gradient entry of the two
    runs agrees within M 2^-23 S (S from field_model on the fp16-rounded inputs: the model's sum of absolute terms of that entry)."""
    M = 129 + 4 * 128
    y = _random_case(M, seed=5)
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(1)).cuda()
    z = _take(y, perm)
    fa, fb = field_forward(y, True, True, 1, False), field_forward(z, True, True, 1, False)
    for k in ("sigma", "rgb", "spec"):
        assert torch.equal(bits(fa[k][perm]), bits(fb[k])), k
    ba, bb = field_backward(y, True, True, 1, False), field_backward(z, True, True, 1, False)
    assert torch.equal(bits(ba["d_h1"].view(16, M)[:, perm]), bits(bb["d_h1"].view(16, M))), "d_h1"
    assert torch.equal(bits(ba["d_h2"].view(16, M, 2)[:, perm]), bits(bb["d_h2"].view(16, M, 2))), "d_h2"
    tr = _model_of_random(z)["trace"]
    for i, name in enumerate(R.W_NAMES):
        key = "dw_" + name + ("_nerf" if i < 2 else "")
        S = torch.as_tensor(tr.dots[key][0])
        diff = (ba["dw"][i].cpu().double() - bb["dw"][i].cpu().double()).abs()
        over = diff > M * 2.0 ** -23 * S
        assert not over.any(), (name, diff[over].max().item())


@pytest.mark.parametrize("m,M", [(1, 33), (31, 128), (127, 129), (129, 257)])
def test_a_prefix_is_the_shorter_call_and_nothing_is_written_behind_M(m, M):
    y = _random_case(M, seed=M)
    z = _take(y, torch.arange(m, device="cuda"))
    pad = 64
    fa, fb = field_forward(y, True, True, 1, False, pad=pad), field_forward(z, True, True, 1, False, pad=pad)
    for k in ("sigma", "rgb", "spec"):
        assert torch.equal(bits(fa[k][:m]), bits(fb[k][:m])), k
        for f, n in ((fa, M), (fb, m)):
            assert (f[k][n:] == SENTINEL).all() and not (f[k][:n] == SENTINEL).any(), (k, "written behind M or not written")
    ba, bb = field_backward(y, True, True, 1, False, pad=pad), field_backward(z, True, True, 1, False, pad=pad)
    assert torch.equal(bits(ba["d_h1"][:16 * M].view(16, M)[:, :m]), bits(bb["d_h1"][:16 * m].view(16, m)))
    assert torch.equal(bits(ba["d_h2"][:32 * M].view(16, M, 2)[:, :m]), bits(bb["d_h2"][:32 * m].view(16, m, 2)))
    for b, n in ((ba, M), (bb, m)):
        assert (b["d_h1"][16 * n:] == SENTINEL).all() and (b["d_h2"][32 * n:] == SENTINEL).all(), "written behind M"
        assert not (b["d_h1"][:16 * n] == SENTINEL).any() and not (b["d_h2"][:32 * n] == SENTINEL).any(), "an element was not written"
