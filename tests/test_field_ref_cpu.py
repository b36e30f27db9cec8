"""tests/field_ref.py on its own, without a GPU: the float64 model against torch autograd (B1), the conditions of the exact cases for every
(M, variant) the GPU test runs (B2), and that the cases are not blind to the defects the GPU test is there to catch (B3)."""
import numpy as np
import pytest
import torch

import field_ref as R

# float64 sigmoid(-64) is 1.6e-28 where fp16 and fp32 give exactly 0: the torch graph carries such a term times (gradient x weights)
# <= 2^20 per sample and 257 samples into sums the model leaves untouched.  1e-18 covers that and is 2^-45 of the smallest nonzero
# value of a case (2^-14); everything else is held to rtol 1e-12.
SIGMOID_FLOOR = 1e-18


def _torch_graph(case):
    """The same call as plain float64 torch: F.linear, relu, sigmoid (fp16 output), clamp, autograd."""
    v, M = case["variant"], case["M"]
    t = lambda a, g=False: torch.tensor(np.asarray(a, np.float64), requires_grad=g)
    F = torch.nn.functional

    def sigmoid(z):
        """torch.sigmoid with its output rounded to fp16 as autocast returns it (value only; the gradient is float64 sigmoid's).  Without
        it float64's sigmoid(-64) = 1.6e-28 instead of 0 opens specular_net ReLUs whose pre-activation is exactly 0 on the case."""
        s = torch.sigmoid(z)
        return s + (s.detach().half().double() - s.detach())

    w = [t(a, True) for a in case["w"]]
    x, h1, h2 = t(case["xyz"]), t(case["h1"], True), t(case["h2"], True)
    out, loss = {}, 0.0
    if v.density:
        o = F.linear(F.relu(F.linear(torch.cat([x, h1.T], dim=1), w[0])), w[1])[:, 0]
        out["sigma"] = o if v.sdf else torch.exp(o)
        loss = loss + (out["sigma"] * t(case["d_sigma"])).sum()
    codes = None
    if v.color:
        cols = [x, h2.permute(1, 0, 2).reshape(M, 32)]
        if v.D:
            codes = t(case["codes"], True)
            cols.append(codes[torch.as_tensor(case["view"]).long()])
        geo = sigmoid(F.linear(F.relu(F.linear(F.relu(F.linear(torch.cat(cols, dim=1), w[2])), w[3])), w[4]))
        rgb = geo[:, :3]
        if v.shading:
            d = t(R.safe_normalize(case["dirs"]) if v.raw_dirs else case["dirs"])
            spec = sigmoid(F.linear(F.relu(F.linear(torch.cat([d, geo[:, 3:]], dim=1), w[5])), w[6]))
            out["specular"] = spec
            rgb = spec if v.shading == 2 else (spec + geo[:, :3]).clamp(0, 1)
            if case["d_spec"] is not None:
                loss = loss + (spec * t(case["d_spec"])).sum()
            if v.train:      # the regulariser's gradient is specular * spec_reg * seed: d/ds of (k / 2) s^2
                loss = loss + 0.5 * R.SPEC_K * (spec * spec).sum()
        out["rgb"] = rgb
        loss = loss + (rgb * t(case["d_rgb"])).sum()
    loss.backward()
    out["dw"] = [p.grad for p in w]
    out["d_h1"], out["d_h2"], out["d_codes"] = h1.grad, h2.grad, None if codes is None else codes.grad
    return out


B1_VARIANTS = [R.Variant(True, True, sh, sdf, raw, train, D)
               for sh, sdf, raw, train, D in ((0, False, False, False, 0), (1, False, False, False, 16), (2, False, True, True, 1),
                                              (0, True, False, False, 1), (1, True, True, True, 0), (2, True, False, False, 16))]


@pytest.mark.parametrize("v", B1_VARIANTS, ids=R.variant_id)
def test_model_is_the_float64_torch_graph_on_an_exact_case(v):
    """Once per shading and once per head.  On an exact case the model's roundings are identities, so both are the same graph."""
    case = R.exact_case(257, 0, v)
    m, ref = case["model"], _torch_graph(case)
    close = lambda a, b, what: np.testing.assert_allclose(a, b.detach().numpy(), rtol=1e-12, atol=SIGMOID_FLOOR, err_msg=what)
    close(m["sigma"], ref["sigma"], "sigma")
    close(m["rgb"], ref["rgb"], "rgb")
    if v.shading:
        close(m["specular"], ref["specular"], "specular")
    if not v.sdf:       # the NeRF head's gradients carry the one fp16 rounding of d_sigma exp(pre): 2^-11 relative, and once more in d_h1;
        # where the integer factor of an element is 0 the float64 graph is left with its own cancellation noise (1e-14 at these sizes)
        np.testing.assert_allclose(m["d_h1"], ref["d_h1"].numpy(), rtol=2.0 ** -10, atol=1e-9)
        for i in (0, 1):
            np.testing.assert_allclose(m["dw"][i], ref["dw"][i].numpy(), rtol=2.0 ** -11, atol=1e-9)
    else:
        close(m["d_h1"], ref["d_h1"], "d_h1")
    close(m["d_h2"], ref["d_h2"], "d_h2")
    for i, (a, b) in enumerate(zip(m["dw"], ref["dw"])):
        if a is not None and (v.sdf or i >= 2):
            close(a, b, "dW_" + R.W_NAMES[i])
    if v.D:
        close(m["d_codes"], ref["d_codes"], "d_codes")


def _chunks(n):
    cases = R.gpu_cases()
    return [cases[i::n] for i in range(n)]


@pytest.mark.parametrize("part", range(8))
def test_conditions_hold_for_every_case_the_gpu_test_runs(part):
    """exact_case asserts conditions 1-8 itself (check_case); here for every (M, variant) of tests/test_field_exact_gpu.py."""
    seen = 0
    for M, v in _chunks(8)[part]:
        case = R.exact_case(M, 0, v)
        assert case["M"] == M and case["xyz"].shape == (M, 3) and case["h1"].shape == (16, M) and case["h2"].shape == (16, M, 2)
        if M >= 127 and v.color and v.shading == 1:
            assert all(case["counts"][f"clamp_{t}"] > 0 for t in (0.0, 1.0, 1.5, 2.0))
        seen += 1
    assert seen > 0


def _model(case, **over):
    c = dict(case, **over)
    v = c["variant"]
    return R.field_model(c["xyz"], c["dirs"], c["h1"], c["h2"], c["w"], c["codes"], c["view"], shading=v.shading, normalize_dirs=c["normalize_dirs"],
                         density=v.density, color=v.color, d_sigma=c["d_sigma"], d_rgb=c["d_rgb"], d_specular=c["d_spec"],
                         spec_k=R.SPEC_K if v.train else 0.0, detail=False)


@pytest.mark.parametrize("M", [129, 257])
def test_planted_defects_are_visible(M):
    """Each defect is applied to the model's inputs or outputs, never to a kernel; the clean output must differ somewhere."""
    case = R.exact_case(M, 0, R.FULL)
    clean = case["model"]
    # swap two levels of h2
    h2 = case["h2"].copy()
    h2[[3, 4]] = h2[[4, 3]]
    bad = _model(case, h2=h2)
    assert not np.array_equal(bad["rgb"], clean["rgb"]) and not np.array_equal(bad["d_h2"], clean["d_h2"])
    swapped = clean["d_h2"].copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    assert not np.array_equal(swapped, clean["d_h2"]), "d_h2 with two levels swapped on the way out"
    # the last partial tile's samples missing from dW
    tail = M - (M // 32) * 32
    assert tail > 0
    keep = np.arange(M - tail)
    short = {k: case[k][keep] for k in ("xyz", "dirs", "d_sigma", "d_rgb", "d_spec")}
    short.update(h1=case["h1"][:, keep], h2=case["h2"][:, keep])
    bad = _model(case, **short)
    for i in range(7):
        assert not np.array_equal(bad["dw"][i], clean["dw"][i]), R.W_NAMES[i]
    # sample i + 32's direction for sample i
    dirs = case["dirs"].copy()
    dirs[:M - 32] = case["dirs"][32:]
    bad = _model(case, dirs=dirs)
    assert not np.array_equal(bad["specular"], clean["specular"]) and not np.array_equal(bad["d_h2"], clean["d_h2"])
    # one 32 x 32 block of w_color1 transposed
    w = [t.copy() for t in case["w"]]
    w[3][32:, :32] = case["w"][3][32:, :32].T
    bad = _model(case, w=w)
    assert not np.array_equal(bad["rgb"], clean["rgb"]) and not np.array_equal(bad["d_h2"], clean["d_h2"])
