"""The optimizer model of tests/adam_ref.py on the CPU: adam_f64 against torch.optim.Adam in float64, the float32 restatement inside adam_f64's
bound on every generated case (with the error-to-bound ratio in the message), scaler_ref against torch.amp.GradScaler's update rule, and the
checker of tests/test_adam_exact_gpu.py against images it must accept and images it must refuse."""
import math

import numpy as np
import pytest
import torch

import adam_ref as R


def test_adam_f64_is_torch_adam_over_five_steps_with_a_late_joining_parameter():
    """Five steps of torch.optim.Adam (float64, CPU) on two parameters, the second of which gets its first gradient at step 3 and so counts its own
    steps: adam_f64 with bias[slot] of each parameter's own count, to 1e-12 relative.  The model takes float32 inputs, so the chain is restarted
    from float32-rounded state every step on both sides."""
    rng = np.random.default_rng(0)
    lr, eps, b1, b2 = [float(np.float32(x)) for x in (1e-2, 1e-8, R.BETA1, R.BETA2)]
    # betas exactly as the model takes them: float32 beta, omb = float32(1 - beta in double)
    n = 257
    state = [dict(p=rng.standard_normal(n).astype(np.float32), m=np.zeros(n, np.float32), v=np.zeros(n, np.float32), t=0) for _ in range(2)]
    for step in range(5):
        live = [0, 1] if step >= 2 else [0]
        for k in live:
            s = state[k]
            s["t"] += 1
            g = (rng.standard_normal(n) * 0.3).astype(np.float32)
            # torch, one step from this state at this parameter's own step count.  torch's Adam forms 1 - beta from ONE double beta and its bias
            # corrections in double; the model normally takes beta, 1 - beta and the corrections as separately rounded floats.  To compare the
            # same numbers the model is given torch's doubles here (_adam_f64_with); what the float rounding is worth is the next test's.
            tp = torch.tensor(s["p"], dtype=torch.float64, requires_grad=True)
            opt = torch.optim.Adam([tp], lr=lr, betas=(b1, b2), eps=eps)
            opt.state[tp] = dict(step=torch.tensor(float(s["t"] - 1)), exp_avg=torch.tensor(s["m"], dtype=torch.float64),
                                 exp_avg_sq=torch.tensor(s["v"], dtype=torch.float64))
            tp.grad = torch.tensor(g, dtype=torch.float64)
            opt.step()
            bc1 = 1.0 - b1 ** s["t"]
            bc2 = math.sqrt(1.0 - b2 ** s["t"])
            r = _adam_f64_with(s["p"], s["m"], s["v"], g, None, bc1, bc2, lr, eps, b1, b2, 1.0 - b1, 1.0 - b2)
            st = opt.state[tp]
            for got, want in ((r["p"], tp.detach().numpy()), (r["m"], st["exp_avg"].numpy()), (r["v"], st["exp_avg_sq"].numpy())):
                rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
                assert rel.max() <= 1e-12, (step, k, rel.max())
            s["p"], s["m"], s["v"] = (tp.detach().numpy().astype(np.float32), st["exp_avg"].numpy().astype(np.float32),
                                      st["exp_avg_sq"].numpy().astype(np.float32))
    assert state[0]["t"] == 5 and state[1]["t"] == 3


def _adam_f64_with(p, m, v, g, scale, bc1, bc2, lr, eps, b1, b2, o1, o2):
    """adam_f64's expression with every scalar given in double (bc1, bc2, omb not rounded to float): the same code path through a subclassed
    rounding -- adam_f64 rounds its scalars with adam_ref.f32 and adam_ref.omb, replaced here by the identity."""
    from unittest import mock
    with mock.patch.object(R, "f32", np.float64), mock.patch.object(R, "omb", lambda beta: {b1: o1, b2: o2}[float(beta)]):
        return R.adam_f64(p, m, v, g, scale, bc1, bc2, lr, eps, b1, b2)


def test_adam_f64_rounds_its_scalars_as_the_kernel_receives_them():
    """With float scalars the model differs from the double-scalar evaluation by what the rounding of beta, 1 - beta, bias and lr is worth, and
    omb is float32(1 - beta) with the subtraction in double, NOT 1.0f - float32(beta) (5e-5 apart for beta2)."""
    assert R.omb(0.999) == np.float32(1.0 - 0.999) and R.omb(0.999) != np.float32(1.0) - np.float32(0.999)
    assert abs(float(np.float32(1.0) - np.float32(0.999)) / float(R.omb(0.999)) - 1.0) > 1e-5
    rng = np.random.default_rng(1)
    p, m, v, g = (rng.standard_normal(64).astype(np.float32) for _ in range(4))
    v = v * v
    a = R.adam_f64(p, m, v, g, 3.0, 0.1, 0.0316, 1e-2, 1e-15)
    b = _adam_f64_with(p, m, v, g, 3.0, 0.1, 0.0316, 1e-2, 1e-15, R.BETA1, R.BETA2, 1.0 - R.BETA1, 1.0 - R.BETA2)
    rel = np.abs(a["v"] - b["v"]) / b["v"]
    assert 0 < rel.max() < 1e-6


def test_adam_f32_lies_inside_the_float64_bound_on_every_generated_case():
    """The bound is a bound (a correct float32 evaluation passes it) and not a vacuous one (the largest error-to-bound ratio is well above 1e-6)."""
    worst = dict(p=0.0, m=0.0, v=0.0)
    count = 0
    for la in R.all_launches():
        for t, (r32, r64) in zip(la.tensors, la.expected()):
            for key in worst:
                err, bound = np.abs(r32[key].astype(np.float64) - r64[key]), r64["b" + key]
                assert np.all(err <= bound), (la.name, t["name"], key, float((err / np.maximum(bound, 1e-300)).max()))
                worst[key] = max(worst[key], float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0))))
            count += t["n"]
    msg = f"largest |adam_f32 - adam_f64| / bound over {count} elements: p {worst['p']:.3f}, m {worst['m']:.3f}, v {worst['v']:.3f}"
    print(msg)
    assert all(0.05 < w < 1.0 for w in worst.values()), msg


def test_generated_cases_cover_what_they_claim():
    las = R.all_launches()
    assert len(las) <= 40, "tens of launches, not thousands"
    singles = [t for la in las if la.name.startswith("single") for t in la.tensors]
    seen = {(t["n"], t["g_half"], t["mode"], t["clear"]) for t in singles}
    assert len(seen) == len(R.SIZES) * 2 * 3
    assert {la.scale for la in las if la.name.startswith("single")} == set(R.SCALES)
    assert {la.eps for la in las if la.name.startswith("single")} == {float(np.float32(e)) for e in R.EPSS}
    for la in las:
        assert len({t["slot"] for t in la.tensors}) == len(la.tensors) and len({t["lr"] for t in la.tensors}) == len(la.tensors)
        assert len({tuple(r) for r in la.bias.tolist()}) == 1 + R.ADAM_MAX
        for t in la.tensors:
            z = float(np.mean(np.asarray(t["g"], np.float32) == 0))
            assert t["n"] < 64 or 0.2 < z < 0.47, (la.name, t["name"], z)
            assert np.all(t["m"] != 0) and np.all(t["v"] > 0)
    assert len(R.sixteen_launch().tensors) == 16 and any(t["partner_of"] is not None for t in R.sixteen_launch().tensors)


def test_the_checker_accepts_the_float32_restatement_and_refuses_subtly_wrong_images():
    """check_launch on images made by the float32 restatement (the CPU stand-in for the kernel), then on the same images with one thing wrong
    each: a sentinel byte, a stale shadow element, a kept clear_grad gradient, a partner updated with the host tensor's bias slot, 1.0f - beta
    for omb, an fp16 slot sum rounded per slot."""
    for la in R.all_launches():
        before = la.arena.image()
        w = R.check_launch(la, before, la.emulate(before))
        assert max(w.values()) < 1.0
        R.check_launch(la, before, la.emulate(before, skip=True), skip=True)
    la = R.sixteen_launch()
    before = la.arena.image()
    good = la.emulate(before)
    ar = la.arena

    def refused(img, what, **kw):
        with pytest.raises(AssertionError, match=what):
            R.check_launch(la, before, img, **kw)

    bad = good.copy(); bad[ar.start("t3.p") + 4 * la.tensors[3]["n"]] ^= 1                      # one byte behind a parameter
    refused(bad, "sentinel behind t3.p")
    bad = good.copy(); bad[ar.start("t0.m") - 1] ^= 0x80
    refused(bad, "sentinel in front of t0.m")
    k = next(i for i, t in enumerate(la.tensors) if t["mode"] == 1 and t["n"] % 4 == 1 and t["n"] > 4)
    name = la.tensors[k]["name"]
    s0 = ar.start(f"{name}.shadow") + 2 * (la.tensors[k]["n"] - 1)
    bad = good.copy(); bad[s0:s0 + 2] = before[s0:s0 + 2]                                       # the tail's last shadow element not refreshed
    refused(bad, f"inside {name}.shadow")
    k = next(i for i, t in enumerate(la.tensors) if t["clear"])
    g0 = ar.start(f"t{k}.g")
    bad = good.copy(); bad[g0:g0 + 4] = before[g0:g0 + 4]
    refused(bad, f"inside t{k}.g")
    bad = la.emulate(before, skip=True); bad[ar.start("t1.p")] ^= 1
    refused(bad, "inside t1.p", skip=True)
    # arithmetic: the partner with the host tensor's bias slot; omb1 = 1.0f - beta1
    a = next(i for i, t in enumerate(la.tensors) if t["partner_of"] is not None)
    host = la.tensors[la.tensors[a]["partner_of"]]
    args = la.tensor_args(la.tensors[a])
    args["bc1"], args["bc2"] = la.bias[host["slot"]]
    outs = [r32 for r32, _ in la.expected()]
    outs[a] = R.adam_f32(**args)
    refused(la.apply(before, outs), rf"\(a\) sixteen t{a}\.p")
    from unittest import mock
    # (1.0f - 0.9f is one ulp, 4 u, from float32(0.1): as large as C_M allows the whole of m' -- it is the bit comparison (b) that sees it)
    true_omb = R.omb
    with mock.patch.object(R, "omb", lambda beta: np.float32(1.0) - np.float32(beta) if beta == R.BETA1 else true_omb(beta)):
        outs = [R.adam_f32(**la.tensor_args(t)) for t in la.tensors]
    refused(la.apply(before, outs), r"\(b\) sixteen t\d+\.m")
    # the peer form's fp16 slot sum, rounded to half after every slot instead of once
    la = next(x for x in R.peer_launches() if x.world == 3)
    before = la.arena.image()
    k = next(i for i, t in enumerate(la.tensors) if t["slots"] is not None and t["g_half"])
    args = la.tensor_args(la.tensors[k])
    acc = np.zeros(la.tensors[k]["n"], np.float16)
    for s in la.tensors[k]["slots"]:
        acc = (acc.astype(np.float32) + s.astype(np.float32)).astype(np.float16)
    assert np.any(acc.astype(np.float32) != args["g"])
    args["g"] = acc
    outs = [r32 for r32, _ in la.expected()]
    outs[k] = R.adam_f32(**args)
    with pytest.raises(AssertionError, match=rf"\(a\) {la.name} t{k}\."):
        R.check_launch(la, before, la.apply(before, outs))


# ------------------------------------------------------------------------------------------------ bookkeeping
def _torch_update(scale, tracker, found_inf, growth, backoff, interval):
    """torch.amp.GradScaler.update()'s rule through the op GradScaler itself calls, on CPU tensors; where this build has no CPU kernel for it,
    the statement of torch/amp/grad_scaler.py + ATen's amp_update_scale: back off and reset on an overflow, else count, and at `interval`
    grow (unless the product is not finite) and reset."""
    s, t, f = torch.tensor(float(scale)), torch.tensor(int(tracker), dtype=torch.int32), torch.tensor(float(found_inf))
    try:
        torch._amp_update_scale_(s, t, f, growth, backoff, int(interval))
    except (RuntimeError, NotImplementedError):
        if float(f) != 0.0:
            s, t = s * backoff, torch.tensor(0, dtype=torch.int32)
        else:
            t = t + 1
            if int(t) == int(interval):
                if bool(torch.isfinite(s * growth)):
                    s = s * growth
                t = torch.tensor(0, dtype=torch.int32)
    return float(s), int(t)


def test_scaler_ref_follows_gradscaler_on_a_scripted_sequence():
    growth, backoff, interval = R.GROWTH
    flags = [0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0]
    scale, tracker, steps = np.float32(3.0 * 65536.0), np.float32(0.0), [0.0] * (1 + R.ADAM_MAX)
    ts, tt = float(scale), 0
    clean, seen = 0, []
    for i, flag in enumerate(flags):
        participants = 0b01 if i < 6 else 0b11                 # slot 2 joins at the seventh step
        before = list(steps)
        scale, tracker, found, steps, bias = R.scaler_ref(scale, tracker, float(flag), steps, participants, growth, backoff, interval)
        ts, tt = _torch_update(ts, tt, float(flag), growth, backoff, interval)
        assert float(scale) == ts and float(tracker) == float(tt) and float(found) == 0.0, (i, scale, ts, tracker, tt)
        clean += 0 if flag else 1
        seen.append(ts)
        assert steps[0] == clean and steps[1] == clean
        assert steps[2] == before[2] + (1.0 if (not flag and i >= 6) else 0.0) and steps[3] == 0.0
        # the corrections of the NEXT step, in double, rounded to float: what torch.optim.Adam computes on the host at that step
        for s in (0, 1, 2, 3):
            t = steps[s] + 1.0
            assert bias[s, 0] == np.float32(1.0 - R.BETA1 ** t) and bias[s, 1] == np.float32(math.sqrt(1.0 - R.BETA2 ** t))
    assert max(seen) > 3.0 * 65536.0 > min(seen) and steps[2] < steps[1], "the sequence grows, backs off, and slot 2 joined late"


def test_scaler_ref_does_not_grow_into_inf_and_handles_absent_state():
    growth, backoff, interval = R.GROWTH
    s, t, f, steps, _ = R.scaler_ref(np.float32(2.0e38), 2.0, 0.0, [4.0] * 17, 0, growth, backoff, interval)
    assert s == np.float32(2.0e38) and t == 0.0 and steps[0] == 5.0 and steps[1] == 4.0
    s, t, *_ = R.scaler_ref(np.float32(1.4e38), 2.0, 0.0, [0.0] * 17, 0, growth, backoff, interval)
    assert s == np.float32(1.4e38) * np.float32(2.0) and np.isfinite(s) and t == 0.0
    s, t, *_ = R.scaler_ref(np.float32(1.6e38), 2.0, 0.0, [0.0] * 17, 0, growth, backoff, interval)           # 3.2e38 is finite, and refused
    assert s == np.float32(1.6e38) and t == 0.0
    s, t, *_ = R.scaler_ref(None, None, 1.0, [0.0] * 17, 0, growth, backoff, interval)
    assert s is None and t is None


def test_loss_ref_bounds_a_float32_sum_in_the_kernels_order():
    """The 256-lane, stride-256 order of the bookkeeping's sums in numpy float32 lies inside loss_ref's bound for every case, and not by six orders."""
    worst = 0.0
    for c in R.loss_cases():
        tot = []
        for x in (c["part"], c["extra"], c["extra2"]):
            acc = np.zeros(256, np.float32)
            for base in range(0, len(x), 256):
                chunk = x[base:base + 256]
                acc[:len(chunk)] = acc[:len(chunk)] + chunk
            waves = []
            for w in range(4):
                a = acc[64 * w:64 * w + 64].copy()
                while len(a) > 1:                              # a butterfly: some fixed tree over the lanes
                    a = a[:len(a) // 2] + a[len(a) // 2:]
                waves.append(a[0])
            t = np.float32(0.0)
            for a in waves:
                t = t + a
            tot.append(t)
        v = tot[0] * (np.float32(1.0) / np.float32(c["n_rays"]))
        v = v + tot[1] * np.float32(c["extra_scale"])
        v = v + tot[2] * np.float32(c["extra2_scale"])
        value, bound = R.loss_ref(c["part"], c["n_rays"], c["extra"], c["extra_scale"], c["extra2"], c["extra2_scale"])
        tight = R.loss_bound_in_kernel_order(c["part"], c["n_rays"], c["extra"], c["extra_scale"], c["extra2"], c["extra2_scale"])
        assert abs(float(v) - value) <= min(bound, tight), (len(c["part"]), float(v), value, bound, tight)
        worst = max(worst, abs(float(v) - value) / tight)
    assert 1e-3 < worst < 1.0, worst
    assert sorted(len(c["part"]) for c in R.loss_cases()) == sorted(R.COUNTS)
    assert all(len({len(c["part"]), len(c["extra"]), len(c["extra2"])}) == 3 for c in R.loss_cases())
