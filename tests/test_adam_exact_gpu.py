"""The fused optimizer pass and its bookkeeping (n2m_adam_step, n2m_adam_step_scaler, n2m_adam_step_peer, n2m_scaler_update_slots) per element
against the model of tests/adam_ref.py: ONE step from random non-trivial state (moments non-zero, a third of the gradients exactly zero, bias
corrections distinct per slot, a learning rate per tensor).  Every buffer of a launch lies in one byte image with 256 sentinel bytes on each side
(adam_ref.Arena); the device gets the image and hands it back, and adam_ref.check_launch asserts on the bytes:
  (a) p', m', v' within adam_f64's per-element bound (rounding counts C_M = 4, C_V = 7, C_U = 10, derived in adam_ref's docstring);
  (b) p', m', v' bit-equal to adam_f32, the float32 restatement (no contraction, correctly rounded divide and sqrt);
  (c) the plain fp16 shadow is half(p') of the device's own p', packed column 0 is p', the packed half pair is half(p') -- in every copy of a
      packed table the peer form writes;
  (d) every sentinel byte, and every byte of a buffer the step does not own, is unchanged;
  (e) a clear_grad gradient is zero afterwards, any other gradient unchanged;
  (f) with found_inf = 1 the image is unchanged but for the clear_grad gradients, which are zero.
The bookkeeping: scale, growth tracker, flag and step counts exactly as adam_ref.scaler_ref, the next step's bias corrections to 1 ulp (the
device's pow may differ from the host's in the last place of the double), the loss value within adam_ref.loss_ref's bound, loss_sum accumulated,
the stand-alone launch and the optimizer pass's tail bit-identical, the ticket words zero."""
import ctypes

import numpy as np
import pytest

import adam_ref as R

pytestmark = pytest.mark.gpu

f32 = np.float32
LAUNCHES = {la.name: la for la in R.single_tensor_launches() + R.packed_mode_launches() + R.paired_launches() + [R.sixteen_launch()]}
PEER = {la.name: la for la in R.peer_launches()}


def _get(img, la, name, dtype=f32):
    start, b = la.arena.regions[name]
    return R.view(img, start, dtype, b.size // np.dtype(dtype).itemsize)


def _image(la, found_inf=0.0):
    img = la.arena.image()
    _get(img, la, "found_inf")[:] = found_inf
    return img


def _desc(la, base):
    from nerf2mesh_amd import _lib as L
    ar, d = la.arena, L.AdamDesc()
    for k, t in enumerate(la.tensors):
        at = lambda key: base + ar.start(f"{t['name']}.{key}")
        d.param[k], d.grad[k], d.exp_avg[k], d.exp_avg_sq[k] = at("p"), at("g"), at("m"), at("v")
        d.numel[k], d.lr[k], d.grad_is_half[k], d.clear_grad[k], d.slot[k] = t["n"], t["lr"], int(t["g_half"]), int(t["clear"]), t["slot"]
        if t["mode"] == 1:
            d.half_shadow[k], d.shadow_mode[k] = at("shadow"), 1
        elif t["mode"] in (2, 3):
            region, off, _ = la.tables[t["table"]]
            d.half_shadow[k], d.shadow_mode[k] = base + ar.start(region) + off, t["mode"]
        else:
            d.half_shadow[k], d.shadow_mode[k] = None, 0
    d.count = len(la.tensors)
    return d


def _peer(la, base):
    from nerf2mesh_amd import _lib as L
    ap = L.AdamPeer()
    ap.world, ap.n_remote = la.world, la.n_remote
    for k, t in enumerate(la.tensors):
        if t["slots"] is not None:
            for w in range(la.world):
                ap.slots[k][w] = base + la.arena.start(f"{t['name']}.slot{w}")
    ap.packed_local = base + la.arena.start("packed_local")
    for r in range(la.n_remote):
        ap.packed_remote[r] = base + la.arena.start(f"packed_remote{r}")
    return ap


def _tail(la, base, participants, loss, ticket):
    from nerf2mesh_amd import _lib as L
    at = lambda name: base + la.arena.start(name)
    growth, backoff, interval = R.GROWTH
    if loss is None:
        return L.ScalerTail(at("tracker"), at("steps"), participants, growth, backoff, interval, None, 0, 0, None, None, None, 0, 0.0, None, 0, 0.0,
                            at("ticket") if ticket else None)
    return L.ScalerTail(at("tracker"), at("steps"), participants, growth, backoff, interval, at("part"), len(loss["part"]), loss["n_rays"], at("loss"),
                        at("loss_sum"), at("extra"), len(loss["extra"]), loss["extra_scale"], at("extra2"), len(loss["extra2"]), loss["extra2_scale"],
                        at("ticket") if ticket else None)


def _run(la, before, form="plain", participants=0, loss=None):
    """One call (form "two": n2m_adam_step, then n2m_scaler_update_slots) on a copy of the image; returns the image afterwards."""
    import torch
    from nerf2mesh_amd import _lib as L
    dev = torch.from_numpy(before).cuda()
    base = dev.data_ptr()
    assert base % 256 == 0
    at = lambda name: base + la.arena.start(name)
    scale = at("scale") if la.scale is not None else None
    args = (R.BETA1, R.BETA2, la.eps, scale, at("found_inf"), at("bias"))
    if la.tensors and form != "book":
        d = _desc(la, base)
        if form == "peer":
            ap = _peer(la, base)
            L.call("n2m_adam_step_peer", ctypes.addressof(d), *args, ctypes.addressof(ap), L.stream())
        elif form == "tail":
            tail = _tail(la, base, participants, loss, True)
            L.call("n2m_adam_step_scaler", ctypes.addressof(d), *args, ctypes.addressof(tail), L.stream())
        else:
            L.call("n2m_adam_step", ctypes.addressof(d), *args, L.stream())
    if form in ("two", "book"):
        tail = _tail(la, base, participants, loss, False)
        L.call("n2m_scaler_update_slots", scale, at("found_inf"), at("bias"), R.BETA1, R.BETA2, ctypes.addressof(tail), L.stream())
    torch.cuda.synchronize()
    return dev.cpu().numpy()


def _report(name, worst):
    print(f"{name}: largest error / bound  p {worst['p']:.3f}  m {worst['m']:.3f}  v {worst['v']:.3f}")


@pytest.mark.parametrize("name", sorted(LAUNCHES))
def test_one_step_per_element(name):
    la = LAUNCHES[name]
    before = _image(la)
    _report(name, R.check_launch(la, before, _run(la, before)))
    before = _image(la, found_inf=1.0)
    R.check_launch(la, before, _run(la, before), skip=True)


@pytest.mark.parametrize("name", sorted(PEER))
def test_one_step_of_the_peer_form_per_element(name):
    """The slot sum inside the gradient load (rank order, fp16 rounded once) and the paired packed rows in the local table and every "remote" one."""
    la = PEER[name]
    before = _image(la)
    after = _run(la, before, "peer")
    _report(name, R.check_launch(la, before, after))
    for r in range(la.n_remote):
        assert np.array_equal(_get(after, la, f"packed_remote{r}", np.uint8), _get(after, la, "packed_local", np.uint8))
    assert not np.array_equal(_get(after, la, "packed_local", np.uint8), _get(before, la, "packed_local", np.uint8))
    before = _image(la, found_inf=1.0)
    R.check_launch(la, before, _run(la, before, "peer"), skip=True)


# ------------------------------------------------------------------------------------------------ bookkeeping
def _with_book(la, loss=None, scale=None, tracker=0.0, steps=None):
    """The bookkeeping's buffers behind a launch's own: growth tracker, step counts, ticket words, the three lists of partials, the loss value and
    its running sum."""
    ar = la.arena
    ar.add("tracker", np.array([tracker], f32))
    ar.add("steps", np.asarray([0.0] * (1 + R.ADAM_MAX) if steps is None else steps, f32))
    ar.add("ticket", np.zeros(R.TICKET_WORDS, np.uint32))
    if loss is not None:
        for key in ("part", "extra", "extra2"):
            ar.add(key, loss[key])
        ar.add("loss", np.array([777.0], f32))
        ar.add("loss_sum", np.array([loss["loss_sum"]], f32))
    return la


def _book_state(la, before, after, participants, loss):
    """What the bookkeeping must leave, for check_launch: exact where the model is exact, the device's own value where a bound applies (bias
    corrections to 1 ulp, the loss value to loss_ref's bound) -- asserted here."""
    growth, backoff, interval = R.GROWTH
    scale0 = _get(before, la, "scale")[0] if la.scale is not None else None
    scale, tracker, found, steps, bias = R.scaler_ref(scale0, _get(before, la, "tracker")[0], _get(before, la, "found_inf")[0], _get(before, la, "steps"),
                                                      participants, growth, backoff, interval)
    got_bias = _get(after, la, "bias").copy()
    ulps = R.ulps_f32(got_bias, bias.reshape(-1))
    assert ulps.max() <= 1, f"{la.name}: bias corrections {int(ulps.max())} ulp from the double evaluation, entry {int(ulps.argmax())}"
    state = dict(tracker=np.array([tracker], f32), found_inf=np.zeros(1, f32), steps=np.asarray(steps, f32), bias=got_bias)
    if scale is not None:
        state["scale"] = np.array([scale], f32)
    if loss is not None:
        value, bound = R.loss_ref(loss["part"], loss["n_rays"], loss["extra"], loss["extra_scale"], loss["extra2"], loss["extra2_scale"])
        tight = R.loss_bound_in_kernel_order(loss["part"], loss["n_rays"], loss["extra"], loss["extra_scale"], loss["extra2"], loss["extra2_scale"])
        got = _get(after, la, "loss")[0]
        print(f"{la.name}: loss value {got!r} model {value!r}: error {abs(float(got) - value):.3e}, bound {bound:.3e}, in the kernel's order {tight:.3e}")
        assert abs(float(got) - value) <= bound, (float(got), value, bound)
        assert abs(float(got) - value) <= tight, (float(got), value, tight)
        state["loss"] = np.array([got], f32)
        state["loss_sum"] = np.array([f32(loss["loss_sum"]) + got], f32)
    return state


@pytest.mark.parametrize("found_inf", [0.0, 1.0])
def test_sixteen_tensors_with_the_scaler_tail(found_inf):
    """n2m_adam_step_scaler on the sixteen-tensor launch: the outputs of (a)-(f), the bookkeeping of the step, the ticket words zero."""
    loss = R.loss_cases()[4]
    la = _with_book(R.sixteen_launch(), loss, tracker=2.0, steps=np.arange(17) % 5)
    participants = 0b1010101010101011
    before = _image(la, found_inf)
    after = _run(la, before, "tail", participants, loss)
    state = _book_state(la, before, after, participants, loss)
    R.check_launch(la, before, after, skip=found_inf != 0.0, state=state)
    assert not _get(after, la, "ticket", np.uint32).any()
    assert _get(after, la, "scale")[0] == (f32(3.0) * f32(0.5) if found_inf else f32(3.0) * f32(2.0))


@pytest.mark.parametrize("case", range(len(R.COUNTS)))
def test_bookkeeping_sums(case):
    """The three sums at 1 ... 4500 partials (the stand-alone kernel strides by 256, the one-wave form walks chunks of 2048), different counts
    in one call: the value within the bound, loss_sum accumulated, and the stand-alone launch, the two launches and the tail in identical bits."""
    loss = R.loss_cases()[case]
    images = {}
    for form in ("book", "two", "tail"):
        la = _with_book(R.small_launch(), loss, tracker=1.0)
        before = _image(la)
        after = images[form] = _run(la, before, form, 0b1, loss)
        state = _book_state(la, before, after, 0b1, loss)
        if form == "book":           # the bookkeeping alone: the tensor is not stepped
            want = before.copy()
            for name, values in state.items():
                _get(want, la, name, np.uint8)[:] = np.ascontiguousarray(values).view(np.uint8).reshape(-1)
            bad = np.flatnonzero(after != want)
            assert bad.size == 0, la.arena.where(int(bad[0]))
        else:
            R.check_launch(la, before, after, state=state)
    assert np.array_equal(images["two"], images["tail"]), "n2m_adam_step + n2m_scaler_update_slots and n2m_adam_step_scaler"
    for name in ("loss", "loss_sum", "bias", "scale", "tracker", "steps", "found_inf"):
        assert np.array_equal(_get(images["book"], la, name, np.uint8), _get(images["two"], la, name, np.uint8)), name


@pytest.mark.parametrize("form", ["book", "tail"])
def test_bookkeeping_follows_the_script(form):
    """Clean steps, an overflow, growth reached, a scale of 2e38 at a growth step (it stays; the tracker resets), slots that join late and one
    that sits a step out, the back-off of a non-power-of-two scale: every word of the state after every step."""
    growth, backoff, interval = R.GROWTH
    cur = dict(scale=f32(65536.0), tracker=f32(0.0), steps=np.zeros(1 + R.ADAM_MAX, f32))
    seen = []
    for i, step in enumerate(R.SCRIPT):
        cur["scale"], cur["tracker"] = f32(step.get("scale", cur["scale"])), f32(step.get("tracker", cur["tracker"]))
        la = _with_book(R.small_launch(seed=460 + i, zero_grad=float(cur["scale"]) > 1e30), None, tracker=cur["tracker"], steps=cur["steps"])
        la.name = f"script step {i}"
        before = _image(la, step["flag"])
        _get(before, la, "scale")[:] = cur["scale"]
        if form == "tail":
            la.scale = float(cur["scale"])          # the tensor's step divides by the scale of the image
            loss = dict(part=np.ones(3, f32), extra=np.ones(1, f32), extra2=np.ones(2, f32), n_rays=4, extra_scale=0.5, extra2_scale=0.25, loss_sum=f32(0))
            for key in ("part", "extra", "extra2"):
                la.arena.add(key, loss[key])
            la.arena.add("loss", np.zeros(1, f32))
            la.arena.add("loss_sum", np.zeros(1, f32))
            before = _image(la, step["flag"])
            _get(before, la, "scale")[:] = cur["scale"]
            after = _run(la, before, "tail", step["participants"], loss)
            state = _book_state(la, before, after, step["participants"], loss)
            R.check_launch(la, before, after, skip=step["flag"] != 0.0, state=state)
            assert not _get(after, la, "ticket", np.uint32).any()
        else:
            after = _run(la, before, "book", step["participants"], None)
            state = _book_state(la, before, after, step["participants"], None)
            for name, values in state.items():
                assert np.array_equal(_get(after, la, name, np.uint8), np.ascontiguousarray(values).view(np.uint8).reshape(-1)), (i, name, _get(after, la, name))
        cur = dict(scale=_get(after, la, "scale")[0], tracker=_get(after, la, "tracker")[0], steps=_get(after, la, "steps").copy())
        seen.append((float(cur["scale"]), float(cur["tracker"]), cur["steps"].tolist()))
    # the script did what its comments say (from the device's own words)
    assert seen[2][0] == 131072.0 and seen[3][0] == 65536.0 and seen[6][:2] == (float(f32(2.0e38)), 0.0) and seen[8][0] == 1.5
    final = seen[-1][2]
    assert final[0] == 8.0 and final[1] == 8.0 and final[2] == 7.0 and final[5] == 5.0 and final[16] == 5.0 and final[3] == 0.0
