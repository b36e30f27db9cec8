"""A per-element model of the fused optimizer pass (adam_body, csrc/step_helpers.hip: n2m_adam_step / n2m_adam_step_scaler / n2m_adam_step_peer) and
of the one-workgroup bookkeeping behind it (scaler_update_slots_body: n2m_scaler_update_slots and the tail of n2m_adam_step_scaler), and the inputs
("launches") that the CPU and GPU tests of those kernels share.  No GPU and no ctypes here: tests/test_adam_ref_cpu.py pins the model to
torch.optim.Adam and torch.amp.GradScaler, tests/test_adam_exact_gpu.py runs the kernels on the launches and hands the bytes to check_launch.

One step of one element, as the kernel states it (float32, no contraction, correctly rounded divide and sqrt):
    inv = 1 / scale          gr = g * inv             step = lr / bc1
    m' = b1 m + omb1 gr      v' = b2 v + (omb2 gr) gr           (omb = float32(1 - beta), the subtraction in double)
    denom = sqrt(v') / bc2 + eps                      p' = p - (step m') / denom
adam_f32 is that statement in numpy float32, rounding for rounding; adam_f64 evaluates it in float64 on the same float32 / float16 inputs and
returns a bound on what ANY float32 evaluation with those rounding points can differ from it by.

The bound counts roundings.  u = 2^-24; a product of k factors (1 + d)^(+-1), |d| <= u, is 1 + t with |t| <= gamma(k) = k u / (1 - k u) (Higham,
Accuracy and Stability, lemma 3.1), so a count of k gives gamma(k), nothing is added to it.
    C_M = 4   m' = b1 m (1 + t2) + omb1 gr (1 + t4): {b1 m, the add} and {1 / scale, g inv, omb1 gr, the add}.  Relative to |b1 m| + |omb1 gr|,
              not to m': the two terms can cancel.
    C_V = 7   v' = b2 v (1 + t2) + omb2 gr^2 (1 + t7): gr carries 2 roundings and enters twice (4), omb2 gr (1), (.) gr (1), the add (1); both
              terms are >= 0, so the bound is relative to v'.
    C_U = 10  the update U = step m' / denom apart from m's own error: step (1), step m' (1), the divide (1), and denom's 7: sqrt halves v's 7
              (3.5, counted as 4), the sqrt (1), / bc2 (1), + eps (1; sqrt / bc2 and eps are both > 0).
    |dp'| <= u (|p'| + |dU|) + |dU|,   |dU| <= gamma(10) |U| + (1 + gamma(10)) (step / denom) |dm'|
(the float64 evaluation's own error, 1e-16 relative, is nine orders below u.)"""
import math

import numpy as np

U = 2.0 ** -24
C_M, C_V, C_U = 4, 7, 10
ADAM_MAX = 16
BETA1, BETA2 = 0.9, 0.999
F32_MIN_NORMAL = 2.0 ** -126
PAD = 256                      # bytes of sentinel on each side of every buffer: 64 float32 / 128 float16 elements
SENTINEL = 0xA5
TICKET_WORDS = 64 * 32         # N2M_TAIL_TICKET_WORDS
f32 = np.float32


def gamma(k):
    return k * U / (1.0 - k * U)


def omb(beta):
    """float32(1 - beta) with the subtraction in double: what the host hands the kernel."""
    return f32(1.0 - float(beta))


def bias_pair(beta1, beta2, t):
    """The bias corrections of step t as the bookkeeping leaves them: double arithmetic, rounded to float."""
    return f32(1.0 - float(beta1) ** float(t)), f32(math.sqrt(1.0 - float(beta2) ** float(t)))


def slot_sum(slots, half):
    """The peer form's gradient: the rank-order float32 sum of the W slots from 0.0f, rounded to half ONCE when the gradient is fp16.
    Returns float32 values."""
    a = np.zeros(slots.shape[1], f32)
    for s in slots:
        a = a + s.astype(f32)
    return a.astype(np.float16).astype(f32) if half else a


def adam_f32(p, m, v, g, scale, bc1, bc2, lr, eps, beta1=BETA1, beta2=BETA2, detail=False):
    """One step in numpy float32 with the kernel's association and rounding points; no fused multiply-add (numpy has none).
    `g` float32 or float16 (converted exactly); scale None: no loss scale (inv = 1).  detail=True adds every intermediate."""
    p, m, v = (np.asarray(x, f32) for x in (p, m, v))
    g = np.asarray(g).astype(f32)
    b1, b2, o1, o2 = f32(beta1), f32(beta2), omb(beta1), omb(beta2)
    inv = f32(1.0) / f32(scale) if scale is not None else f32(1.0)
    step = f32(lr) / f32(bc1)
    gr = g * inv
    b1m, o1g = b1 * m, o1 * gr
    m2 = b1m + o1g
    b2v, o2g = b2 * v, o2 * gr
    o2gg = o2g * gr
    v2 = b2v + o2gg
    sq = np.sqrt(v2)
    sqb = sq / f32(bc2)
    den = sqb + f32(eps)
    sm = step * m2
    upd = sm / den
    p2 = p - upd
    out = dict(p=p2, m=m2, v=v2)
    assert all(x.dtype == np.float32 for x in out.values())
    if detail:
        out.update(inv=inv, step=step, gr=gr, b1m=b1m, o1g=o1g, b2v=b2v, o2g=o2g, o2gg=o2gg, sq=sq, sqb=sqb, den=den, sm=sm, upd=upd)
    return out


def adam_f64(p, m, v, g, scale, bc1, bc2, lr, eps, beta1=BETA1, beta2=BETA2):
    """The same step in float64 on the values the kernel reads, and the per-element bounds bp, bm, bv (module docstring)."""
    p, m, v, g = (np.asarray(x).astype(np.float64) for x in (p, m, v, g))
    b1, b2, o1, o2 = (float(x) for x in (f32(beta1), f32(beta2), omb(beta1), omb(beta2)))
    inv = 1.0 / float(f32(scale)) if scale is not None else 1.0
    step = float(f32(lr)) / float(f32(bc1))
    gr = g * inv
    A, B = b1 * m, o1 * gr
    m2 = A + B
    v2 = b2 * v + o2 * gr * gr
    den = np.sqrt(v2) / float(f32(bc2)) + float(f32(eps))
    upd = step * m2 / den
    p2 = p - upd
    bm = gamma(C_M) * (np.abs(A) + np.abs(B))
    bv = gamma(C_V) * v2
    bu = gamma(C_U) * np.abs(upd) + (1.0 + gamma(C_U)) * (step / den) * bm
    bp = U * (np.abs(p2) + bu) + bu
    return dict(p=p2, m=m2, v=v2, bp=bp, bm=bm, bv=bv, upd=upd)


def normal_or_zero(x):
    a = np.abs(np.asarray(x, np.float64))
    return bool(np.all(np.isfinite(a) & ((a == 0.0) | (a >= F32_MIN_NORMAL))))


# ------------------------------------------------------------------------------------------------ bookkeeping
def scaler_ref(scale, tracker, found_inf, steps, participants, growth, backoff, interval, beta1=BETA1, beta2=BETA2):
    """GradScaler.update() with one step count per slot, as scaler_update_slots_body does it.  scale: float32 value or None; steps: 1 + ADAM_MAX
    counts.  Returns the new (scale, tracker, found_inf, steps, bias [1 + ADAM_MAX, 2] float32)."""
    ok = float(found_inf) == 0.0
    scale = None if scale is None else f32(scale)
    tracker = None if tracker is None else f32(tracker)
    with np.errstate(over="ignore"):
        if not ok:
            if scale is not None:
                scale = scale * f32(backoff)
            if tracker is not None:
                tracker = f32(0.0)
        elif tracker is not None:
            g = tracker + f32(1.0)
            if g >= f32(interval):
                ns = scale * f32(growth)
                if ns <= f32(3.0e38):                 # do not grow into inf; the tracker resets all the same
                    scale = ns
                tracker = f32(0.0)
            else:
                tracker = g
    steps = [float(s) for s in steps]
    bias = np.zeros((1 + ADAM_MAX, 2), f32)
    for s in range(1 + ADAM_MAX):
        if ok and (s == 0 or (participants >> (s - 1)) & 1):
            steps[s] += 1.0
        bias[s] = bias_pair(beta1, beta2, steps[s] + 1.0)
    return scale, tracker, f32(0.0), steps, bias


def loss_ref(part, n_rays, extra=None, extra_scale=0.0, extra2=None, extra2_scale=0.0):
    """The step's loss value in float64 and its bound: sum(part) / n_rays + sum(extra) extra_scale + sum(extra2) extra2_scale.  Per sum of n
    partials n u sum|x| (any summation order), times its coefficient; plus 2 u on the combination (its two additions), relative to the terms'
    magnitudes.  The coefficients' own roundings (1 / n_rays, the three products) are exact when n_rays and the scales are powers of two;
    elsewhere they are four more u on a term, which the n u of a sum of n >= 63 partials covers many times: the cases below pair a sum of
    ONE partial with power-of-two coefficients."""
    value, bound, mag = 0.0, 0.0, 0.0
    for x, c in ((part, 1.0 / float(n_rays)), (extra, float(f32(extra_scale))), (extra2, float(f32(extra2_scale)))):
        if x is None:
            continue
        x = np.asarray(x, np.float64)
        value += float(x.sum()) * c
        bound += abs(c) * len(x) * U * float(np.abs(x).sum())
        mag += abs(c) * abs(float(x.sum()))
    return value, bound + 2.0 * U * mag


def loss_bound_in_kernel_order(part, n_rays, extra=None, extra_scale=0.0, extra2=None, extra2_scale=0.0):
    """A second, sharper bound for the order both forms of the bookkeeping document: a partial is added into its lane's accumulator (at most
    ceil(n / 256) additions), goes through the six levels of the wave scan and at most four additions across the waves -- a depth of
    d = ceil(n / 256) + 10, so gamma(d) sum|x| per sum whatever the tree's shape; then 1 / n_rays and its product (2), the other products (1
    each) and the two additions of the combination (2).  At 4500 partials this is 32 u against loss_ref's 4500 u."""
    bound = 0.0
    for x, c, k in ((part, 1.0 / float(n_rays), 2), (extra, float(f32(extra_scale)), 1), (extra2, float(f32(extra2_scale)), 1)):
        if x is not None:
            bound += abs(c) * gamma((len(x) + 255) // 256 + 10 + k + 2) * float(np.abs(np.asarray(x, np.float64)).sum())
    return bound


def ulps_f32(a, b):
    """Distance of two float32 arrays of one sign in units of the last place."""
    a, b = np.asarray(a, f32).view(np.int32).astype(np.int64), np.asarray(b, f32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


# ------------------------------------------------------------------------------------------------ memory image of a launch
class Arena:
    """Every buffer of a launch in ONE byte image: each at (a 256-byte boundary + PAD + its own offset), PAD sentinel bytes in front and behind.
    The device gets the image in one copy and hands it back in one; whatever the kernel wrote outside its outputs shows as a changed byte."""

    def __init__(self):
        self.regions, self.size = {}, 0

    def add(self, name, data, off=0):
        assert name not in self.regions, name
        data = np.ascontiguousarray(data)
        start = (self.size + 255) // 256 * 256 + PAD + off
        self.regions[name] = (start, data.view(np.uint8).reshape(-1).copy())
        self.size = start + data.nbytes + PAD
        return name

    def image(self):
        img = np.full((self.size + 255) // 256 * 256, SENTINEL, np.uint8)
        for start, b in self.regions.values():
            img[start:start + b.size] = b
        return img

    def start(self, name):
        return self.regions[name][0]

    def where(self, byte):
        for name, (start, b) in self.regions.items():
            if start - PAD <= byte < start + b.size + PAD:
                what = "sentinel in front of" if byte < start else ("sentinel behind" if byte >= start + b.size else "inside")
                return f"{what} {name} (byte {byte - start} of {b.size})"
        return f"byte {byte} (alignment gap)"


def view(img, start, dtype, count):
    return img[start:start + count * np.dtype(dtype).itemsize].view(dtype)


class Launch:
    """One call of n2m_adam_step / _scaler / _peer: up to 16 tensors, the step's scalars and their buffers' places in an Arena.  Every tensor has
    its own learning rate and bias slot; the bias rows are distinct per slot (step counts 1, 3, 5, ...)."""

    def __init__(self, name, seed, scale=None, eps=1e-15, world=0, n_remote=0):
        self.name, self.scale, self.eps, self.world, self.n_remote = name, scale, float(f32(eps)), world, n_remote
        self.rng = np.random.default_rng(seed)
        self.arena, self.tensors, self.tables = Arena(), [], []
        self.bias = np.array([bias_pair(BETA1, BETA2, 1 + 2 * s) for s in range(1 + ADAM_MAX)], f32)
        self.arena.add("bias", self.bias)
        self.arena.add("found_inf", np.zeros(1, f32))
        if scale is not None:
            self.arena.add("scale", np.array([scale], f32))
        self.packed = None           # peer form: every packed table of the launch lives in ONE region, mirrored by the "remote" ones

    # ---- packed tables ([rows] x 8 bytes: float32 column 0, half2 column 1), initialised with arbitrary bytes
    def table(self, rows, off=0):
        assert self.world == 0
        name = self.arena.add(f"table{len(self.tables)}", self.rng.integers(0, 256, rows * 8, dtype=np.uint8), off)
        self.tables.append((name, 0, rows))
        return len(self.tables) - 1

    def peer_tables(self, rows_list):
        """The peer form's packed tables: one 16-byte aligned region with 64 arbitrary bytes between the tables, and n_remote copies of it."""
        offs, size = [], 0
        for rows in rows_list:
            offs.append(size)
            size += rows * 8 + 64
        blob = self.rng.integers(0, 256, size, dtype=np.uint8)
        self.packed = [self.arena.add("packed_local", blob)] + [self.arena.add(f"packed_remote{r}", blob) for r in range(self.n_remote)]
        ids = []
        for rows, o in zip(rows_list, offs):
            self.tables.append(("packed_local", o, rows))
            ids.append(len(self.tables) - 1)
        return ids

    # ---- tensors
    def tensor(self, n, g_half=False, mode=0, table=None, off=0, g_off=None, s_off=0, clear=False, slots=False, partner_of=None):
        """n elements of random state: p ~ N(0, 1), m ~ 0.1 N(0, 1) and v ~ 0.01 N(0, 1)^2 + 1e-6 (never zero), unscaled gradient ~ 0.3 N(0, 1) with a
        third of the elements exactly zero.  Every intermediate of the step stays a normal float32 number or an exact zero (asserted in
        `expected`): subnormal handling is not what these cases test.  off: byte offset of p / m / v / a float32 g from 16-byte alignment (an
        int, or a dict per array); g_off: the same for the gradient alone; s_off: for a plain fp16 shadow.  slots: the gradient is the sum of
        `world` staging slots (peer form)."""
        k, rng = len(self.tensors), self.rng
        assert k < ADAM_MAX
        s = 1.0 if self.scale is None else float(self.scale)
        p = rng.standard_normal(n).astype(f32)
        m = (0.1 * rng.standard_normal(n)).astype(f32)
        m[m == 0] = f32(0.05)
        v = (0.01 * rng.standard_normal(n) ** 2 + 1e-6).astype(f32)
        zero = rng.random(n) < 1.0 / 3.0
        gd = np.float16 if g_half else f32
        lim = 60000.0                                   # fp16 gradients stay finite
        t = dict(n=n, g_half=g_half, mode=mode, table=table, clear=clear, lr=float(f32(1e-2 / (1 + 0.37 * k))), slot=(5 * k + 3) % (1 + ADAM_MAX),
                 p=p, m=m, v=v, slots=None, partner_of=partner_of, name=f"t{k}")
        if slots:
            W = self.world
            sl = 0.3 * s / W * rng.standard_normal((W, n))
            sl[:, zero] = 0.0
            t["slots"] = np.clip(sl, -lim / W, lim / W).astype(gd)
            t["g"] = slot_sum(t["slots"], g_half)
            g_mem = rng.standard_normal(n).astype(gd)    # the descriptor's own gradient pointer of a slot-fed tensor: never read, never written
        else:
            gr = 0.3 * rng.standard_normal(n)
            gr[zero] = 0.0
            t["g"] = g_mem = np.clip(gr * s, -lim, lim).astype(gd)
        offs = off if isinstance(off, dict) else dict(p=off, m=off, v=off, g=off if not g_half else 0)
        if g_off is not None:
            offs["g"] = g_off
        for key, data in (("p", p), ("m", m), ("v", v), ("g", g_mem)):
            self.arena.add(f"{t['name']}.{key}", data, offs.get(key, 0))
        if slots:
            for w in range(self.world):
                self.arena.add(f"{t['name']}.slot{w}", t["slots"][w], offs.get("g", 0))
        if mode == 1:
            self.arena.add(f"{t['name']}.shadow", rng.standard_normal(n).astype(np.float16), s_off)
        self.tensors.append(t)
        return k

    def pair(self, rows, g1_half=False, g2_half=True, off1=0, off2=0, table=None, slots1=False, slots2=False):
        """A [rows,1] tensor (mode 2) and a [rows,2] tensor (mode 3) on one 16-byte aligned packed table: the second one's threads update both."""
        table = self.table(rows) if table is None else table
        a = self.tensor(rows, g_half=g1_half, mode=2, table=table, off=off1, slots=slots1)
        b = self.tensor(2 * rows, g_half=g2_half, mode=3, table=table, off=off2, slots=slots2)
        self.tensors[a]["partner_of"] = b
        return a, b

    # ---- what the step must compute
    def tensor_args(self, t):
        bc1, bc2 = self.bias[t["slot"]]
        return dict(p=t["p"], m=t["m"], v=t["v"], g=t["g"], scale=self.scale, bc1=bc1, bc2=bc2, lr=t["lr"], eps=self.eps)

    def expected(self):
        """Per tensor the float32 restatement (with intermediates) and the float64 model.  Computed once per launch."""
        if getattr(self, "_expected", None) is not None and len(self._expected) == len(self.tensors):
            return self._expected
        out = self._expected = []
        for t in self.tensors:
            a = self.tensor_args(t)
            r32 = adam_f32(detail=True, **a)
            for key, x in r32.items():
                assert getattr(self, "zero_grad", False) or normal_or_zero(x), f"{self.name} {t['name']}: intermediate {key} leaves the normal float32 range"
            out.append((r32, adam_f64(**a)))
        return out

    # ---- the image after a step, given p', m', v' per tensor
    def apply(self, before, outputs, skip=False):
        """The bytes a correct step leaves: `outputs[k]` = dict(p, m, v) float32 goes to the tensor's arrays, half(p') to a plain shadow, p' to
        column 0 / half2(p') to column 1 of a packed table (and of its remote copies), a clear_grad gradient becomes zero -- also on a skipped
        step (skip=True), which changes nothing else."""
        img, ar = before.copy(), self.arena
        for k, t in enumerate(self.tensors):
            n = t["n"]
            if t["clear"]:
                view(img, ar.start(f"{t['name']}.g"), f32, n)[:] = 0.0
            if skip:
                continue
            o = outputs[k]
            for key in ("p", "m", "v"):
                view(img, ar.start(f"{t['name']}.{key}"), np.uint32, n)[:] = np.asarray(o[key], f32).view(np.uint32)
            ph = np.asarray(o["p"], f32).astype(np.float16)
            if t["mode"] == 1:
                view(img, ar.start(f"{t['name']}.shadow"), np.uint16, n)[:] = ph.view(np.uint16)
            elif t["mode"] in (2, 3):
                region, o_tab, rows = self.tables[t["table"]]
                for reg in ([region] if self.packed is None else self.packed):
                    rows32 = view(img, ar.start(reg) + o_tab, np.uint32, rows * 2).reshape(rows, 2)
                    if t["mode"] == 2:
                        rows32[:, 0] = np.asarray(o["p"], f32).view(np.uint32)
                    else:
                        rows32[:, 1] = ph.view(np.uint32)
        return img

    def outputs_of(self, img):
        ar = self.arena
        return [{key: view(img, ar.start(f"{t['name']}.{key}"), f32, t["n"]).copy() for key in ("p", "m", "v")} for t in self.tensors]

    def emulate(self, before, skip=False):
        """What the float32 restatement makes of the image: the CPU stand-in for the kernel."""
        return self.apply(before, [r32 for r32, _ in self.expected()], skip)


def check_launch(launch, before, after, skip=False, bits=True, state=None):
    """Checks (a)-(f) of one launch on the bytes the device handed back.  Returns the largest error-to-bound ratio per output.
    state: {region: values} that the call's bookkeeping must leave (n2m_adam_step_scaler, n2m_scaler_update_slots)."""
    worst = dict(p=0.0, m=0.0, v=0.0)
    if not skip:
        got = launch.outputs_of(after)
        for k, (t, (r32, r64)) in enumerate(zip(launch.tensors, launch.expected())):
            for key in ("m", "v", "p"):
                err, bound = np.abs(got[k][key].astype(np.float64) - r64[key]), r64["b" + key]
                bad = np.flatnonzero(~(err <= bound))
                assert bad.size == 0, (f"(a) {launch.name} {t['name']}.{key} (n={t['n']}, mode {t['mode']}, slot {t['slot']}): {bad.size} elements outside the "
                                       f"float64 bound, first {bad[0]}: got {got[k][key][bad[0]]!r} model {r64[key][bad[0]]!r} bound {bound[bad[0]]:.3e}")
                with np.errstate(divide="ignore", invalid="ignore"):
                    worst[key] = max(worst[key], float(np.max(np.where(bound > 0, err / bound, 0.0), initial=0.0)))
                if bits:
                    bad = np.flatnonzero(got[k][key].view(np.uint32) != r32[key].view(np.uint32))
                    assert bad.size == 0, (f"(b) {launch.name} {t['name']}.{key} (n={t['n']}, mode {t['mode']}): {bad.size} elements differ from the float32 "
                                           f"restatement, first {bad[0]}: got {got[k][key][bad[0]]!r} want {r32[key][bad[0]]!r}")
    want = launch.apply(before, None if skip else launch.outputs_of(after), skip)
    for name, values in (state or {}).items():
        b = np.ascontiguousarray(values).view(np.uint8).reshape(-1)
        assert b.size == launch.arena.regions[name][1].size, name
        want[launch.arena.start(name):launch.arena.start(name) + b.size] = b
    bad = np.flatnonzero(after != want)
    assert bad.size == 0, (f"(c)-(f) {launch.name}{' (skipped step)' if skip else ''}: {bad.size} bytes differ from what the step may write, first: "
                           f"{launch.arena.where(int(bad[0]))}; last: {launch.arena.where(int(bad[-1]))}")
    return worst


# ------------------------------------------------------------------------------------------------ the launches
SCALES = (None, 1.0, 65536.0, 3.0)
EPSS = (1e-15, 1e-8)
SIZES = (1, 2, 3, 4, 5, 1023, 1024, 1025, 2049)
PAIR_ROWS = (1, 2, 3, 4, 511, 512, 513, 1027)
SIXTEEN = (1, 5, 1024, 1025, 4096, 5, 1, 1025, 4096, 1024, 5, 1, 1024, 1025)      # + one pair = 16 tensors


def single_tensor_launches():
    """numel x gradient type x shadow x alignment x clear_grad, sixteen tensors to a launch; the launches walk scale x eps."""
    specs = []
    for n in SIZES:
        for shadow in (0, 1):
            for off in (0, 4, 8, 12):
                for clear in (False, True):
                    specs.append(dict(n=n, g_half=False, mode=shadow, off=off, clear=clear, s_off=4 if off in (4, 8) else 0))
                for g_off in (0, 4):
                    specs.append(dict(n=n, g_half=True, mode=shadow, off=off, g_off=g_off, s_off=4 if off in (0, 4) else 0))
    out = []
    for i in range(0, len(specs), ADAM_MAX):
        j = i // ADAM_MAX
        la = Launch(f"single{j}", 100 + j, scale=SCALES[j % 4], eps=EPSS[(j // 4) % 2])
        # (a stride of 7 through the list, so that a launch mixes sizes and types)
        for q in range(ADAM_MAX):
            la.tensor(**specs[(i + q) * 7 % len(specs)])
        out.append(la)
    assert len(specs) % ADAM_MAX == 0 and math.gcd(7, len(specs)) == 1
    return out


def packed_mode_launches():
    """Mode 2 alone and mode 3 alone (a table that no partner shares, or one at 8 mod 16), and both on one table at 8 mod 16: no paired update."""
    out = []
    for j, rows_pair in enumerate(((1, 2), (3, 1027))):
        la = Launch(f"packed{j}", 200 + j, scale=SCALES[1 + j], eps=EPSS[j])
        for rows in rows_pair:
            la.tensor(rows, mode=2, table=la.table(rows, 0), off=4 * (rows % 4))
            la.tensor(rows, mode=2, table=la.table(rows, 8))
            la.tensor(2 * rows, g_half=True, mode=3, table=la.table(rows, 8), g_off=4 * (rows % 2))
            la.tensor(2 * rows, mode=3, table=la.table(rows, 0), off=8)
            tb = la.table(rows, 8)
            la.tensor(rows, mode=2, table=tb, clear=True)
            la.tensor(2 * rows, g_half=True, mode=3, table=tb)
        out.append(la)
    return out


def paired_launches():
    """The paired update: rows x partner alignment {0, 4 bytes off 8} x partner gradient {fp32, fp16}, and two mixed alignments (only the partner's
    gradient, only its exp_avg off 8-byte alignment: the 8-byte load and the 8-byte store fall back separately)."""
    specs = [dict(rows=r, g1_half=h, off1=o) for r in PAIR_ROWS for h in (False, True) for o in (0, 4)]
    specs += [dict(rows=r, g1_half=False, off1=o) for r in (3, 513, 1027) for o in (dict(p=0, m=0, v=0, g=4), dict(p=8, m=4, v=0, g=0))]
    out = []
    for i in range(0, len(specs), 8):
        j = i // 8
        la = Launch(f"paired{j}", 300 + j, scale=SCALES[(j + 2) % 4], eps=EPSS[j % 2])
        for q, s in enumerate(specs[i:i + 8]):
            la.pair(g2_half=bool((q + j) & 1), off2=4 * ((q + j) % 4), **s)
        out.append(la)
    return out


def sixteen_launch(seed=400, scale=3.0):
    la = Launch("sixteen", seed, scale=scale, eps=1e-15)
    for q, n in enumerate(SIXTEEN[:7]):
        la.tensor(n, g_half=q % 3 == 1, mode=q % 2, off=4 * (q % 4), clear=q % 3 == 2)
    la.pair(513, g1_half=False, g2_half=True)
    for q, n in enumerate(SIXTEEN[7:]):
        la.tensor(n, g_half=q % 3 == 0, mode=(q + 1) % 2, off=4 * ((q + 1) % 4), clear=q % 3 == 1, s_off=4 * (q % 2))
    assert len(la.tensors) == ADAM_MAX
    return la


def small_launch(seed=450, zero_grad=False):
    """The least the tail needs in front of it: one tensor, one workgroup.  zero_grad: an all-zero gradient, for a step at a loss scale of 2e38
    (1 / 2e38 is subnormal; times zero it is the exact zero the cases are held to)."""
    la = Launch("small", seed, scale=65536.0, eps=1e-15)
    la.tensor(5)
    if zero_grad:
        la.zero_grad = True
        la.tensors[0]["g"][:] = 0.0
        la.arena.regions["t0.g"][1][:] = 0
    return la


def peer_launches():
    """The peer form in one device's memory: world x n_remote.  Pair A takes both gradients from slots (fp32 [rows,1], fp16 [rows,2]), pair B
    only the [rows,2] one (fp32 slots; its partner reads an fp16 gradient), pair C none (the 8-byte partner load of the plain form); a plain
    tensor takes fp32 or fp16 slots.  Rows are even: whole 16-byte packed pairs, which is all the form's store to the other tables covers."""
    out = []
    for world in (1, 2, 3):
        for n_remote in (0, 2):
            la = Launch(f"peer_w{world}_r{n_remote}", 500 + 10 * world + n_remote, scale=SCALES[world], eps=EPSS[n_remote // 2], world=world, n_remote=n_remote)
            ta, tb, tc = la.peer_tables([516, 514, 6])
            la.pair(516, g1_half=False, g2_half=True, table=ta, slots1=True, slots2=True)
            la.pair(514, g1_half=True, g2_half=False, table=tb, slots2=True)
            la.pair(6, g1_half=False, g2_half=False, table=tc)
            la.tensor(1028 if world != 2 else 8, g_half=world == 3, mode=1, slots=True)
            la.tensor(7, mode=1, clear=True, off=4)
            out.append(la)
    return out


def all_launches():
    return single_tensor_launches() + packed_mode_launches() + paired_launches() + [sixteen_launch()] + peer_launches()


# ------------------------------------------------------------------------------------------------ bookkeeping cases
COUNTS = (1, 63, 64, 255, 256, 257, 2047, 2048, 2049, 4500)
GROWTH = (2.0, 0.5, 3.0)           # growth factor, back-off factor, growth interval


def loss_cases():
    """Ten calls; the three sums take different counts in each, every count comes to every sum once.  Partials of both signs and of magnitudes
    over three decades.  A call in which one of the sums has a single partial uses power-of-two coefficients (loss_ref)."""
    rng = np.random.default_rng(600)
    out = []
    for i in range(len(COUNTS)):
        n = (COUNTS[i], COUNTS[(i + 3) % 10], COUNTS[(i + 7) % 10])
        xs = [(rng.standard_normal(c) * 10.0 ** rng.uniform(-2, 1, c)).astype(f32) for c in n]
        pow2 = 1 in n
        out.append(dict(part=xs[0], extra=xs[1], extra2=xs[2], n_rays=4096 if pow2 else 1481, extra_scale=0.25 if pow2 else 0.3,
                        extra2_scale=0.125 if pow2 else 0.07, loss_sum=f32(3.25)))
    return out


# flag, participants, and state written before the step (a scale of 2e38 one clean step short of growth)
SCRIPT = (
    dict(flag=0.0, participants=0b0011),
    dict(flag=0.0, participants=0b0011),
    dict(flag=0.0, participants=0b0011),                                # the third clean step: the scale grows
    dict(flag=1.0, participants=0b0011),                                # overflow: back-off, nobody counts
    dict(flag=0.0, participants=0b1000000000010011),                    # slots 5 and 16 join late
    dict(flag=0.0, participants=0b1000000000010011),
    dict(flag=0.0, participants=0b1000000000010011, scale=2.0e38, tracker=2.0),      # growth step at 2e38: the scale stays, the tracker resets
    dict(flag=0.0, participants=0b1000000000010001),                    # slot 2 sits one out
    dict(flag=1.0, participants=0b1000000000010011, scale=3.0),         # back-off of a non-power-of-two scale
    dict(flag=0.0, participants=0b1000000000010011),
)
