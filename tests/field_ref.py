"""Float64 model of the fused field kernels (include/n2m_mlp.h) and a generator of inputs on which that model -- and any implementation
with fp16 operands, fp32 sums and fp16 layer outputs -- is exact whatever the order of its sums.  No GPU, no kernel of the package.

The model (`field_model`) follows the header: operands and layer outputs are rounded to fp16, sums are exact (float64), sigma = exp(.) or
the raw output (SDF head), sigmoid outputs are fp16, colour = clamp(specular + diffuse, 0, 1) evaluated on the fp16 sum.  Ties follow
torch: relu'(0) = 0, clamp passes the gradient at both bounds.

The generator (`exact_case`) draws small integers (times fixed powers of two) for everything, evaluates the model on a pool of candidate
samples and keeps those on which no rounding changes a value; it then asserts the conditions the GPU test relies on (`check_case`).
Per sample nothing depends on the other samples, so selecting samples does not change what the kept ones compute."""
import collections

import numpy as np

W_SHAPES = [(32, 19), (1, 32), (64, 35), (64, 64), (6, 64), (32, 6), (3, 32)]
W_NAMES = ["sigma0", "sigma1", "color0", "color1", "color2", "spec0", "spec1"]
R_CODES = 5                      # code rows; the last one is never named
EXACT_LIMIT = float(1 << 24)     # fp32 holds every multiple of q below 2^24 q


def f16(v):
    """Round to fp16 (nearest even, one rounding) and return float64."""
    with np.errstate(over="ignore"):
        return np.asarray(v, np.float64).astype(np.float16).astype(np.float64)


def lowbit(v):
    """Value of the lowest set bit of every element (inf for 0): all terms are multiples of the smallest one."""
    v = np.asarray(v, np.float64)
    m, e = np.frexp(v)
    mi = np.abs(np.where(np.isfinite(m), m, 0.5) * float(1 << 53)).astype(np.int64)
    lb = (mi & -mi).astype(np.float64)
    out = np.ldexp(lb, e - 53)
    return np.where(v == 0, np.inf, out)


class _Trace:
    """What the model records for `check_case`: per rounding whether it changed a value (per sample), per dot product the sum of absolute
    terms S and a lower bound q of the lowest set bit of its terms (lowbit(a b) = lowbit(a) lowbit(b) for exact products; the bound takes
    the smallest factor of either side over the whole contraction, so it is never larger than the true one)."""

    def __init__(self, M, detail):
        self.M, self.detail = M, detail
        self.inexact = {}            # name -> bool [M] (or a scalar for weights)
        self.dots = {}               # name -> (S, q) arrays of the output's shape (per-sample dots only with detail)
        self.dot_bad = {}            # name -> bool [M]: S / q >= 2^24 somewhere in the sample's row
        self.dot_ratio = {}          # name -> max S / q
        self.pre = {}                # ReLU pre-activations (detail)
        self.active = {}             # name -> mean fraction of active hidden units

    def r(self, name, v, per_sample=True):
        out = f16(v)
        bad = out != v
        self.inexact[name] = bad.reshape(bad.shape[0], -1).any(axis=1) if per_sample and bad.ndim else bad.any()
        return out

    def dot(self, name, A, B, per_sample=True):
        with np.errstate(invalid="ignore", over="ignore"):      # (an overflowing candidate is rejected by its flags, not here)
            out = A @ B
            S = np.abs(A) @ np.abs(B)
        qa = lowbit(A).min(axis=1) if A.size else np.full(A.shape[0], np.inf)
        qb = lowbit(B).min(axis=0) if B.size else np.full(B.shape[1], np.inf)
        q = qa[:, None] * qb[None, :]
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(S > 0, S / q, 0.0)
        self.dot_ratio[name] = float(ratio.max()) if ratio.size else 0.0
        if per_sample:
            self.dot_bad[name] = (ratio >= EXACT_LIMIT).any(axis=1)
        if self.detail or not per_sample:
            self.dots[name] = (S, q)
        return out

    def relu(self, name, pre):
        if self.detail:
            self.pre[name] = pre
        self.active[name] = float((pre > 0).mean()) if pre.size else 0.0
        return np.maximum(pre, 0.0)


def _sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def safe_normalize(d):
    """x / sqrt(clamp(sum x^2, 1e-20)) in fp32, the operation of the reference's safe_normalize."""
    d = np.asarray(d, np.float32)
    n = np.sqrt(np.maximum((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], np.float32(1e-20)))
    return (d / n[:, None]).astype(np.float64)


def field_model(xyz, dirs, h1, h2, w, codes=None, sample_view=None, *, shading=1, normalize_dirs=0, density=True, color=True,
                d_sigma=None, d_rgb=None, d_specular=None, spec_k=0.0, detail=True):
    """One call of n2m_field_forward[_ind][_train] and, with upstream gradients, n2m_field_backward[_ind][_train].

    Layouts are the header's: xyz [M,3], dirs [M,3], h1 [16,M], h2 [16,M,2], w the seven weights as nn.Linear stores them (w[2] is
    [64, 35+D] with codes [R,D] and sample_view [M]).  normalize_dirs bit 0: safe_normalize on load, bit 1: SDF head.  spec_k is
    spec_reg * seed of the *_train forms.  Returns a dict; `trace` holds what check_case needs."""
    xyz = np.asarray(xyz, np.float64)
    M = xyz.shape[0]
    tr = _Trace(M, detail)
    out = dict(trace=tr, M=M)
    W = [None if t is None else tr.r("w_" + n, np.asarray(t, np.float64), per_sample=False) for t, n in zip(w, W_NAMES)]
    x = tr.r("xyz", xyz)
    sdf = bool(normalize_dirs & 2)
    backward = d_sigma is not None or d_rgb is not None
    dw = [None] * 7

    if density:
        X0 = np.concatenate([x, tr.r("h1", np.asarray(h1, np.float64).T)], axis=1)                     # [M,19], nn.Linear column order
        pre0 = tr.r("s_pre0", tr.dot("s_l0", X0, W[0].T))
        H1 = tr.relu("sigma0", pre0)
        o = tr.r("s_pre1", tr.dot("s_l1", H1, W[1].T))                                                # [M,1]
        out["sigma_pre"] = o[:, 0]
        out["sigma"] = o[:, 0] if sdf else np.exp(o[:, 0])
        if d_sigma is not None:
            ds = np.asarray(d_sigma, np.float64)[:, None]
            if sdf:
                dy1 = tr.r("s_dy1", ds)
            else:   # trunc_exp backward: g * exp(clamp(x, -15, 15)); the one inexact rounding of the NeRF head
                dy1 = tr.r("s_dy1_nerf", ds * np.exp(np.clip(o, -15.0, 15.0)))
            sfx = "" if sdf else "_nerf"
            dw[1] = tr.dot("dw_sigma1" + sfx, dy1.T, H1, per_sample=False)
            with np.errstate(invalid="ignore"):
                dy0 = tr.r("s_dy0" + sfx, tr.dot("s_b1" + sfx, dy1, W[1])) * (H1 > 0)
            dw[0] = tr.dot("dw_sigma0" + sfx, dy0.T, X0, per_sample=False)
            dx = tr.r("s_dx" + sfx, tr.dot("s_b0" + sfx, dy0, W[0]))
            out["d_h1"] = np.ascontiguousarray(dx[:, 3:].T)
            # the density gradients as (an integer per element) x dy1: W1 and the mask are all that lies between
            unit = W[1] * (H1 > 0)
            out["density_int_h1"] = (unit @ W[0])[:, 3:].T
            out["dy_sigma"] = dy1[:, 0]

    if color:
        D = 0 if codes is None else np.asarray(codes).shape[1]
        cols = [x, tr.r("h2", np.asarray(h2, np.float64).transpose(1, 0, 2).reshape(M, 32))]
        if D:
            cd = tr.r("codes", np.asarray(codes, np.float64), per_sample=False)
            view = np.zeros(M, np.int64) if sample_view is None else np.clip(np.asarray(sample_view, np.int64), 0, cd.shape[0] - 1)
            cols.append(cd[view])
        X0 = np.concatenate(cols, axis=1)                                                             # [M, 35 + D]
        c1 = tr.relu("color0", tr.r("c_pre0", tr.dot("c_l0", X0, W[2].T)))
        c2 = tr.relu("color1", tr.r("c_pre1", tr.dot("c_l1", c1, W[3].T)))
        pre3 = tr.r("c_pre2", tr.dot("c_l2", c2, W[4].T))                                             # [M,6]
        geo = tr.r("geo", _sigmoid(pre3))
        out["geo_pre"], out["geo"] = pre3, geo
        diffuse = geo[:, :3]
        spec = None
        if shading != 0:
            d = np.asarray(dirs, np.float64)
            if normalize_dirs & 1:
                d = safe_normalize(d)
            Pin = np.concatenate([tr.r("dirs", d), geo[:, 3:]], axis=1)                              # [M,6]
            p1 = tr.relu("spec0", tr.r("p_pre0", tr.dot("p_l0", Pin, W[5].T)))
            ppre = tr.r("p_pre1", tr.dot("p_l1", p1, W[6].T))
            spec = tr.r("spec", _sigmoid(ppre))
            out["spec_pre"] = ppre
            out["specular"] = spec
            out["spec_sq"] = float((spec * spec).sum())
        if shading == 0:
            rgb = diffuse
        elif shading == 2:
            rgb = spec
        else:
            t = tr.r("clamp_sum", spec + diffuse)
            out["clamp_sum"] = t
            rgb = np.clip(t, 0.0, 1.0)
        out["rgb"] = rgb
        if d_rgb is not None:
            g = np.asarray(d_rgb, np.float64)
            dq = np.zeros((M, 6))
            if shading == 0:
                dq[:, :3] = g
            else:
                ts = (np.zeros((M, 3)) if d_specular is None else np.asarray(d_specular, np.float64)) + spec * spec_k
                if shading == 2:
                    ts = ts + g
                else:
                    pg = g * ((t >= 0.0) & (t <= 1.0))
                    ts = ts + pg
                    dq[:, :3] = pg
                dsp = tr.r("p_dy1", ts * spec * (1.0 - spec))
                out["dsp"] = dsp
                dw[6] = tr.dot("dw_spec1", dsp.T, p1, per_sample=False)
                dyp = tr.r("p_dy0", tr.dot("p_b1", dsp, W[6])) * (p1 > 0)
                dw[5] = tr.dot("dw_spec0", dyp.T, Pin, per_sample=False)
                dxp = tr.r("p_dx", tr.dot("p_b0", dyp, W[5]))
                dq[:, 3:] = dxp[:, 3:]
            dc = tr.r("c_dy2", dq * geo * (1.0 - geo))
            out["dc"] = dc
            dw[4] = tr.dot("dw_color2", dc.T, c2, per_sample=False)
            dy2 = tr.r("c_dy1", tr.dot("c_b2", dc, W[4])) * (c2 > 0)
            dw[3] = tr.dot("dw_color1", dy2.T, c1, per_sample=False)
            dy1 = tr.r("c_dy0", tr.dot("c_b1", dy2, W[3])) * (c1 > 0)
            dw[2] = tr.dot("dw_color0", dy1.T, X0, per_sample=False)
            dx = tr.r("c_dx", tr.dot("c_b0", dy1, W[2]))
            out["d_h2"] = np.ascontiguousarray(dx[:, 3:35].reshape(M, 16, 2).transpose(1, 0, 2))
            if D:
                out["d_code_rows"] = dx[:, 35:]
                dcodes = np.zeros_like(cd)
                np.add.at(dcodes, view, dx[:, 35:])
                out["d_codes"] = dcodes
                S = np.zeros_like(cd)
                np.add.at(S, view, np.abs(dx[:, 35:]))
                q = lowbit(dx[:, 35:]).min() if dx[:, 35:].size else np.inf
                tr.dots["d_codes"] = (S, np.full_like(S, q))
                tr.dot_ratio["d_codes"] = float((S / q).max()) if np.isfinite(q) else 0.0
    if backward:
        out["dw"] = dw
    return out


# ------------------------------------------------------------------------------------------------------------------------ variants
Variant = collections.namedtuple("Variant", "density color shading sdf raw_dirs train D")


def variant_id(v):
    what = "full" if v.density and v.color else ("color" if v.color else "density")
    return f"{what}-sh{v.shading}-{'sdf' if v.sdf else 'nerf'}-{'raw' if v.raw_dirs else 'unit'}-{'train' if v.train else 'plain'}-D{v.D}"


def all_variants():
    """{density + colour, colour-only, density-only} x shading x head x dirs x {plain, train} x codes, wherever a factor applies: the head
    only with the density branch, directions and the training form only with a specular branch, codes only with the colour branch."""
    out = []
    for sdf in (False, True):
        out.append(Variant(True, False, 0, sdf, False, False, 0))
    for density in (True, False):
        for sdf in ((False, True) if density else (False,)):
            for shading in (0, 1, 2):
                for raw in ((False, True) if shading else (False,)):
                    for train in ((False, True) if shading else (False,)):
                        for D in (0, 1, 16):
                            out.append(Variant(density, True, shading, sdf, raw, train, D))
    return out


SMALL_MS = [1, 31, 32, 33, 127, 128, 129, 257]
LARGE_MS = [32768 + 33, 65536 + 33]       # the backward's 256 x 4 tiles and the forward's 512 x 4 waves wrap
FULL = Variant(True, True, 1, False, False, False, 0)
SPEC_K = 0.125                            # spec_reg * seed of the training forms: 2^-5 on the host, seed 4
SPEC_REG, SEED = 2.0 ** -5, 4.0


def gpu_cases():
    """Every (M, variant) tests/test_field_exact_gpu.py runs as an exact case."""
    cases = [(M, v) for v in all_variants() for M in SMALL_MS]
    for M in LARGE_MS:
        cases += [(M, FULL), (M, FULL._replace(sdf=True))]
    return cases


# ----------------------------------------------------------------------------------------------------------------------- generator
def _sparse(rng, shape, values, density):
    return rng.choice(np.asarray(values, np.float64), size=shape) * (rng.random(shape) < density)


def _cover(rng, W, unit, row_min, col_min):
    """At least row_min nonzeros in every row and col_min in every column (+-unit where one is missing): no dead unit, no dead input."""
    for axis, need in ((1, row_min), (0, col_min)):
        V = W if axis == 1 else W.T
        for line in V:
            while (line != 0).sum() < min(need, line.size):
                line[rng.choice(np.nonzero(line == 0)[0])] = unit * rng.choice([-1.0, 1.0])
    return W


def _weights(rng, D):
    """Small integers, sparse.  sigma_net's output layer: zero or +-1, +-2 (powers of two).  color_net's output layer: diffuse rows
    multiples of 1024, feature rows multiples of 64; specular_net's output layer multiples of 64 and its feature columns even, so every
    sigmoid pre-activation is 0 or at least 64 in magnitude (sigmoid exactly 0, 0.5 or 1 in fp16 and in fp32).  The larger diffuse rows
    keep the two gradient paths that meet in color_net (straight from the colour, and through specular_net and the features) within a few
    binades of each other, so their sums fit fp16's eleven bits."""
    half = lambda unit: _cover(rng, _sparse(rng, (3, 64), [-unit, unit], 0.3), unit, 8, 1)
    w = [_cover(rng, _sparse(rng, (32, 19), [-2, -1, 1, 2], 0.15), 1, 2, 3),
         rng.choice(np.array([-2.0, -1, -1, -1, 1, 1, 1, 2]), (1, 32)),
         _cover(rng, _sparse(rng, (64, 35 + D), [-1, 1], 0.09), 1, 2, 3),
         _cover(rng, _sparse(rng, (64, 64), [-1, 1], 0.05), 1, 2, 2),
         np.concatenate([half(1024), half(64)]),
         np.concatenate([_cover(rng, _sparse(rng, (32, 3), [-2, -1, 1, 2], 0.5), 1, 1, 8),
                         _cover(rng, _sparse(rng, (32, 3), [-2, 2], 0.6), 2, 1, 8)], axis=1),
         _cover(rng, _sparse(rng, (3, 32), [-64, 64], 0.5), 64, 6, 2)]
    return w


AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
RAW_SCALES = np.array([2.0, 3.0, 0.5])


def _pool(rng, P, v):
    """P candidate samples.  xyz and h1 are non-negative: with d_sigma > 0 under the NeRF head every term of a sigma_net weight gradient
    then has the sign of its weight, and the one inexact factor (the fp16 rounding of d_sigma exp(pre)) cannot be amplified by cancellation."""
    c = dict(xyz=rng.integers(0, 3, (P, 3)).astype(np.float64) * (rng.random((P, 3)) < 0.6),
             h1=rng.integers(1, 4, (16, P)).astype(np.float64) * (rng.random((16, P)) < 0.45),
             h2=rng.integers(-2, 3, (16, P, 2)).astype(np.float64) * (rng.random((16, P, 2)) < 0.5))
    d = AXES[rng.integers(0, 6, P)]
    if v.raw_dirs:
        d = d * RAW_SCALES[rng.integers(0, 3, P)][:, None]
    zero = rng.random(P) < 0.1                                   # candidates for the one all-zero direction
    c["dirs"], c["zero_dir"] = d * ~zero[:, None], zero
    c["view"] = rng.integers(0, R_CODES - 1, P).astype(np.int32)
    if v.sdf:
        c["d_sigma"] = rng.choice([-4.0, -2.0, -1.0, 1.0, 2.0, 4.0], P)
    else:
        c["d_sigma"] = rng.choice([0.25, 0.5, 1.0], P)           # powers of two; d_sigma exp(+-8) stays a normal fp16 number
    c["d_rgb"] = rng.integers(-3, 4, (P, 3)).astype(np.float64) / 16.0
    c["d_spec"] = rng.integers(-2, 3, (P, 3)).astype(np.float64) / 16.0
    return c


def _model_of(c, w, codes, v, idx=None, detail=True):
    take = (lambda a, ax=0: a) if idx is None else (lambda a, ax=0: np.take(a, idx, axis=ax))
    return field_model(take(c["xyz"]), take(c["dirs"]), take(c["h1"], 1), take(c["h2"], 1), w, codes if v.D else None,
                       take(c["view"]) if v.D else None, shading=v.shading, normalize_dirs=(1 if v.raw_dirs else 0) | (2 if v.sdf else 0),
                       density=v.density, color=v.color, d_sigma=take(c["d_sigma"]) if v.density else None,
                       d_rgb=take(c["d_rgb"]) if v.color else None,
                       d_specular=take(c["d_spec"]) if (v.color and v.shading and not v.train) else None,
                       spec_k=SPEC_K if v.train else 0.0, detail=detail)


# roundings that are not identities by design: the NeRF head's exp(pre) and what it multiplies (condition 8), and the sigmoids, whose
# float64 value at -64 is 1.6e-28 where fp32 and fp16 give 0 (condition 4 pins their results to 0, 0.5 and 1 instead)
INEXACT_BY_DESIGN = ("s_dy1_nerf", "s_dy0_nerf", "s_dx_nerf", "geo", "spec")


def _sample_flags(m, v):
    """Per candidate: `ok` (no rounding changed a value, every dot product exact in fp32, sigma pre-activation an integer in [-8, 8]) and
    `alive` (nonzero d_h1 column / nonzero d_h2 entry)."""
    tr, M = m["trace"], m["M"]
    ok = np.ones(M, bool)
    for k, bad in tr.inexact.items():
        if k not in INEXACT_BY_DESIGN and np.ndim(bad):
            ok &= ~bad
    for k, bad in tr.dot_bad.items():
        ok &= ~bad
    alive = np.ones(M, bool)
    if v.density:
        pre = m["sigma_pre"]
        if not v.sdf:
            ok &= (np.abs(pre) <= 8) & (pre == np.round(pre))
            ok &= np.isfinite(m["d_h1"]).all(axis=0)
        ok &= (m["d_h1"] != 0).any(axis=0)
    if v.color:
        alive = (m["d_h2"] != 0).any(axis=(0, 2))
    return ok, alive


# the weight draw per variant: the first salt in 0, 1, 2, ... whose cases meet every condition of check_case at every M of the GPU test
# (0 where no entry; found by running exactly that search)
WEIGHT_SALT = {"full-sh2-nerf-unit-plain-D16": 1}
WEIGHT_SALT.update({f"{what}-sh2-{head}-{dirs}-{form}-D1": 2 for what, head in (("full", "nerf"), ("full", "sdf"), ("color", "nerf"))
                    for dirs in ("unit", "raw") for form in ("plain", "train")})
N_SMALL, N_LARGE = 257, 1031      # selected samples per variant: the small shapes are prefixes, the large ones repeat 1031 (= 7 mod 32)
_SELECTIONS = {}


def _selection(seed, v, n):
    """Weights, codes and n + 1 kept candidates of the variant in their final order, plus one kept candidate with an all-zero direction.
    Order: richest first (most sigmoid channels that pass a gradient), the four clamp ties in front, every sixteenth sample a dead one
    (zero d_h2: the kernels must write those zeros too).  A prefix of the order is therefore a case of its own."""
    key = (seed, v, n)
    if key in _SELECTIONS:
        return _SELECTIONS[key]
    rng = np.random.default_rng([seed, v.D, WEIGHT_SALT.get(variant_id(v), 0)])
    w = _weights(rng, v.D)
    codes = rng.choice([-2.0, -1.0, 1.0, 2.0], (R_CODES, max(v.D, 1)))
    rng = np.random.default_rng([seed, n, sum(map(ord, variant_id(v)))])
    spec_branch = v.color and v.shading != 0
    keep, zero_keep, dead, pools = [], [], [], []
    chunk, need = 8192, n + 1
    for _ in range(64):
        c = _pool(rng, chunk, v)
        m = _model_of(c, w, codes, v, detail=False)
        ok, alive = _sample_flags(m, v)
        t = m.get("clamp_sum")
        score = np.zeros(chunk)
        for k, weight in (("dc", 1), ("dsp", 4)):               # (samples whose specular sigmoid passes a gradient are the rare ones)
            if k in m:
                score = score + weight * (m[k] != 0).sum(axis=1)
        base = len(pools) * chunk
        pools.append(c)
        for i in np.nonzero(ok)[0]:
            if spec_branch and c["zero_dir"][i]:
                zero_keep.append(base + i)
            elif alive[i]:
                keep.append((-score[i], base + i, None if t is None else t[i]))
            else:
                dead.append(base + i)
        if len(keep) >= 2 * need and (zero_keep or not spec_branch):
            break
    assert len(keep) >= need, (variant_id(v), n, len(keep))
    keep.sort(key=lambda e: (e[0], e[1]))
    order = [k for _, k, _ in keep]
    if v.color and v.shading == 1:
        front = []
        for val in (0.0, 1.0, 1.5, 2.0):
            hit = next((k for _, k, t in keep if k not in front and (t == val).any()), None)
            if hit is not None:
                front.append(hit)
        order = front + [k for k in order if k not in front]
    sel, dead_it = [], iter(dead)
    for j, k in enumerate(order):
        if v.color and j % 16 == 15:
            dk = next(dead_it, None)
            if dk is not None:
                sel.append(dk)
        sel.append(k)
    sel = np.asarray(sel[:need] + ([zero_keep[0]] if spec_branch else []))
    axis = lambda k: 1 if k in ("h1", "h2") else 0
    c = {k: np.take(np.concatenate([p[k] for p in pools], axis=axis(k)), sel, axis=axis(k)) for k in pools[0]}
    _SELECTIONS[key] = (w, codes, c)
    return _SELECTIONS[key]


def exact_case(M, seed, variant):
    """Inputs (numpy, the header's layouts and dtypes), the model's outputs on them and the counts check_case asserts on.  Deterministic
    in (M, seed, variant)."""
    v = variant
    n = N_SMALL if M <= N_SMALL else N_LARGE
    w, codes, sel = _selection(seed, v, n)
    idx = np.arange(M) % n
    if v.color and v.shading != 0:
        z = min(M - 1, 5)                                        # exactly one all-zero direction (the eps clamp of safe_normalize)
        idx[idx == z] = n                                        # (its repeats in a large case: the spare candidate)
        idx[z] = n + 1
    c = {k: np.take(a, idx, axis=1 if k in ("h1", "h2") else 0) for k, a in sel.items()}
    m = _model_of(c, w, codes, v, detail=M <= 4096)
    case = dict(M=M, variant=v, w=w, codes=codes[:, :v.D] if v.D else None, model=m,
                xyz=c["xyz"].astype(np.float32), dirs=c["dirs"].astype(np.float32), h1=c["h1"].astype(np.float32),
                h2=c["h2"].astype(np.float16), view=c["view"].astype(np.int32) if v.D else None,
                d_sigma=c["d_sigma"].astype(np.float32) if v.density else None, d_rgb=c["d_rgb"].astype(np.float32) if v.color else None,
                d_spec=c["d_spec"].astype(np.float32) if (v.color and v.shading and not v.train) else None,
                normalize_dirs=(1 if v.raw_dirs else 0) | (2 if v.sdf else 0), spec_reg=SPEC_REG if v.train else 0.0, seed=SEED)
    case["counts"] = check_case(case)
    return case


def check_case(case):
    """Conditions 1-8 of the exact cases; returns the tie counts.  The structural conditions (1-5, 8) and "every sample has a nonzero d_h1
    column" hold at every M.  The statistical ones (6: every kind of tie present; 7: the case is alive) are asserted from M = 127 on: one
    sample cannot show four clamp ties, and 31 samples with one direction column each do not fill half of every weight gradient.  The
    smaller cases are prefixes of the 257-sample one (richest samples first), so they run the same values."""
    v, m, M = case["variant"], case["model"], case["M"]
    tr = m["trace"]
    nerf = v.density and not v.sdf
    # 1. inputs, weights, codes and upstream gradients are fp16 numbers (integers times a fixed power of two)
    for k in ("xyz", "h1", "h2", "d_sigma", "d_rgb", "d_spec"):
        if case[k] is not None:
            a = np.asarray(case[k], np.float64)
            assert np.array_equal(f16(a), a) and np.array_equal(a * 16, np.round(a * 16)), k
    for t in case["w"] + ([case["codes"]] if v.D else []):
        assert np.array_equal(f16(t), t) and np.array_equal(t, np.round(t))
    s1 = np.abs(case["w"][1][case["w"][1] != 0])
    assert np.array_equal(lowbit(s1), s1), "w_sigma1: zero or powers of two"
    # 2. no rounding of the model changes a value (but the NeRF head's exp and what it multiplies: condition 8)
    for k, bad in tr.inexact.items():
        assert k in INEXACT_BY_DESIGN or not np.any(bad), ("rounded", k)
    # 3. every dot product: sum |terms| / lowest bit of the terms < 2^24, the weight-gradient sums over all samples included
    for k, ratio in tr.dot_ratio.items():
        if k.endswith("_nerf"):
            continue
        assert ratio < EXACT_LIMIT, (k, ratio)
    counts = {}
    if v.color:
        # 4. sigmoid pre-activations are 0 or at least 40 in magnitude; the outputs are then 0, 0.5 or 1
        for k in ("geo_pre", "spec_pre"):
            if k in m:
                p = np.abs(m[k])
                assert ((p == 0) | (p >= 40)).all(), k
        for k in ("geo", "specular"):
            if k in m:
                assert np.isin(m[k], [0.0, 0.5, 1.0]).all(), k
        # 5. signed unit axes (scaled by 2, 3, 0.5 in the raw form), exactly one all-zero direction
        if v.shading != 0:
            d = np.asarray(case["dirs"], np.float64)
            nz = (d != 0).sum(axis=1)
            assert (nz <= 1).all() and int((nz == 0).sum()) == 1
            mag = np.abs(d).sum(axis=1)[nz == 1]
            assert np.isin(mag, [2.0, 3.0, 0.5] if v.raw_dirs else [1.0]).all()
            if v.raw_dirs and M >= 31:
                assert len(np.unique(mag)) == 3
    # 6. ties, counted
    if M <= 4096:
        for k, pre in tr.pre.items():
            counts["relu0_" + k] = int((pre == 0).sum())
    if v.color and v.shading == 1:
        t = m["clamp_sum"]
        for val in (0.0, 1.0, 1.5, 2.0):
            counts[f"clamp_{val}"] = int((t == val).sum())
    # 8. NeRF head: integer pre-activation in [-8, 8], d_sigma a power of two, gradients = integer x fp16(d_sigma exp(pre)), and no
    #    cancellation in the sigma_net weight gradients (|sum| == sum of |terms|)
    if v.density:
        assert (m["d_h1"] != 0).any(axis=0).all(), "7: every sample has a nonzero d_h1 column"
        assert (np.asarray(case["d_sigma"]) != 0).all()
        if nerf:
            pre = m["sigma_pre"]
            assert (np.abs(pre) <= 8).all() and np.array_equal(pre, np.round(pre))
            ds = np.asarray(case["d_sigma"], np.float64)
            assert (ds > 0).all() and np.array_equal(lowbit(ds), ds)
            k = m["density_int_h1"]
            assert np.array_equal(k, np.round(k))
            assert np.array_equal(m["d_h1"], f16(k * m["dy_sigma"][None, :]))
            dy = m["dy_sigma"]
            assert (dy >= 2.0 ** -14).all() and np.isfinite(m["d_h1"]).all(), "normal fp16 numbers, no overflow"
            for i in (0, 1):
                S = tr.dots["dw_" + W_NAMES[i] + "_nerf"][0]
                assert np.array_equal(np.abs(m["dw"][i]), S), "no cancellation"
    if M < 127:      # (the one sample of M = 1 under a specular branch is the all-zero direction, alive or not)
        return counts
    # 6 (presence) and 7 (alive)
    if M <= 4096:
        for k in tr.pre:
            assert counts["relu0_" + k] > 0, ("no ReLU tie", k)
    if v.color and v.shading == 1:
        for val in (0.0, 1.0, 1.5, 2.0):
            assert counts[f"clamp_{val}"] > 0, ("no clamp tie", val)
    for k, frac in tr.active.items():
        assert frac >= 0.25, ("active", k, frac)
    if v.density:
        assert (m["d_h1"] != 0).any(axis=1).all(), "a d_h1 row is all zero"
    if v.color:
        assert (m["d_h2"] != 0).any(axis=1).all(), "a d_h2 row is all zero"
        assert (m["d_h2"] != 0).any(axis=(0, 2)).mean() >= 0.9
    for i, t in enumerate(m["dw"]):
        if t is not None:
            if i == 4 and v.shading != 1:      # rows of d W_color2 no gradient reaches in any implementation: features under diffuse
                t = t[:3] if v.shading == 0 else t[3:]      # shading, diffuse colours under specular shading
            assert (t != 0).mean() >= 0.5, ("dW mostly zero", W_NAMES[i], float((t != 0).mean()))
    if v.D:
        assert not m["d_codes"][R_CODES - 1].any() and m["d_codes"][:R_CODES - 1].any()
        assert (m["dw"][2][:, 35:] != 0).mean() >= 0.5
    return counts
