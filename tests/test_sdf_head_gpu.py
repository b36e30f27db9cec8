"""The SDF head kernels (n2m_sdf_offsets / n2m_sdf_alpha_forward / n2m_sdf_alpha_backward and the one-workgroup sum behind the backward) per
sample against the float64 model of tests/sdf_head_ref.py.  Every check is per element, never relative to a tensor's maximum:

  pts, pts01     bit-equal to the model (the same float32 expression).
  normal         relative error <= 4 * 2^-24 per entry (derived: one subtraction, exact or nearly so, one multiply by 0.5, exact, one divide;
                 the model divides by the same float32 eps); an entry below 2^-126 may be flushed to 0.
  alpha          absolute error <= KERNEL_FACTOR * yardstick.
  d_sdf, d_sdf6  |got - ref| / (|ref| + median |ref|) <= KERNEL_FACTOR * yardstick, the median over the case's ordinary samples from the model;
                 what sdf_head_ref.condition marks in a random population is left out (at most 1 %, asserted on the CPU).
  d_variance     against the float64 sum of the model's summands, see variance_bound.
  eikonal        each workgroup's partial against the float64 sum of its 256 summands, see eikonal_bound.
The yardsticks are measured, not derived: the float32 torch statement on the CPU against the model on the same inputs, recorded in
sdf_head_ref.YARDSTICK and recomputed by tests/test_sdf_head_ref_cpu.py.  Every output is over-allocated and filled with a sentinel; nothing may
be written past M, 3M, 6M, 18M or ceil(M / 256) values."""
import numpy as np
import pytest

import sdf_head_ref as R

pytestmark = pytest.mark.gpu

SENTINEL, PAD = -12345.0, 41
U = R.U


def _dev(t, n):
    """The first n values of a CPU tensor on the device, with one spare value behind them (so that n = 0 still has an address)."""
    import torch
    return torch.cat([t.reshape(-1)[:n], torch.zeros(1)]).cuda()


def _out(n):
    import torch
    return torch.full((n + PAD,), SENTINEL, device="cuda")


def _take(t, n, what):
    a = t.cpu().numpy()
    assert np.all(a[n:] == np.float32(SENTINEL)), f"{what}: written past its {n} values"
    return a[:n]


def run(c, rows=None, eik_coef=None, with_seed=True, with_normal=True, with_eik=True, found_inf=0.0, d_alpha=None, backward=True):
    """One forward and one backward call on the first `rows` samples of case c.  Returns the outputs as numpy arrays."""
    import torch
    from nerf2mesh_amd import _lib as L
    p = L.ptr
    M = c["M"] if rows is None else rows
    nb = (M + 255) // 256
    eik_coef = c["eik_coef"] if eik_coef is None else eik_coef
    sdf, s6, dirs, ts = _dev(c["sdf"], M), _dev(c["s6"], 6 * M), _dev(c["dirs"], 3 * M), _dev(c["ts"], 2 * M)
    g = _dev(c["d_alpha"] if d_alpha is None else d_alpha, M)
    var = torch.tensor([c["var"]], device="cuda")
    seed = torch.tensor([c["seed"]], device="cuda")
    alpha, normal, eik = _out(M), _out(3 * M), _out(nb)
    L.call("n2m_sdf_alpha_forward", p(sdf), p(s6), p(dirs), p(ts), M, p(var), c["eps"], c["car"], p(alpha), p(normal) if with_normal else None,
           p(eik) if with_eik else None, L.stream())
    out = dict(alpha=_take(alpha, M, "alpha"), normal=_take(normal, 3 * M if with_normal else 0, "normal").reshape(-1, 3),
               eik_partial=_take(eik, nb if with_eik else 0, "eik_partial"))
    if backward:
        d_sdf, d_s6, var_part, d_var = _out(M), _out(6 * M), _out(nb), _out(1)
        finf = torch.full((1,), float(found_inf), device="cuda")
        L.call("n2m_sdf_alpha_backward", p(g), p(sdf), p(s6), p(dirs), p(ts), M, p(var), c["eps"], c["car"], p(seed) if with_seed else None,
               float(eik_coef), p(d_sdf), p(d_s6), p(var_part), p(d_var), p(finf), L.stream())
        out.update(d_sdf=_take(d_sdf, M, "d_sdf"), d_s6=_take(d_s6, 6 * M, "d_sdf6").reshape(-1, 6), var_partial=_take(var_part, nb, "var_partial"),
                   d_var=float(_take(d_var, 1, "d_variance")[0]), found_inf=float(finf))
    return out


def eikonal_bound(m, lo, hi):
    """Bound on |partial - sum of the model's (|n| - 1)^2 over samples [lo, hi)|, from the model, u = 2^-24, t = |n| - 1:
      * |n|: the float32 normal, its squares, their sum and the (correctly rounded) sqrt leave |n| with a relative error of 2.5 u;
      * t = |n| - 1 is exact near |n| = 1 (Sterbenz) and carries one rounding elsewhere: t' = t (1 + u) + 2.5 u |n| -- the cancellation
        at |n| ~ 1 is why the error is relative to |n| and not to t;
      * t'^2 = t^2 + 2 t (u t + 2.5 u |n|) + one rounding of the square: t^2 (1 + 3 u) + 5 u |t| |n|;
      * the sum: 6 wave levels + 2 for the four waves, a depth-8 sum of non-negative terms, 8 u t^2 to first order.
    Together sum_i (11 u t_i^2 + 5 u |t_i| |n_i|)."""
    n = np.sqrt((m["normal"][lo:hi] ** 2).sum(-1))
    t = np.abs(n - 1.0)
    return float((11.0 * U * t * t + 5.0 * U * t * n).sum())


def variance_bound(m, name, rows, nb):
    """Bound on |d_variance - float64 sum of the model's summands t_i|:
      * each summand comes out of the same chain as d_sdf and is allowed the same kind of error, KERNEL_FACTOR * yardstick relative to
        |t_i| + median |t| (the yardstick's fourth figure, measured over ALL samples of the case: none can be left out of a sum);
      * the summation, to first order, depth * 2^-24 * sum |t_i| with depth = 6 + 2 (the workgroup's partial) + ceil(nb / 256) (the stride
        loop of the one-workgroup sum) + 8 (its wave sums).
    The first part adds the summands' allowances as if all their errors had one sign, so the bound is only as sharp as the yardstick: about
    5e-4 of sum |t_i| where var is 0.35 or 0.6 and car is 0 or 0.3 -- the configurations that count for d_variance -- and several per cent at
    var = -0.3, where it says little.  That d_variance is exactly 0 under a clipped inv_s is asserted apart from this bound."""
    t = np.abs(m["d_var_term"][:rows])
    return float(R.KERNEL_FACTOR * R.YARDSTICK[name][3] * (t + m["med_d_var"]).sum() + R.var_sum_depth(nb) * U * t.sum())


def check(name, got, rows=None):
    c, m, yard = R.case(name), R.model(name), R.YARDSTICK[name]
    M = c["M"] if rows is None else rows
    nb = (M + 255) // 256
    # normal
    ref = m["normal"][:M]
    err = np.abs(got["normal"] - ref)
    ok = (err <= 4.0 * U * np.abs(ref)) | ((np.abs(ref) < 2.0 ** -126) & (got["normal"] == 0))
    assert ok.all(), (name, "normal", float((err / np.maximum(np.abs(ref), 1e-300)).max()))
    # alpha, d_sdf, d_sdf6
    e_alpha, e_sdf, e_s6 = R.errors(name, got["alpha"], got["d_sdf"], got["d_s6"], rows=M)
    print(f"{name}[:{M}]: alpha {e_alpha:.3g} (yardstick {yard[0]:.3g}), d_sdf {e_sdf:.3g} ({yard[1]:.3g}), d_sdf6 {e_s6:.3g} ({yard[2]:.3g})")
    assert np.isfinite(got["alpha"]).all() and got["alpha"].min() >= 0.0 and got["alpha"].max() <= 1.0
    assert e_alpha <= R.KERNEL_FACTOR * yard[0], (name, "alpha", e_alpha)
    assert e_sdf <= R.KERNEL_FACTOR * yard[1], (name, "d_sdf", e_sdf)
    assert e_s6 <= R.KERNEL_FACTOR * yard[2], (name, "d_sdf6", e_s6)
    assert np.array_equal(got["d_s6"][:, 1::2], -got["d_s6"][:, 0::2]), "the minus copy's gradient is the plus copy's, negated"
    # d_variance
    want = float(m["d_var_term"][:M].sum())
    bound = variance_bound(m, name, M, nb)
    print(f"{name}[:{M}]: d_variance {got['d_var']:.9g} vs {want:.9g}, error {abs(got['d_var'] - want):.3g}, bound {bound:.3g}")
    assert abs(got["d_var"] - want) <= bound, (name, "d_variance", got["d_var"], want, bound)
    assert got["found_inf"] == 0.0
    # eikonal partials, one per workgroup
    for b in range(nb):
        lo, hi = 256 * b, min(256 * b + 256, M)
        want, bound = float(m["eik_term"][lo:hi].sum()), eikonal_bound(m, lo, hi)
        assert abs(float(got["eik_partial"][b]) - want) <= bound, (name, "eikonal partial", b, float(got["eik_partial"][b]), want, bound)


@pytest.mark.parametrize("name", R.CASES)
def test_case_against_the_model(name):
    """Every random population (variance x cos_anneal_ratio x eps at M = 4099, M = 65793 with 258 partials, eik_coef = 0 with seed = NULL)
    and every directed case, forward and backward; normal = NULL and eik_partial = NULL leave alpha bit-identical."""
    c, m = R.case(name), R.model(name)
    got = run(c, with_seed=(name != "no_eikonal"))
    check(name, got)
    bare = run(c, with_normal=False, with_eik=False, backward=False)
    assert np.array_equal(bare["alpha"].view(np.uint32), got["alpha"].view(np.uint32))
    if name == "flat":
        # zero normal; d_sdf6 = +-0.5 dtc dir^ / 1e-10 / eps is ~1e10 times an ordinary gradient: relative error per element
        assert not got["normal"].any()
        rel = np.abs(got["d_s6"] - m["d_s6"]) / np.abs(m["d_s6"])
        print(f"flat: d_sdf6 relative error {rel.max():.3g} (yardstick {R.FLAT_RELATIVE:.3g})")
        assert rel.max() <= R.KERNEL_FACTOR * R.FLAT_RELATIVE
    if name == "tiny_normal":
        # the d_alpha == 0 rows carry the clamped branch's eikonal gradient alone, of order 1 under a median of ~1e9: relative error per element
        rel = R.tiny_eikonal_relative(got["d_s6"])
        print(f"tiny_normal: eikonal rows' d_sdf6 relative error {rel:.3g} (yardstick {R.TINY_EIKONAL_RELATIVE:.3g})")
        assert rel <= R.KERNEL_FACTOR * R.TINY_EIKONAL_RELATIVE
    if name == "axis":
        kind = np.minimum(np.arange(c["M"]) % 8, 2)
        plus = kind == 0                    # cos = +1: alpha = 1e-5 / (p + 1e-5); the x and y copies get no gradient at all
        p = 1.0 / (1.0 + np.exp(-c["sdf"].double().numpy() * np.exp(10.0 * R.f32(c["var"]))))
        assert np.abs(got["alpha"][plus] - 1e-5 / (p[plus] + 1e-5)).max() <= R.KERNEL_FACTOR * R.YARDSTICK[name][0]
        assert not got["d_s6"][kind < 2][:, :4].any()
        assert not got["d_s6"][kind == 2][:, 2:4].any()
    if name in ("clip_high", "clip_low"):
        assert got["d_var"] == 0.0 and not got["var_partial"].any(), "a clipped inv_s passes no gradient to the variance"


@pytest.mark.parametrize("M", R.SIZES)
def test_sizes(M):
    """Below a wave, below a workgroup, around both, several workgroups: the first M samples of the standard population.  eik_coef and the
    normalising medians stay those of the whole population, so each prefix is held to the yardstick measured on the whole."""
    check(R.STANDARD, run(R.case(R.STANDARD), rows=M), rows=M)


def test_no_samples():
    """M = 0: forward and offsets write nothing, backward writes d_variance = 0 and leaves the flag alone."""
    import torch
    from nerf2mesh_amd import _lib as L
    got = run(R.case(R.STANDARD), rows=0, found_inf=1.0)
    assert got["d_var"] == 0.0 and got["found_inf"] == 1.0
    xyz, pts, pts01 = torch.zeros(3, device="cuda"), _out(0), _out(0)
    L.call("n2m_sdf_offsets", L.ptr(xyz), 0, 3e-2, 1.0, L.ptr(pts), L.ptr(pts01), L.stream())
    _take(pts, 0, "pts"), _take(pts01, 0, "pts01")


def test_the_eikonal_term_needs_its_seed():
    """eik_coef != 0 with seed = NULL is refused; eik_coef == 0 with seed = NULL is accepted and d_sdf6 carries no eikonal part."""
    c = R.case("no_eikonal")
    with pytest.raises(RuntimeError, match="seed"):
        run(c, rows=65, with_seed=False, eik_coef=R.LAMBDA_EIK * 2.0 / 65)
    got = run(c, rows=65, with_seed=False)
    check("no_eikonal", got, rows=65)
    full = run(c, rows=65, eik_coef=R.LAMBDA_EIK * 2.0 / 65)
    assert np.abs(full["d_s6"] - got["d_s6"]).max() > 1e-3, "the eikonal term is visible at these weights"


def test_found_inf():
    """0 on finite input (asserted for every case above), 1 when one d_alpha is inf, and a flag already raised is not lowered."""
    c = R.case(R.STANDARD)
    g = c["d_alpha"].clone()
    g[300] = float("inf")
    assert run(c, rows=700, d_alpha=g)["found_inf"] == 1.0
    assert run(c, rows=700, found_inf=1.0)["found_inf"] == 1.0
    assert run(c, rows=700, found_inf=0.0)["found_inf"] == 0.0


@pytest.mark.parametrize("bound", [1.0, 4.0])
@pytest.mark.parametrize("eps", R.EPSS)
@pytest.mark.parametrize("M", [1, 15, 257, 4099])
def test_offsets_bit_equal(M, eps, bound):
    """Points inside, at and beyond +-bound on each axis (the clamp), pts01 given and NULL; 18 M values over ceil(18 M / 256) workgroups."""
    import torch
    from nerf2mesh_amd import _lib as L
    gen = torch.Generator().manual_seed(M)
    xyz = (torch.rand(M, 3, generator=gen) * 2 - 1) * (1.02 * bound)
    for i in range(min(M, 12)):                                               # at the bound, within eps of it, and beyond it, on each axis
        axis, kind = i % 3, i // 3
        xyz[i, axis] = [bound, -bound, bound - 0.5 * eps, -(bound + 3 * eps)][kind]
    want, want01 = R.offsets(xyz.numpy(), eps, bound)
    x = xyz.cuda()
    pts, pts01, alone = _out(18 * M), _out(18 * M), _out(18 * M)
    L.call("n2m_sdf_offsets", L.ptr(x), M, eps, bound, L.ptr(pts), L.ptr(pts01), L.stream())
    L.call("n2m_sdf_offsets", L.ptr(x), M, eps, bound, L.ptr(alone), None, L.stream())
    pts, pts01, alone = _take(pts, 18 * M, "pts"), _take(pts01, 18 * M, "pts01"), _take(alone, 18 * M, "pts")
    assert np.array_equal(pts.view(np.uint32), want.reshape(-1).view(np.uint32))
    assert np.array_equal(pts01.view(np.uint32), want01.reshape(-1).view(np.uint32))
    assert np.array_equal(alone.view(np.uint32), pts.view(np.uint32))
    assert M == 1 or (np.abs(want).max() == np.float32(bound) and want01.min() == 0.0 and want01.max() == 1.0)
