"""The field backward's weight-gradient sum as rider workgroups of the table backward's accumulate kernel.

The second stage of the dW reduction (dw_finalize_kernel: the rows the field backward's workgroups leave, added up in a fixed order into the seven d_w
tensors, found_inf raised on a non-finite sum) is a launch of its own between the field backward and the fill.  Its inputs are complete when the field
backward ends and only the optimizer reads its outputs, so the step executor lets the accumulate kernel carry it as 120 extra workgroups at the end of
its grid (n2m_field_backward_defer_dw + n2m_grid_backward_dw_rider).  Held here, bit for bit: the carried sum against the stand-alone launch
(n2m_field_dw_sum) for 1, 2 and 256 partial rows, clean / inf / nan, the masks of diffuse and full shading; the accumulate's own table gradients with
and without riders; a seeded executor run under N2M_RIDERS=1 and =0."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DW_OFF = [0, 608, 640, 2880, 6976, 7360, 7552, 7648]      # sigma0 sigma1 color0 color1 color2 spec0 spec1
DW_TOTAL = 7648
MASKS = {"diffuse": 0x1F, "full": 0x7F}                   # what the step uses: density + colour [+ specular]
ENGINE_ROWS = 256                                         # the field backward's grid at any batch of >= 2^15 samples


@pytest.fixture(scope="module")
def host():
    """A table backward over 2^10 samples of the standard 16-level pair of tables, and its gradients WITHOUT riders (computed once)."""
    from nerf2mesh_amd import _lib as L
    from nerf2mesh_amd.gridencoder import GridEncoder, _host_offsets
    p = L.ptr
    M = 1 << 10
    g = torch.Generator(device="cuda").manual_seed(3)
    e1 = GridEncoder(level_dim=1, desired_resolution=2048).cuda()
    ho = _host_offsets(e1)
    rows = e1.embeddings.shape[0]
    xyz = (torch.rand(M, 3, device="cuda", generator=g) * 2 - 1).contiguous()
    d1 = torch.randn(16, M, device="cuda", generator=g) * 1e-3
    d2 = (torch.randn(16, M, 2, device="cuda", generator=g) * 0.05).half()
    emb = (torch.randn(rows, 1, device="cuda", generator=g) * 0.1).contiguous()
    scale_t = torch.tensor(4096.0, device="cuda")
    ws = L.workspace(xyz.device, L.lib().n2m_grid_binned_pair_workspace_bytes(M, 16, ho.ctypes.data))
    S, H0 = float(np.log2(e1.per_level_scale)), int(e1.base_resolution)

    def run(dsum=None):
        g1 = torch.full((rows, 1), float("nan"), device="cuda")
        g2 = torch.full((rows, 2), float("nan"), device="cuda", dtype=torch.float16)
        finf = torch.zeros((), device="cuda")
        carried = ctypes.c_int(0)
        L.grid_backward_config(1, 1.0)
        if dsum is not None:
            L.call("n2m_grid_backward_dw_rider", ctypes.addressof(dsum), ctypes.byref(carried))
        try:
            L.call("n2m_grid_encode_backward_binned_pair", p(d1), p(d2), p(xyz), ho.ctypes.data, p(g1), p(g2), M, 16, 16, S, H0, e1.gridtype_id,
                   int(bool(e1.align_corners)), e1.interp_id, p(emb), 1e-4, 1e-4, 0.5, p(scale_t), p(finf), 0.5, 0.5, 1, p(ws), ws.numel(), L.stream())
        finally:
            L.call("n2m_grid_backward_dw_rider", None, None)
        torch.cuda.synchronize()
        return g1, g2, finf, carried.value

    g1, g2, finf, carried = run()
    assert carried == 0 and float(finf) == 0.0
    assert bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0 and float(g2.float().abs().max()) > 0
    return run, (g1, g2)


def _dw_sum(L, part, n_rows, mask, dw0, finf):
    """N2mDwSum over views of one flat [7648] buffer, like the executor's dw_views."""
    d = L.DwSum()
    d.partial, d.n_rows, d.mask, d.found_inf = part.data_ptr(), n_rows, mask, finf.data_ptr()
    for i in range(7):
        d.dw[i] = dw0.data_ptr() + 4 * DW_OFF[i]
    return d


@pytest.mark.parametrize("plant", ["clean", "inf", "nan"])
@pytest.mark.parametrize("n_rows", [1, 2, ENGINE_ROWS])
def test_carried_sum_equals_the_stand_alone_launch(host, n_rows, plant):
    from nerf2mesh_amd import _lib as L
    run, (ref_g1, ref_g2) = host
    g = torch.Generator(device="cuda").manual_seed(100 * n_rows + len(plant))
    part = torch.randn(n_rows, DW_TOTAL, device="cuda", generator=g)
    part[:, 17] = 0.0                                       # a column that sums to exactly zero: the tensor's entry is not touched
    if plant != "clean":                                    # one bad value in one row: a colour weight (in both masks)
        part[n_rows // 2, 3000] = float(plant)
    base = torch.randn(DW_TOTAL, device="cuda", generator=g)      # the sums are ACCUMULATED into what the tensors hold
    for name, mask in MASKS.items():
        dw_a, dw_b = base.clone(), base.clone()
        finf_a, finf_b = torch.zeros((), device="cuda"), torch.zeros((), device="cuda")
        sum_a, sum_b = _dw_sum(L, part, n_rows, mask, dw_a, finf_a), _dw_sum(L, part, n_rows, mask, dw_b, finf_b)
        L.call("n2m_field_dw_sum", ctypes.addressof(sum_a), L.stream())
        g1, g2, table_finf, carried = run(sum_b)
        assert carried == 1, "the partition-major accumulate must have taken the sum along"
        assert torch.equal(dw_a.view(torch.int32), dw_b.view(torch.int32)), f"{name}: d_w tensors"
        assert torch.equal(finf_a, finf_b) and float(finf_a) == (0.0 if plant == "clean" else 1.0), f"{name}: found_inf"
        assert float(table_finf) == 0.0
        if mask == MASKS["diffuse"]:                        # tensors outside the mask keep their values
            assert torch.equal(dw_b[DW_OFF[5]:], base[DW_OFF[5]:])
        assert not torch.equal(dw_b[:DW_OFF[5]], base[:DW_OFF[5]])
        assert float(dw_b[17]) == float(base[17])
        # the host kernel's own outputs: the table gradients of the launch without riders
        assert torch.equal(g1, ref_g1) and torch.equal(g2, ref_g2), f"{name}: table gradients with riders"


def test_field_backward_defers_its_second_stage():
    """n2m_field_backward_defer_dw: the backward's other outputs do not change, and backward + n2m_field_dw_sum leaves the d_w the plain call leaves."""
    from nerf2mesh_amd import _lib as L
    p = L.ptr
    M = 1000
    g = torch.Generator(device="cuda").manual_seed(11)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    x, d = (torch.rand(M, 3, device="cuda", generator=g) * 2 - 1), torch.nn.functional.normalize(r(M, 3), dim=-1)
    h1, h2 = r(16, M) * 0.1, (r(16, M, 2) * 0.1).half()
    shapes = [(32, 19), (1, 32), (64, 35), (64, 64), (6, 64), (32, 6), (3, 32)]
    w = [r(*s) * 0.2 for s in shapes]
    d_sigma, d_rgb = r(M) * 1e-2, r(M, 3) * 1e-2
    out = {}
    for defer in (False, True):
        dh1, dh2 = torch.zeros(16, M, device="cuda"), torch.zeros(16, M, 2, device="cuda", dtype=torch.float16)
        dw = torch.zeros(DW_TOTAL, device="cuda")
        views = [dw[DW_OFF[i]:DW_OFF[i + 1]] for i in range(7)]
        finf = torch.zeros((), device="cuda")
        dsum = L.DwSum()
        if defer:
            L.call("n2m_field_backward_defer_dw", ctypes.addressof(dsum))
        try:
            L.call("n2m_field_backward_train", p(x), p(d), p(h1), p(h2), *[p(t) for t in w], M, 1, 0, p(d_sigma), p(d_rgb), None, p(dh1), p(dh2),
                   *[p(v) for v in views], p(finf), 0.0, None, L.stream())
        finally:
            L.call("n2m_field_backward_defer_dw", None)
        if defer:
            torch.cuda.synchronize()
            assert float(dw.abs().max()) == 0.0, "the deferred call must not have summed"
            assert dsum.partial and dsum.n_rows == (M + 127) // 128 and dsum.mask == 0x7F and dsum.found_inf == finf.data_ptr()
            L.call("n2m_field_dw_sum", ctypes.addressof(dsum), L.stream())
        torch.cuda.synchronize()
        out[defer] = (dh1, dh2, dw, finf)
    assert float(out[False][2].abs().max()) > 0
    for a, b in zip(out[False], out[True]):
        assert torch.equal(a, b)


def test_executor_trains_to_identical_bits_with_and_without_riders(monkeypatch):
    """40 seeded steps at --num-points 4096 (two occupancy refreshes): parameters, loss scale and every step's loss value."""
    from nerf2mesh_amd import _lib as L
    from nerf2mesh_amd import synthetic
    from nerf2mesh_amd.engine import Stage0Engine
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    dev = torch.device("cuda", 0)
    calls = []
    plain_call = L.call

    def spy(name, *args):
        calls.append(name if name != "n2m_grid_backward_dw_rider" or args[0] is None else "arm")
        return plain_call(name, *args)
    monkeypatch.setattr(L, "call", spy)
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("N2M_RIDERS", flag)
        del calls[:]
        torch.manual_seed(0)
        opt = make_options(O=True, bound=1, dt_gamma=0, iters=30000, fused_mlp=True)
        opt.num_points, opt.num_rays = 4096, 256
        eng = Stage0Engine(NeRFNetwork(opt), opt, synthetic.make_cameras(20, seed=0), dev, seed=0)
        assert eng.riders == (flag == "1")
        eng.mark_untrained()
        losses = [eng.train_step().clone() for _ in range(40)]
        torch.cuda.synchronize()
        res[flag] = ([q.detach().clone() for q in eng.model.parameters()], eng.optimizer.scale.clone(), torch.stack(losses))
        armed = calls.count("arm")
        if flag == "1":
            assert armed > 0 and calls.count("n2m_field_dw_sum") == 0, "every step's accumulate carries the sum"
        else:
            assert armed == 0 and calls.count("n2m_field_backward_defer_dw") == 0
    for a, b in zip(res["1"][0], res["0"][0]):
        assert torch.equal(a, b)
    assert torch.equal(res["1"][1], res["0"][1]), "loss scale"
    assert torch.equal(res["1"][2].view(torch.int32), res["0"][2].view(torch.int32)), "per-step loss values"
    assert bool(torch.isfinite(res["1"][2]).all())
