"""GPU: n2m_contract / n2m_uncontract against the CPU torch statements bit for bit, and n2m_gather_contract_x01 against
n2m_gather_rows_strided + the statement + the stage-1 executor's table-coordinate expressions (csrc/contract.hip)."""
import numpy as np
import pytest

import contract_case as C

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
    """torch.equal on the int32 views, NaN-aware: NaNs in the same places, every other element in the same bits."""
    import torch
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(a.view(torch.int32)[~na], b.view(torch.int32)[~nb])


@pytest.fixture(scope="module")
def points():
    """The special points, the non-finite rows and random points in [-8, 8]^3, shuffled so that every prefix mixes them; with the CPU
    statements' results, computed once."""
    import torch
    from nerf2mesh_amd.renderer import contract, uncontract
    x = np.concatenate([C.special_points(), C.nonfinite_points(), C.uncontract_points(64), C.contract_points(1000)[len(C.special_points()):]])
    x = x[np.random.default_rng(5).permutation(len(x))][:1000]
    # the rows every size must see: put a NaN row, an inf row, mag == 1 and the next float above it up front
    up = np.nextafter(np.float32(1), np.float32(2))
    x[0] = [up, -0.5, 0.25]
    x[1:5] = [[np.nan, 1, 2], [np.inf, -3, 0], [1, -1, 0.5], [1e4, -1e4, 7]]
    t = torch.from_numpy(x)
    assert not t.is_cuda
    with np.errstate(all="ignore"):
        return t, contract(t), uncontract(t)


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
def test_contract_kernels_equal_the_cpu_statements(points, N):
    import torch
    from nerf2mesh_amd import _lib as L
    x, want_c, want_u = (t[:N] for t in points)
    dev = torch.device("cuda")
    for name, want in (("n2m_contract", want_c), ("n2m_uncontract", want_u)):
        src = x.to(dev)
        out = torch.full((N + 1, 3), -7.0, device=dev)                       # one guard row behind the output
        L.call(name, L.ptr(src), N, L.ptr(out), L.stream())
        assert _same_bits(out[:N], want), name
        assert bool((out[N] == -7.0).all()) and _same_bits(src, x), name      # nothing past row N, input untouched
        buf = torch.full((N + 1, 3), -7.0, device=dev)
        buf[:N] = src
        L.call(name, L.ptr(buf), N, L.ptr(buf), L.stream())                   # in place
        assert _same_bits(buf[:N], want) and bool((buf[N] == -7.0).all()), name


def test_contract_kernels_empty_and_null():
    import torch
    from nerf2mesh_amd import _lib as L
    buf = torch.zeros(4, 3, device="cuda")
    for name in ("n2m_contract", "n2m_uncontract"):
        L.call(name, None, 0, None, L.stream())                                # N == 0: success, no launch
        L.call(name, L.ptr(buf), 0, L.ptr(buf), L.stream())
        for args in ((None, 4, L.ptr(buf)), (L.ptr(buf), 4, None)):
            assert getattr(L.lib(), name)(*args, L.stream()) == -1             # N2M_EINVAL
    L.call("n2m_gather_contract_x01", None, None, 0, 4, 1, 2.0, None, None, L.stream())
    assert L.lib().n2m_gather_contract_x01(None, None, 4, 4, 1, 2.0, L.ptr(buf), L.ptr(buf), L.stream()) == -1
    assert not bool(buf.any())


def test_renderer_routes_device_rows_through_the_kernels(points):
    """renderer.contract / uncontract on device rows (no gradient): the kernels' bits; with a gradient attached the statement, as before."""
    import torch
    from nerf2mesh_amd.renderer import contract, uncontract
    x, want_c, want_u = points
    d = x.cuda()
    assert _same_bits(contract(d), want_c) and _same_bits(uncontract(d), want_u)
    g = d[5:]
    g = g[torch.isfinite(g).all(dim=1) & (g.abs().amax(dim=1) < 100) & (g.abs().amax(dim=1) > 1e-3)].clone().requires_grad_()
    assert g.shape[0] > 500
    y = contract(g)
    assert y.requires_grad
    y.sum().backward()
    assert g.grad is not None and bool(torch.isfinite(g.grad).all())


@pytest.fixture(scope="module")
def image():
    """A [5000, 4] image whose position columns reach outside the unit box, and ascending index lists of 1, 257 and 4099 rows."""
    import torch
    g = torch.Generator().manual_seed(21)
    img = (torch.rand(5000, 4, generator=g) * 2 - 1) * 3
    idx = {1: torch.tensor([4321]), 257: torch.sort(torch.randperm(5000, generator=g)[:257]).values,
           4099: torch.sort(torch.randperm(5000, generator=g)[:4099]).values}
    sp = torch.from_numpy(C.special_points())
    img[idx[257][:len(sp)], :3] = sp                         # the special points sit on rows the 257-row list gathers
    img[4321, :3] = torch.tensor([1.5, -2.75, 0.2])
    return img, idx


@pytest.mark.parametrize("bound", [2.0, 1.5])
@pytest.mark.parametrize("contract_on", [0, 1])
@pytest.mark.parametrize("K", [1, 257, 4099])
def test_gather_contract_x01(image, K, contract_on, bound):
    import torch
    from nerf2mesh_amd import _lib as L
    from nerf2mesh_amd.renderer import contract
    dev = torch.device("cuda")
    img_cpu, idx_all = image
    idx = idx_all[K].to(dev)
    K = int(idx.numel())
    img = img_cpu.to(dev)
    s = L.stream()
    # what the executor did: n2m_gather_rows_strided, [the statement, on the CPU], its two table-coordinate expressions on the device
    want_pts = torch.empty(K, 3, device=dev)
    L.call("n2m_gather_rows_strided", L.ptr(img), L.ptr(idx), K, 3, 4, L.ptr(want_pts), 3, s)
    assert torch.equal(want_pts.cpu(), img_cpu[idx.cpu(), :3])
    if contract_on:
        want_pts = contract(want_pts.cpu()).to(dev)
    want_x01 = torch.empty(K, 3, device=dev)
    if float(np.log2(bound)).is_integer():
        torch.add(torch.tensor(0.5, device=dev), want_pts, alpha=0.5 / bound, out=want_x01)
    else:
        torch.add(want_pts, bound, out=want_x01)
        want_x01.div_(2.0 * bound)
    pts, x01 = torch.full((K + 1, 3), -7.0, device=dev), torch.full((K + 1, 3), -7.0, device=dev)
    L.call("n2m_gather_contract_x01", L.ptr(img), L.ptr(idx), K, 4, contract_on, bound, L.ptr(pts), L.ptr(x01), s)
    assert _same_bits(pts[:K], want_pts) and _same_bits(x01[:K], want_x01)
    assert bool((pts[K] == -7.0).all()) and bool((x01[K] == -7.0).all())
    assert torch.equal(img.cpu(), img_cpu)                  # the fourth column and every row, gathered or not, unchanged
    if contract_on:
        assert float(pts[:K].abs().max()) < 2.0 and bool((img_cpu[idx.cpu(), :3].abs().amax(dim=1) > 1).any())
