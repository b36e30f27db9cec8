"""n2m_capture_undistort (csrc/capture.hip) against its torch statement (capture.undistort_bank / undistort_depth on CPU tensors): bit for
bit, for every lens case of tests/undistort_ref.py, in the broadcast and the per-view form; and a geometric round trip against an analytic
target, with the float64 loop model of the resampler as its yardstick."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import undistort_ref as R   # noqa: E402
from nerf2mesh_amd import capture as C   # noqa: E402

pytestmark = pytest.mark.gpu

IDS = [c[0] for c in R.CASES]
H, W = R.H, R.W                            # 24 x 33: a row is no multiple of a wave, the last block has a tail


def _lens(model, intr, coeff):
    _, family, row = C.lens_row(model, R.colmap_params(model, intr, coeff))
    return family, row


def _out(intr, s):
    return (s * intr[0], s * intr[1], intr[2], intr[3])


def _tables(V, intr, out, row):
    """Per-view rows that differ from view to view: focal lengths, zoom and coefficients scaled a little per view."""
    f = 1 + 0.03 * np.arange(V)[:, None]
    src = np.tile(intr, (V, 1)) * np.concatenate([f, f, np.ones((V, 2))], 1)
    dst = np.tile(out, (V, 1)) * np.concatenate([f * f, f * f, np.ones((V, 2))], 1)
    return src, dst, np.tile(row, (V, 1)) / f


@pytest.mark.parametrize("V,form", [(1, "broadcast"), (3, "broadcast"), (3, "table")])
@pytest.mark.parametrize("name,model,coeff,intr", R.CASES, ids=IDS)
def test_bank_equals_the_torch_statement(name, model, coeff, intr, V, form):
    family, row = _lens(model, intr, coeff)
    s = C.undistort_zoom(H, W, intr, family, row)
    args = (intr, _out(intr, s), row) if form == "broadcast" else _tables(V, intr, _out(intr, s), row)
    bank, _ = C.pack_rgba8(R.noise_images(V, H, W, seed=V))
    want = C.undistort_bank(bank, H, W, *args, family)
    buf = torch.full((V * H * W + 7,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")          # 7 guard words behind the bank
    got = C.undistort_bank(bank.cuda(), H, W, *args, family, out=buf[:V * H * W].view(V, H * W))
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr()
    assert torch.equal(got.cpu(), want), f"{(got.cpu() != want).sum().item()} of {want.numel()} words differ"
    assert (buf[V * H * W:] == 0x5A5A5A5A).all(), "wrote past the bank"
    assert not torch.equal(want, bank)
    if form == "table":
        assert not torch.equal(want[1], C.undistort_bank(bank[1:2], H, W, intr, _out(intr, s), row, family)[0])      # the rows are read per view


@pytest.mark.parametrize("form", ["broadcast", "table"])
@pytest.mark.parametrize("name,model,coeff,intr", R.CASES, ids=IDS)
def test_depth_planes_equal_the_statement_and_only_move_values(name, model, coeff, intr, form):
    family, row = _lens(model, intr, coeff)
    s = C.undistort_zoom(H, W, intr, family, row)
    V = 2
    out = _out(intr, 1.15 * s)            # a further zoom: at the rule's own zoom the map stays within half a texel here and would move nothing
    args = (intr, out, row) if form == "broadcast" else _tables(V, intr, out, row)
    planes = torch.rand(V, H * W, generator=torch.Generator().manual_seed(7)) * 5 + 0.5
    want = C.undistort_depth(planes, H, W, *args, family)
    buf = torch.full((V * H * W + 7,), -7.0, device="cuda")
    got = C.undistort_depth(planes.cuda(), H, W, *args, family, out=buf[:V * H * W].view(V, H * W)).cpu()
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert (buf[V * H * W:] == -7.0).all(), "wrote past the planes"
    for v in range(V):
        assert torch.isin(got[v], planes[v]).all()                        # nearest texel: every value is one of its source plane's, nothing mixed
    assert not torch.equal(got, planes)


def test_entry_point_refuses_bad_arguments():
    import ctypes
    from nerf2mesh_amd import _lib as L
    bank = torch.zeros(1, H * W, dtype=torch.int32, device="cuda")
    out = torch.full_like(bank, 3)
    rows = torch.zeros(16, device="cuda")
    def rc(**over):
        kw = dict(src=L.ptr(bank), dst=L.ptr(out), V=1, H=H, W=W, model=L.LENS_BROWN, depth=0, per_view=0, src_intrinsics=L.ptr(rows),
                  out_intrinsics=L.ptr(rows), lens=L.ptr(rows))
        kw.update(over)
        return L.lib().n2m_capture_undistort(ctypes.byref(L.Undistort(**kw)), L.stream())
    assert rc(lens=None) == rc(src=None) == -2                            # N2M_ENULL
    assert rc(model=0) != 0 and rc(model=3) != 0 and rc(dst=L.ptr(bank)) != 0 and rc(W=0) != 0 and rc(lens=L.ptr(rows) + 4) != 0
    torch.cuda.synchronize()
    assert (out == 3).all()                                               # nothing was launched


def _round_trip(model, coeff, intr, freq_scale=1.0):
    family, row = _lens(model, intr, coeff)
    s = C.undistort_zoom(H, W, intr, family, row)
    out = _out(intr, s)
    photo = R.photograph(lambda a, b: C.lens_undistort(family, row, a, b), intr, H, W, freq_scale)
    bank, _ = C.pack_rgba8(photo[None])
    got = C.undistort_bank(bank.cuda(), H, W, intr, out, row, family).cpu().view(torch.uint8).view(H, W, 4).numpy().astype(np.float64)
    model64, _ = R.undistort_images(photo[None], model, coeff, intr, out)
    want = R.target(out, H, W, freq_scale)
    kernel = np.abs(got - want).max()
    yard = np.abs(model64[0].astype(np.float64) - want).max()
    plain = np.abs(photo.astype(np.float64) - R.target(intr, H, W, freq_scale)).max()           # the photograph read as a pinhole image
    return kernel, yard, plain


@pytest.mark.parametrize("name,model,coeff,intr", R.CASES, ids=IDS)
def test_round_trip_against_the_analytic_target(name, model, coeff, intr):
    """The kernel may miss the target by the float64 resampler's own error (bilinear interpolation + 8-bit rounding of the photograph and of
    the result) plus the 1 LSB the fp32 statement may differ from the float64 model by (tests/test_undistort_cpu.py)."""
    kernel, yard, plain = _round_trip(model, coeff, intr)
    print(f"{name}: kernel {kernel:.3f} LSB, float64 resampler {yard:.3f} LSB, read without undistortion {plain:.3f} LSB")
    assert kernel <= yard + 1.0
    if name == "pincushion":                                              # k1 = 0.1: ignoring the lens is several LSB wrong at the corners
        assert plain > yard + 4.0
