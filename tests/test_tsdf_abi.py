"""CPU: n2m_tsdf_integrate refuses bad arguments on the host, before any launch (no GPU needed), and the Python layer's checks."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def L():
    from nerf2mesh_amd import _lib, build
    build.build(verbose=False)
    return _lib


p = 16                                                                     # a stand-in for a device pointer: nothing is dereferenced
f3 = ctypes.c_float * 3


def _args(R=(4, 5, 6), lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), n=2, H=3, W=4, trunc=0.5, min_depth=0.0, w_max=8.0):
    # tsdf weight | R0 R1 R2 | lo hi (host) | cams depth | n H W | trunc min_depth w_max
    return [p, p, *R, f3(*lo), f3(*hi), p, p, n, H, W, trunc, min_depth, w_max]


def _refused(L, code, match, **kw):
    with pytest.raises(RuntimeError, match=rf"n2m_tsdf_integrate failed \({code}\).*{match}"):
        L.call("n2m_tsdf_integrate", *_args(**kw), None)


def test_null_in_each_pointer_slot(L):
    for hole in (0, 1, 5, 6, 7, 8):
        args = _args()
        args[hole] = None
        with pytest.raises(RuntimeError, match=r"n2m_tsdf_integrate failed \(-2\).*NULL"):
            L.call("n2m_tsdf_integrate", *args, None)


def test_empty_inputs_are_refused(L):
    for kw in (dict(n=0), dict(H=0), dict(W=0), dict(H=0, W=0)):
        _refused(L, -1, "empty depth maps", **kw)
    for kw in (dict(H=1 << 24), dict(W=1 << 24)):
        _refused(L, -1, "below 2\\^24", **kw)


def test_degenerate_volumes_are_refused(L):
    for R in ((1, 5, 6), (4, 1, 6), (4, 5, 1), (0, 5, 6), (1, 1, 1)):
        _refused(L, -1, "at least 2 lattice points", R=R)
    for R in ((1 << 16, 1 << 16, 2), (2048, 2048, 1024), (4294967295, 2, 2)):            # 2^33, 2^32, ~2^34 points
        _refused(L, -1, "beyond 32-bit indexing", R=R)
    for lo, hi in (((-1, -1, -1), (-1, 1, 1)), ((-1, -1, -1), (1, -2, 1)), ((0, 0, 0.5), (1, 1, 0.5)), ((float("nan"), 0, 0), (1, 1, 1))):
        _refused(L, -1, "hi must be above lo", lo=lo, hi=hi)


def test_bad_scalars_are_refused(L):
    for trunc in (0.0, -0.1, float("nan")):
        _refused(L, -1, "trunc must be > 0", trunc=trunc)
    for w_max in (0.0, 0.999, -3.0, float("nan")):
        _refused(L, -1, "w_max must be >= 1", w_max=w_max)
    for min_depth in (-1e-6, -2.0, float("nan")):
        _refused(L, -1, "min_depth must be >= 0", min_depth=min_depth)


def test_volume_constructor_checks():
    import torch
    from nerf2mesh_amd.tsdf import TSDFVolume
    vol = TSDFVolume((3, 4, 5), device="cpu")
    assert vol.resolution == (3, 4, 5) and tuple(vol.tsdf.shape) == (3, 4, 5) and vol.tsdf.dtype == vol.weight.dtype == torch.float32
    assert bool((vol.tsdf == 1).all()) and bool((vol.weight == 0).all())
    assert vol.trunc == pytest.approx(4 * 1.0) and vol.w_max == 64.0 and vol.min_depth == 0.0      # spacings 1, 2/3, 1/2: the coarsest is 1
    assert TSDFVolume(9, device="cpu").resolution == (9, 9, 9) and TSDFVolume(9, lo=(0, 0, 0), hi=(1, 2, 4), device="cpu").trunc == pytest.approx(2.0)
    for res in (1, (4, 4), (4, 1, 4), 2.5, (4, 4, 4, 4)):
        with pytest.raises(ValueError, match="resolution"):
            TSDFVolume(res, device="cpu")
    with pytest.raises(ValueError, match="hi must be above lo"):
        TSDFVolume(4, lo=(0, 0, 0), hi=(1, 0, 1), device="cpu")
    for kw, match in ((dict(trunc=0.0), "trunc"), (dict(trunc=-1.0), "trunc"), (dict(w_max=0.5), "w_max"), (dict(min_depth=-0.1), "min_depth")):
        with pytest.raises(ValueError, match=match):
            TSDFVolume(4, device="cpu", **kw)


def test_integrate_checks_shapes_dtypes_and_devices():
    import torch
    from nerf2mesh_amd.tsdf import TSDFVolume, camera_rows, surface_depth
    vol = TSDFVolume(4, device="cpu")
    cams, depth = torch.zeros(2, 16), torch.zeros(2, 3, 5)
    for bad in ((cams[:, :15], depth), (cams.reshape(-1), depth), (cams, depth[0]), (cams, depth[:1]), (cams[:1], depth), (cams, depth.reshape(2, 15))):
        with pytest.raises(ValueError, match=r"expected cams \[n,16\] and depth \[n,H,W\]"):
            vol.integrate(*bad)
    with pytest.raises(ValueError, match="no views or empty"):
        vol.integrate(cams[:0], depth[:0])
    with pytest.raises(ValueError, match="no views or empty"):
        vol.integrate(cams, depth[:, :0])
    for bad in ((cams.double(), depth), (cams, depth.half()), (cams, depth.long())):
        with pytest.raises(ValueError, match="must be float32"):
            vol.integrate(*bad)
    for bad in ((cams.to("meta"), depth), (cams, depth.to("meta"))):                 # another device than the volume's
        with pytest.raises(ValueError, match="the volume lives on cpu"):
            vol.integrate(*bad)
    with pytest.raises(ValueError, match="must be tensors"):
        vol.integrate(cams.numpy(), depth)
    with pytest.raises(RuntimeError, match="no host path"):                          # well-formed, but the fusion runs on the device only
        vol.integrate(cams, depth)
    assert bool((vol.tsdf == 1).all()) and bool((vol.weight == 0).all())
    # the helpers' own checks
    with pytest.raises(ValueError, match=r"poses must be \[n,4,4\]"):
        camera_rows(torch.eye(4), (1.0, 1.0, 0.5, 0.5))
    with pytest.raises(ValueError, match="intrinsics must be"):
        camera_rows(torch.eye(4)[None].repeat(2, 1, 1), torch.ones(3, 4))
    rows = camera_rows(torch.eye(4)[None].repeat(2, 1, 1), (7.0, 8.0, 1.5, 2.5))
    assert tuple(rows.shape) == (2, 16) and rows[1].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 7, 8, 1.5, 2.5]
    with pytest.raises(ValueError, match="alpha_carve <= alpha_min"):
        surface_depth({"depth": depth, "weights_sum": depth}, alpha_min=0.1, alpha_carve=0.2)
    with pytest.raises(ValueError, match="no 'weights_sum'"):
        surface_depth({"depth": depth})


def test_surface_depth_encoding():
    import math
    import torch
    from nerf2mesh_amd.tsdf import surface_depth
    alpha = torch.tensor([1.0, 0.8, 0.5, 0.49, 0.05, 0.04, 0.0])
    out = {"depth": alpha * 2.0, "weights_sum": alpha}
    assert surface_depth(out).tolist() == pytest.approx([2.0, 2.0, 2.0, 0.0, 0.0, 0.0, 0.0])
    carved = surface_depth(out, carve=True).tolist()
    assert carved[:5] == pytest.approx([2.0, 2.0, 2.0, 0.0, 0.0]) and carved[5:] == [math.inf, math.inf]
    assert surface_depth(out, alpha_min=0.9, carve=True, alpha_carve=0.5).tolist() == pytest.approx([2.0, 0, 0, math.inf, math.inf, math.inf, math.inf])


def test_export_stage0_refuses_bad_methods(tmp_path):
    """method="tsdf" needs a Capture and the density recipe; an unknown method is refused.  All before anything is computed or written."""
    import torch
    from nerf2mesh_amd import synthetic
    from nerf2mesh_amd.capture import Capture
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    o = make_options()
    assert (o.mesh_method, o.tsdf_trunc, o.tsdf_carve, o.tsdf_alpha_min) == ("density", 0, False, 0.5)
    model = NeRFNetwork(make_options(bound=1, dt_gamma=0))
    out = tmp_path / "mesh"
    with pytest.raises(ValueError, match="method must be 'density' or 'tsdf'"):
        model.export_stage0(str(out), method="sdf")

    class DS:
        H = W = 8
        mvps = torch.eye(4)[None]
    for dataset in (None, DS()):
        with pytest.raises(ValueError, match="needs dataset=<capture.Capture>"):
            model.export_stage0(str(out), method="tsdf", dataset=dataset)
    cap = Capture.synthetic(synthetic.make_cameras(2, seed=0), H=4, W=4, intrinsics=(9.0, 9.0, 2.0, 2.0))
    sdf_model = NeRFNetwork(make_options(bound=1, dt_gamma=0, sdf=True))
    with pytest.raises(ValueError, match="SDF recipe"):
        sdf_model.export_stage0(str(out), method="tsdf", dataset=cap)
    assert not out.exists()


def test_export_options_follow_the_namespace():
    from nerf2mesh_amd.options import make_options
    from nerf2mesh_amd.tsdf import export_options
    assert export_options(make_options()) == {}
    assert export_options(make_options(mesh_method="tsdf")) == {"method": "tsdf", "tsdf": {"trunc": None, "carve": False, "alpha_min": 0.5}}
    assert export_options(make_options(mesh_method="tsdf", tsdf_trunc=0.1, tsdf_carve=True, tsdf_alpha_min=0.7)) == \
        {"method": "tsdf", "tsdf": {"trunc": 0.1, "carve": True, "alpha_min": 0.7}}
