"""CPU: the distortion entry points refuse bad arguments on the host, before any launch (no GPU needed), and the Python layer's checks."""
import pytest


@pytest.fixture(scope="module")
def L():
    from nerf2mesh_amd import _lib, build
    build.build(verbose=False)
    return _lib


p = 16                                                                     # a stand-in for a device pointer: nothing is dereferenced


def _fwd(M=8, N=2, space=0):
    return [p, p, p, p, p, M, N, space, p, p]                              # weights ts rays nears fars | M N space | loss_ray totals


def _bwd(M=8, N=2, space=0, zero_fill=0):
    return [p, p, p, p, p, p, p, M, N, space, zero_fill, p]                # weights ts rays nears fars totals grad_ray | ... | grad_weights


def test_null_in_each_pointer_slot(L):
    for hole in (0, 1, 2, 3, 4, 8, 9):
        args = _fwd()
        args[hole] = None
        with pytest.raises(RuntimeError, match=r"n2m_distortion_forward failed \(-2\).*NULL"):
            L.call("n2m_distortion_forward", *args, None)
    for hole in (0, 1, 2, 3, 4, 5, 6, 11):
        for zero_fill in (0, 1):                                           # the clearing pass comes after the checks as well
            args = _bwd(zero_fill=zero_fill)
            args[hole] = None
            with pytest.raises(RuntimeError, match=r"n2m_distortion_backward failed \(-2\).*NULL"):
                L.call("n2m_distortion_backward", *args, None)


def test_empty_tensors_are_refused(L):
    for M, N in ((0, 2), (8, 0), (0, 0)):
        with pytest.raises(RuntimeError, match=r"n2m_distortion_forward failed \(-1\).*empty"):
            L.call("n2m_distortion_forward", *_fwd(M=M, N=N), None)
        with pytest.raises(RuntimeError, match=r"n2m_distortion_backward failed \(-1\).*empty"):
            L.call("n2m_distortion_backward", *_bwd(M=M, N=N, zero_fill=1), None)


def test_bad_space_is_refused(L):
    for space in (-1, 2, 7):
        with pytest.raises(RuntimeError, match=r"n2m_distortion_forward failed \(-1\).*space must be 0 \(linear\) or 1 \(disparity\)"):
            L.call("n2m_distortion_forward", *_fwd(space=space), None)
        with pytest.raises(RuntimeError, match=r"n2m_distortion_backward failed \(-1\).*space must be 0 \(linear\) or 1 \(disparity\)"):
            L.call("n2m_distortion_backward", *_bwd(space=space, zero_fill=1), None)


def test_python_layer_refuses_unknown_space_and_mismatched_shapes(L):
    import torch
    from nerf2mesh_amd.losses import DISTORT_SPACES, distortion_loss
    assert DISTORT_SPACES == {"linear": 0, "disparity": 1}
    w, ts, rays, near, far = torch.rand(5), torch.rand(5, 2), torch.tensor([[0, 3], [3, 2]], dtype=torch.int32), torch.ones(2), torch.full((2,), 2.0)
    with pytest.raises(ValueError, match="space must be one of"):
        distortion_loss(w, ts, rays, near, far, space="log")
    for bad in ((w[:4], ts, rays, near, far), (w, ts[:, :1], rays, near, far), (w, ts, rays.reshape(-1), near, far), (w, ts, rays, near[:1], far),
                (w, ts, rays, near, far[:1]), (w.view(5, 1), ts, rays, near, far)):
        with pytest.raises(ValueError, match="expected weights"):
            distortion_loss(*bad)
    with pytest.raises(ValueError, match="no rays"):
        distortion_loss(w, ts, rays[:0], near[:0], far[:0])


def test_trainer_refuses_an_unknown_space():
    import torch
    from nerf2mesh_amd.network import NeRFNetwork
    from nerf2mesh_amd.options import make_options
    from nerf2mesh_amd.trainer import Stage0Trainer
    from nerf2mesh_amd import synthetic
    assert make_options().lambda_distort == 0 and make_options().distort_space == "linear"
    opt = make_options(bound=1, dt_gamma=0, lambda_distort=0.01, distort_space="log")
    with pytest.raises(ValueError, match="distort_space must be one of"):
        Stage0Trainer(NeRFNetwork(opt), opt, synthetic.make_cameras(2, seed=0), torch.device("cpu"))
