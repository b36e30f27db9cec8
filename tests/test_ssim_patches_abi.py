"""CPU: the batched patch SSIM entry points refuse bad arguments on the host, before any launch (no GPU needed); the scratch size is the
band count; the Python layer's checks."""
import pytest


@pytest.fixture(scope="module")
def L():
    from nerf2mesh_amd import _lib, build
    build.build(verbose=False)
    return _lib


def test_entry_points_refuse_before_any_launch(L):
    from nerf2mesh_amd.metrics import _TAPS
    p = 16                                                                 # a stand-in for a device pointer: nothing is dereferenced
    for P in (0, 10, 65, 1 << 20):
        with pytest.raises(RuntimeError, match=r"n2m_ssim_patches_forward failed \(-1\).*P must be 11 .. 64"):
            L.call("n2m_ssim_patches_forward", p, p, 2, P, 3, _TAPS, None, p, p, p, None)
        with pytest.raises(RuntimeError, match=r"n2m_ssim_patches_backward failed \(-1\).*P must be 11 .. 64"):
            L.call("n2m_ssim_patches_backward", p, p, p, 2, P, 3, _TAPS, p, p, None)
    for C in (0, 2, 4):
        with pytest.raises(RuntimeError, match=r"failed \(-1\).*C must be 1 or 3"):
            L.call("n2m_ssim_patches_forward", p, p, 2, 16, C, _TAPS, None, p, p, p, None)
        with pytest.raises(RuntimeError, match=r"failed \(-1\).*C must be 1 or 3"):
            L.call("n2m_ssim_patches_backward", p, p, p, 2, 16, C, _TAPS, p, p, None)
    with pytest.raises(RuntimeError, match=r"failed \(-1\).*B must be"):
        L.call("n2m_ssim_patches_forward", p, p, 0, 16, 3, _TAPS, None, p, p, p, None)
    with pytest.raises(RuntimeError, match=r"failed \(-1\).*B must be"):
        L.call("n2m_ssim_patches_backward", p, p, p, 0, 16, 3, _TAPS, p, p, None)
    for hole in (0, 1, 5, 7, 8, 9):                                        # dS (6) may be NULL: the path without a gradient request
        args = [p, p, 2, 16, 3, _TAPS, None, p, p, p]
        args[hole] = None
        with pytest.raises(RuntimeError, match=r"failed \(-2\).*NULL"):
            L.call("n2m_ssim_patches_forward", *args, None)
    for hole in (0, 1, 2, 6, 7, 8):
        args = [p, p, p, 2, 16, 3, _TAPS, p, p]
        args[hole] = None
        with pytest.raises(RuntimeError, match=r"failed \(-2\).*NULL"):
            L.call("n2m_ssim_patches_backward", *args, None)


def test_partials_count_is_patches_times_bands(L):
    lib = L.lib()
    assert lib.n2m_ssim_patches_partials(4, 10) == 0 and lib.n2m_ssim_patches_partials(4, 65) == 0
    for P in (11, 16, 17, 27, 32):                                         # up to 32 a patch is one workgroup
        assert lib.n2m_ssim_patches_partials(5, P) == 5
    assert lib.n2m_ssim_patches_partials(5, 33) == 5 * 4                   # 23 window rows in bands of 6
    assert lib.n2m_ssim_patches_partials(3, 64) == 3 * 9                   # 54 window rows in bands of 6


def test_shape_and_device_checks_of_the_python_layer():
    import torch
    from nerf2mesh_amd.metrics import ssim_patches
    with pytest.raises(ValueError, match="P must be 11 .. 64"):
        ssim_patches(torch.zeros(2, 10, 10, 3), torch.zeros(2, 10, 10, 3))
    with pytest.raises(ValueError, match="C must be 1 or 3"):
        ssim_patches(torch.zeros(2, 11, 11, 2), torch.zeros(2, 11, 11, 2))
    with pytest.raises(ValueError, match="one shape"):
        ssim_patches(torch.zeros(11, 11, 3), torch.zeros(11, 11, 3))
    with pytest.raises(RuntimeError, match="no host path"):
        ssim_patches(torch.zeros(2, 11, 11, 3), torch.zeros(2, 11, 11, 3))
