"""CPU: the SSIM entry points refuse bad arguments on the host, before any launch (no GPU needed), and the Python layer's taps are the
reference model's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ssim_ref as R   # noqa: E402


@pytest.fixture(scope="module")
def L():
    from nerf2mesh_amd import _lib, build
    build.build(verbose=False)
    return _lib


def test_entry_points_refuse_before_any_launch(L):
    from nerf2mesh_amd.metrics import _TAPS
    p = 16                                                                 # a stand-in for a device pointer: nothing is dereferenced
    for H, W in ((10, 11), (11, 10), (0, 0)):
        with pytest.raises(RuntimeError, match=r"failed \(-1\).*at least 11"):
            L.call("n2m_ssim_forward", p, p, H, W, 3, _TAPS, None, None, p, p, None)
        with pytest.raises(RuntimeError, match=r"failed \(-1\).*at least 11"):
            L.call("n2m_ssim_backward", p, p, p, H, W, 3, _TAPS, p, p, None)
    for C in (0, 2, 4):
        with pytest.raises(RuntimeError, match=r"failed \(-1\).*C must be 1 or 3"):
            L.call("n2m_ssim_forward", p, p, 11, 11, C, _TAPS, None, None, p, p, None)
        with pytest.raises(RuntimeError, match=r"failed \(-1\).*C must be 1 or 3"):
            L.call("n2m_ssim_backward", p, p, p, 11, 11, C, _TAPS, p, p, None)
    for args in ((None, p, 11, 11, 3, _TAPS, None, None, p, p), (p, None, 11, 11, 3, _TAPS, None, None, p, p), (p, p, 11, 11, 3, None, None, None, p, p),
                 (p, p, 11, 11, 3, _TAPS, None, None, None, p), (p, p, 11, 11, 3, _TAPS, None, None, p, None)):
        with pytest.raises(RuntimeError, match=r"failed \(-2\).*NULL"):
            L.call("n2m_ssim_forward", *args, None)
    for hole in (0, 1, 2, 6, 7, 8):
        args = [p, p, p, 11, 11, 3, _TAPS, p, p]
        args[hole] = None
        with pytest.raises(RuntimeError, match=r"failed \(-2\).*NULL"):
            L.call("n2m_ssim_backward", *args, None)


def test_partials_count_is_the_tile_count(L):
    lib = L.lib()
    assert lib.n2m_ssim_partials(11, 11) == 1 and lib.n2m_ssim_partials(10, 64) == 0
    assert lib.n2m_ssim_partials(42, 75) == 3 * 2 and lib.n2m_ssim_partials(76, 43) == 2 * 5        # maps of 32 x 65 and 66 x 33, tiles of 16 x 32
    assert lib.n2m_ssim_partials(800, 800) == 25 * 50


def test_python_taps_are_the_models_rounded_once():
    from nerf2mesh_amd import metrics
    assert np.array_equal(metrics.gaussian_taps(), R.taps64())
    assert np.array_equal(np.array(list(metrics._TAPS), dtype=np.float32), R.taps64().astype(np.float32))


def test_shape_and_device_checks_of_the_python_layer():
    import torch
    from nerf2mesh_amd.metrics import ssim
    with pytest.raises(ValueError, match="at least 11"):
        ssim(torch.zeros(10, 11, 3), torch.zeros(10, 11, 3))
    with pytest.raises(ValueError, match="C must be 1 or 3"):
        ssim(torch.zeros(11, 11, 2), torch.zeros(11, 11, 2))
    with pytest.raises(RuntimeError, match="no host path"):
        ssim(torch.zeros(11, 11, 3), torch.zeros(11, 11, 3))


def test_option_default_and_override():
    from nerf2mesh_amd.options import make_options
    assert make_options().lambda_ssim == 0 and make_options(lambda_ssim=0.2).lambda_ssim == 0.2
