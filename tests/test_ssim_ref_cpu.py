"""The SSIM reference model (tests/ssim_ref.py) against the definition itself, on the CPU: a literal double loop over windows, the two closed
forms (ssim(x, x) = 1, two all-zero images give 1) and central differences for the float64 autograd gradient the GPU tests compare with."""
import numpy as np
import pytest
import torch

import ssim_ref as R


def test_taps_are_the_normalised_gaussian():
    t = R.taps64()
    assert t.shape == (11,) and abs(t.sum() - 1.0) < 1e-15
    assert np.array_equal(t, t[::-1]) and t.argmax() == 5
    assert t[4] / t[5] == pytest.approx(np.exp(-1 / (2 * 1.5 ** 2)), rel=1e-14)


@pytest.mark.parametrize("shape", [(11, 11), (12, 13)])
@pytest.mark.parametrize("C", [1, 3])
def test_model_equals_the_double_loop(shape, C):
    gen = torch.Generator().manual_seed(5)
    x, y = torch.rand(*shape, C, generator=gen), torch.rand(*shape, C, generator=gen)
    mean, smap = R.ssim_model(x, y)
    ref_mean, ref_map = R.ssim_loops(x, y)
    assert tuple(smap.shape) == (shape[0] - 10, shape[1] - 10, C)
    # two float64 evaluations of one 121-term sum in different orders: a few ulp of the moments, amplified by at most 1 / C2 ~ 1e3
    assert np.abs(smap.numpy() - ref_map).max() < 1e-12
    assert abs(float(mean) - ref_mean) < 1e-12


@pytest.mark.parametrize("C", [1, 3])
def test_identical_images_give_one(C):
    x = torch.rand(14, 17, C, generator=torch.Generator().manual_seed(1))
    mean, smap = R.ssim_model(x, x.clone())
    assert float(mean) == pytest.approx(1.0, abs=1e-14) and float((smap - 1).abs().max()) < 1e-13
    m32, s32 = R.ssim_model(x, x.clone(), torch.float32)
    assert float(m32) == pytest.approx(1.0, abs=1e-6)


def test_two_zero_images_give_one():
    z = torch.zeros(11, 13, 3)
    mean, smap = R.ssim_model(z, z)
    assert float(mean) == 1.0 and bool((smap == 1).all())        # C1 C2 / (C1 C2)
    assert float(R.ssim_model(z, z, torch.float32)[0]) == 1.0


def test_float64_gradient_agrees_with_central_differences():
    gen = torch.Generator().manual_seed(2)
    x, y = torch.rand(12, 13, 3, generator=gen).double(), torch.rand(12, 13, 3, generator=gen).double()
    g = R.ssim_model_grad(x, y, g=3.0)
    assert g.shape == x.shape and g.dtype == torch.float64
    h = 1e-6
    idx = torch.randperm(x.numel(), generator=gen)[:40]
    for i in idx.tolist():
        e = torch.zeros(x.numel(), dtype=torch.float64)
        e[i] = h
        e = e.view_as(x)
        fd = 3.0 * (float(R.ssim_model(x + e, y)[0]) - float(R.ssim_model(x - e, y)[0])) / (2 * h)
        # central differences: truncation h^2 f''' / 6 ~ 1e-12 * O(1e2), rounding eps / h ~ 1e-10
        assert abs(fd - float(g.view(-1)[i])) < 1e-7 * max(1.0, float(g.abs().max())), (i, fd, float(g.view(-1)[i]))


def test_case_set_is_what_the_gpu_tests_state():
    assert R.SHAPES == [(11, 11), (11, 43), (43, 11), (42, 75), (76, 43)] and R.CHANNELS == [1, 3] and len(R.INPUTS) == 5
    x, y = R.make_pair((11, 43), 3, "inverse")
    assert torch.equal(y, 1 - x) and x.dtype == torch.float32
    a, b = R.make_pair((11, 43), 3, "random")
    assert torch.equal(a, x) and not torch.equal(a, b)            # every kind of one shape shares x
