"""The CPU half of tests/test_gpu_window_kernels.py: the float32 restatements that set the reduction tolerances stay within
their own yardsticks (tests/window_kernels_utils.py), and the restatements mean what include/sdy_amd.h says."""
import pytest
import torch

import window_kernels_utils as wk


def test_float32_restatements_stay_within_their_yardsticks():
    """Every (kernel, M): the measured error of the float32 restatement against float64, relative to the float64 sum of the
    absolute terms, is no larger than the constant written down in window_kernels_utils.YARD -- and the constant is that
    measurement rounded up, not something looser (within 10 %)."""
    measured = wk.measure_yardsticks()
    assert set(measured) == set(wk.YARD)
    for key, err in measured.items():
        print(key, f"measured {err:.3e}  yardstick {wk.YARD[key]:.1e}  kernel tolerance {wk.KERNEL_FACTOR * wk.YARD[key]:.1e}")
        assert 0.0 < err <= wk.YARD[key], (key, err)
        assert wk.YARD[key] <= 1.1 * err, (key, err)


def test_gradient_restatement_is_torch_gradient():
    x = torch.randn(2, 3, 9, 116, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    gy, gx = torch.gradient(x, dim=(-2, -1))
    assert torch.equal(wk.gradient_magnitude(x), torch.sqrt(gy * gy + gx * gx))


@pytest.mark.parametrize("M", wk.ENS_M)
def test_ensemble_restatement_against_the_vectorised_formulas(M):
    """The sequential loops in float64 against the textbook expressions: unbiased variance, fair CRPS = mean |x - t| -
    sum_{i,j} |x_i - x_j| / (2 M (M - 1)), and for M = 1 variance 0 and CRPS = |x - t|."""
    H, W = wk.ENS_SHAPES[0]
    pred, truth, w = wk.ens_case(M, H, W)
    terms = wk.ens_terms(pred, truth, w, torch.float64)
    x, t, wd = pred.double(), truth.double(), w.double()
    mean = x.mean(dim=0)
    skill = (x - t).abs().mean(dim=0)
    if M > 1:
        var = x.var(dim=0, unbiased=True)
        crps = skill - (x[:, None] - x[None]).abs().sum(dim=(0, 1)) / (2 * M * (M - 1))
    else:
        var, crps = torch.zeros_like(t), skill
        assert bool((terms[..., 1] == 0).all()) and torch.equal(terms[..., 2], wd * (x[0] - t).abs())
    for q, want in enumerate((wd * (mean - t) ** 2, wd * var, wd * crps, wd * (mean - t), wd * mean, wd * mean ** 2, wd * t,
                              wd * t ** 2)):
        assert torch.allclose(terms[..., q], want, rtol=1e-11, atol=1e-13), q
    gm = torch.stack([wk.gradient_magnitude(x[m]) for m in range(M)]).sum(dim=0)
    assert torch.allclose(terms[..., 9], wd * gm, rtol=1e-12) and torch.equal(terms[..., 8], wd * wk.gradient_magnitude(t))
