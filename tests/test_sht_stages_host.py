"""The CPU half of tests/test_gpu_sht_stages.py: the float32 restatements that set the tolerances of the spherical-harmonic
stage kernels stay within their own yardsticks and within every bound tests/sht_stages_utils.py states, the float64
references mean what include/sdy_amd.h says, and plan creation refuses what it cannot transform before touching a device."""
import ctypes as C
import math

import pytest
import torch

import sht_stages_utils as su


@pytest.fixture(scope="module")
def measured():
    return su.measure_yardsticks()


def test_float32_restatements_stay_within_their_yardsticks(measured):
    """Every stored constant is at least the re-measured error of its float32 restatement and at most twice that."""
    assert set(measured) == set(su.YARD), sorted(set(measured) ^ set(su.YARD), key=str)
    for key, err in sorted(measured.items(), key=str):
        print(key, f"measured {err:.3e}  yardstick {su.YARD[key]:.1e}  kernel tolerance {su.KERNEL_FACTOR * su.YARD[key]:.1e}")
        assert 0.0 < err <= su.YARD[key], (key, err)
        assert su.YARD[key] <= 2.0 * err, (key, err)


def test_float32_restatements_stay_within_every_bound():
    """All cases, both directions: the float32 restatement is inside the bound its kernel is held to (fp32: yardstick x S
    without the kernel factor; split-fp16: the derived bound, which must not be tighter than plain float32 arithmetic)."""
    for case in su.FFT_CASES:
        x, Yf, _, _, _ = su.fft_inputs(case)
        ref, S = su.rfft_ref(x, case.mtr)
        assert bool(((su.rfft_f32(x, case.mtr).double() - ref).abs() <= su.YARD[("rfft", case.nlon)] * S).all()), case.id
        ref, S = su.irfft_ref(Yf, case.nlon)
        assert bool(((su.irfft_f32(Yf, case.nlon).double() - ref).abs() <= su.YARD[("irfft", case.nlon)] * S).all()), case.id
    for case in su.LEG_CASES:
        for grid in su.GRIDS:
            for B, Cc in case.BC:
                for direction in ("fwd", "inv"):
                    X, ref, W = su.leg_case_io(case, grid, B, Cc, direction)
                    S, sw, wsx, F = su.leg_sums(direction, W, X)
                    err = ((su.leg_fwd if direction == "fwd" else su.leg_inv)(W, X, torch.float32).double() - ref).abs()
                    what = (case.name, grid, B, Cc, direction)
                    assert bool((err <= su.YARD[(direction, case.name)] * S + F).all()), what
                    assert bool((err <= su.leg_bound(case, direction, S, sw, wsx, F)).all()), what


def test_split_constants_follow_from_the_number_formats():
    """fp16 keeps 11 significant bits and its subnormals are spaced 2^-24 (checked on torch's float16), which is what
    SPLIT_REL and the two floors are built from."""
    assert torch.finfo(torch.float16).eps == 2.0 ** -10 and torch.finfo(torch.float16).smallest_normal == 2.0 ** -14
    g = torch.Generator().manual_seed(5)
    v = torch.randn(4096, generator=g).double() * torch.logspace(-6, 3, 4096, dtype=torch.float64)
    t = su.ACT_SX * v
    hi = t.to(torch.float16).double()
    lo = (t - hi).to(torch.float16).double()
    assert bool((((hi + lo) / su.ACT_SX - v).abs() <= 2.0 ** -22 * v.abs() + su.SPLIT_ACT_FLOOR).all())
    assert su.SPLIT_REL == 3 * 2.0 ** -22 and su.SPLIT_TAB_FLOOR == 2.0 ** -37


@pytest.mark.parametrize("nlon,mtr", [(4, 3), (12, 7), (20, 5), (64, 33), (360, 181), (360, 18)])
def test_fft_references_against_numpy_style_transforms(nlon, mtr):
    """The explicit float64 sums against torch.fft in float64 (which is given zeroed DC / Nyquist imaginary parts)."""
    g = torch.Generator().manual_seed(nlon + mtr)
    x = torch.randn(2, 4, 3, nlon, generator=g, dtype=torch.float64)
    ref, S = su.rfft_ref(x, mtr)
    X = 2.0 * math.pi * torch.fft.rfft(x, dim=-1, norm="forward")[..., :mtr]
    assert torch.allclose(ref, su.to_spec_layout(X.real, X.imag), rtol=0, atol=1e-13)
    assert bool((S > 0).all()) and bool((ref.abs() <= S * (1 + 1e-12)).all())
    Yf = torch.randn(mtr, 3, 2, 2, 4, generator=g, dtype=torch.float64)
    y, S = su.irfft_ref(Yf, nlon)
    Y = torch.zeros(2, 4, 3, nlon // 2 + 1, dtype=torch.complex128)
    Y[..., :mtr] = torch.complex(Yf[:, :, :, 0].permute(2, 3, 1, 0), Yf[:, :, :, 1].permute(2, 3, 1, 0))
    Y[..., 0] = Y[..., 0].real.to(torch.complex128)
    Y[..., -1] = Y[..., -1].real.to(torch.complex128)
    assert torch.allclose(y, torch.fft.irfft(Y, n=nlon, dim=-1, norm="forward"), rtol=0, atol=1e-11)
    assert bool((y.abs() <= S * (1 + 1e-12)).all())


def test_legendre_tables_are_triangular_and_round_trip():
    """m > l entries of both tables are exact zeros, and synthesis followed by analysis is the identity on a legendre-gauss
    grid up to the 2 pi that the forward FFT carries (float64 einsums of the float32 tables: 1e-6)."""
    Wq, P = su.leg_tables(17, 32, 17, 17, "legendre-gauss")
    m, l = torch.arange(17)[:, None], torch.arange(17)[None, :]
    assert bool((Wq[(m > l)] == 0).all()) and bool((P[(m > l)] == 0).all())
    g = torch.Generator().manual_seed(1)
    Cs = torch.randn(17, 17, 4, generator=g, dtype=torch.float64) * (l.T >= m.T)[:, :, None]
    back = 2.0 * math.pi * su.leg_fwd(Wq, su.leg_inv(P, Cs))
    assert torch.allclose(back, Cs, rtol=0, atol=1e-6)


def test_cases_cover_what_they_claim():
    paths = {}
    for c in su.FFT_CASES:
        paths.setdefault(c.path, []).append(c)
        assert c.nlon % 4 == 0 and c.C % 4 == 0 and c.mmax <= c.nlon // 2 + 1
    for p in ("n32", "n180", "fft360"):
        assert {c.nlat % 4 for c in paths[p]} == {0, 1, 2, 3}, p
    for p, cs in paths.items():
        assert any(c.mtr == c.nlon // 2 + 1 for c in cs) and any(c.mtr < c.nlon // 2 + 1 for c in cs), p
    assert {c.nlon for c in paths["generic"]} == {4, 8, 12, 20, 40, 72, 100, 120, 180}
    assert {c.C for c in paths["generic"]} == {4, 20} and {c.B for c in paths["generic"]} == {1, 3}
    assert {c.C % 16 for c in paths["fft360"]} == {0} and all(c.C % 16 for c in paths["n180"])
    for leg in (su.LEG_PAR, su.LEG_H3, su.LEG_GEMM_H3):
        assert any((3, 22) in c.BC for c in su.LEG_CASES if c.leg == leg), su.LEG_NAME[leg]


def test_plan_kernels_refuses_a_null_plan():
    """(The plan-creation refusals without a device are in tests/test_capi_cpu.py.)"""
    import sdy_amd

    lib = sdy_amd.lib
    out = (C.c_int * 2)()
    assert lib.sdy_sht_plan_kernels(None, C.byref(out)) == su.SDY_ERR_ARG
