"""The InstanceNorm statistics chain without a GPU: the CPU restatement of the producers' accumulation (float32 trees over
groups of 4, 64 and 128 values, float64 across groups: tests/instnorm_utils.py) must stay inside the derived bounds on every
case tests/test_gpu_instnorm.py runs, the G table is recounted from the accumulation structure, and the bound is shown to have
teeth: one missing or doubled pixel breaks it on every case.  The consumer bound is held against a float32 restatement of the
consumer's statements."""
import math

import numpy as np
import pytest

import instnorm_utils as iu

CASES = iu.PRODUCER_CASES
IDS = [c.id for c in CASES]


def test_g_table_is_the_structure_and_capped():
    assert set(iu.G_TABLE) == set(iu.ACCUM) == set(iu.PRODUCER_ACCUM.values())
    for kind, g in iu.G_TABLE.items():
        assert g == iu.g_from_structure(kind), kind
        assert max(g) <= iu.G_CAP
    # every producer of the chain has an entry, and the GPU cases cover every producer
    assert {c.producer for c in CASES} == set(iu.PRODUCER_ACCUM)
    assert {c.grid for c in CASES if c.producer != "irfft_lon_act"} == set(iu.GRIDS)
    assert {(c.grid[0] % 4, c.C) for c in CASES if c.producer == "irfft_lon_act"} >= {(2, 48), (3, 16), (0, 16)}
    assert all(c.B <= 3 and c.HW % 4 == 0 for c in CASES)


def test_restatement_sums_what_it_should():
    """On integers every float32 partial sum is exact: each restatement returns the exact sums, ragged tile and ring tail
    included (a structural check of the restatement itself)."""
    rng = np.random.default_rng(5)
    for kind, HW in (("quad", 216), ("row64", 216), ("row64", 8352), ("row128", 19 * 360)):
        v = rng.integers(-8, 9, size=(3, HW)).astype(np.float32)
        got = iu.emulate(kind, v)
        assert np.array_equal(got[:, 0], v.astype(np.float64).sum(-1)) and np.array_equal(got[:, 1], (v.astype(np.float64) ** 2).sum(-1))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_stays_inside_the_bounds(case):
    kind = iu.PRODUCER_ACCUM[case.producer]
    v = iu.synthetic_planes(case)
    off, const, zero = iu.roles(v.shape[1], case.gelu)
    got = iu.emulate(kind, v, case.grid[1])
    iu.check_stats(got, v, kind, case.id, off)
    if zero is not None:
        assert (got[:, zero] == 0).all()
    # the constant plane: its float64 variance is zero up to the bound, on either side of zero
    ref = iu.plane_sums(v[:, const], kind)
    assert (np.abs(got[:, const, 1] / case.HW - (got[:, const, 0] / case.HW) ** 2) <= ref.dvar).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_pixel_breaks_the_bound(case):
    """Statistics of the plane with its median-magnitude pixel missing, or counted twice, violate the sum or the sum-of-squares
    bound of the full plane, on every non-zero plane of every case."""
    kind = iu.PRODUCER_ACCUM[case.producer]
    v = iu.synthetic_planes(case)
    _, _, zero = iu.roles(v.shape[1], case.gelu)
    keep = [c for c in range(v.shape[1]) if c != zero]
    v = v[:, keep]
    ref = iu.plane_sums(v, kind)
    j = np.argsort(np.abs(v), axis=-1)[..., case.HW // 2]
    vj = np.take_along_axis(v, j[..., None], -1)[..., 0].astype(np.float64)
    missing = v.copy()
    np.put_along_axis(missing, j[..., None], 0.0, -1)
    got = iu.emulate(kind, missing, case.grid[1])
    rs, rq, _ = iu.stats_ratios(got, ref, case.HW)
    assert (np.maximum(rs, rq) > 1.0).all(), float(np.maximum(rs, rq).min())
    doubled = iu.emulate(kind, v, case.grid[1]) + np.stack([vj, vj * vj], -1)
    rs, rq, _ = iu.stats_ratios(doubled, ref, case.HW)
    assert (np.maximum(rs, rq) > 1.0).all(), float(np.maximum(rs, rq).min())


def _consumer_f32(S, S2, HW, gamma, beta, scale, shift, eps=iu.EPS):
    """The consumer's statements in numpy: float64 up to rstd, float32 from there (unfused products)."""
    f = np.float32
    mean = S / HW
    var = np.maximum(S2 / HW - mean * mean, 0.0)
    rstd = (1.0 / np.sqrt(var + np.float64(f(eps)))).astype(f)
    a = f(gamma)[None, :] * rstd
    d = f(beta)[None, :] - mean.astype(f) * a
    if scale is not None:
        sc = f(scale) + f(1.0)
        a, d = a * sc, d * sc + f(shift)
    return a, d


@pytest.mark.parametrize("with_ss", [False, True])
def test_consumer_bound_holds_for_its_float32_restatement(with_ss):
    rng = np.random.default_rng(11)
    B, Cc, HW = 3, 16, 8352
    x = iu.offset_planes(HW, n=12).reshape(3, 16, HW)
    x[0, 0] = iu.CONST_VALUE
    S, S2 = iu.exact_sums(x)
    S2[1, 1] = S[1, 1] ** 2 / HW * (1 - 1e-15)          # a variance that comes out negative: rstd = 1 / sqrt(eps)
    gamma, beta = rng.standard_normal(Cc).astype(np.float32), rng.standard_normal(Cc).astype(np.float32)
    scale = rng.standard_normal((B, Cc)).astype(np.float32) if with_ss else None
    shift = rng.standard_normal((B, Cc)).astype(np.float32) if with_ss else None
    ref = iu.consumer_ref(S, S2, HW, gamma, beta, scale, shift)
    a, d = _consumer_f32(S, S2, HW, gamma, beta, scale, shift)
    iu.check_coeffs(a, d, ref, f"float32 restatement ss={with_ss}")
    rstd = ref[0][1, 1] / (float(gamma[1]) * (1.0 + (float(scale[1, 1]) if with_ss else 0.0)))
    assert abs(rstd * math.sqrt(float(np.float32(iu.EPS))) - 1.0) < 1e-12
    # the bound is a rounding bound: a coefficient four float32 steps away is outside it
    off = a.astype(np.float64) * (1 + 8 * iu.U)
    with pytest.raises(AssertionError):
        iu.check_coeffs(off, d, ref, "shifted a")
