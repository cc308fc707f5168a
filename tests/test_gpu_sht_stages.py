"""The four stage entry points of the spherical-harmonic transform -- sdy_rfft_lon, sdy_legendre_fwd, sdy_legendre_inv,
sdy_irfft_lon (include/sdy_amd.h) -- one by one through the C ABI, every element against float64 explicit sums
(tests/sht_stages_utils.py holds the cases, the references and the tolerances; NOTEBOOK.md 7k the derivation).

FFT paths (csrc/fft.hip): the generic Stockham loop `<0,1>` at nlon = 4 .. 180 (every radix alone, in pairs and mixed), the
compile-time `<32,4>` and `<180,4>` kernels and fft360.hip, each with nlat % 4 = 0 .. 3 (ring tail of a workgroup), a channel
tail, a case that reaches the Nyquist bin and a truncated one.  Legendre back ends (csrc/capi.hip): LEG_PAR, LEG_H3,
LEG_GEMM_H3, LEG_GEMM_F32, each asserted through sdy_sht_plan_kernels so that a changed support predicate cannot turn the
table into copies of one path.  The query reports the plan's fft360 flag only: that a 360-point case with C % 16 != 0 runs
`<180,4>` and one with C % 16 == 0 runs fft360.hip rests on the launcher's own predicate, which no status code exposes.

Every output starts as NaN inside an allocation with NaN guard bands; a test asserts that no NaN is left where the kernel
writes, that the guard bands (and, for a truncated forward FFT, everything past mtr) are untouched, and that inputs are
unchanged."""
import ctypes as C

import pytest
import torch

import sht_stages_utils as su
from sht_stages_utils import Buf, bits_equal, within

pytestmark = pytest.mark.gpu


def lib_and_stream():
    import sdy_amd
    from sdy_amd._lib import current_stream

    return sdy_amd.lib, current_stream()


def plan_for(nlat, nlon, lmax, mmax, grid="equiangular", gemm_mode="h3"):
    from sdy_amd.sht import ShtPlan

    return ShtPlan.get(nlat, nlon, lmax, mmax, grid, torch.cuda.current_device(), gemm_mode)


def kernels_of(plan):
    lib, _ = lib_and_stream()
    out = (C.c_int * 2)()
    assert lib.sdy_sht_plan_kernels(plan.handle, C.byref(out)) == 0
    return out[0], out[1]


def fft_plan(case):
    plan = plan_for(case.nlat, case.nlon, case.nlat, case.mmax)
    assert plan.mtr == case.mtr
    if case.nlon == 360:
        assert kernels_of(plan)[1] == 1, "the 360-point cases expect fft360.hip to be enabled"
    return plan


# ---- forward FFT ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", su.FFT_CASES, ids=[c.id for c in su.FFT_CASES])
def test_rfft_lon(case):
    lib, stream = lib_and_stream()
    plan = fft_plan(case)
    B, Cc, K, N, mtr = case.B, case.C, case.nlat, case.nlon, case.mtr
    x, _, a, d, _ = su.fft_inputs(case)
    yard = su.YARD[("rfft", N)]
    xb = Buf((B, Cc, K, N), x)

    def run(ab, db, with_xn):
        Xf = Buf((mtr, K, B, 2, Cc))
        xn = Buf((B, Cc, K, N)) if with_xn else None
        rc = lib.sdy_rfft_lon(plan.handle, xb.ptr, ab.ptr if ab else None, db.ptr if db else None, xn.ptr if xn else None,
                              Xf.ptr, B, Cc, stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert Xf.guards_intact() and xb.unchanged(), "a guard band or the input was written"
        assert xn is None or xn.guards_intact()
        return Xf, xn

    # a = d = NULL: Xf against the float64 sum; xn_out is a bit-for-bit copy of x; Xf does not depend on xn_out
    ref, S = su.rfft_ref(x, mtr)
    Xf, xn = run(None, None, True)
    within(Xf.t.cpu().double(), ref, su.f32_bound(yard, S), f"rfft {case.id}")
    assert bits_equal(xn.t, xb.t), "xn_out is not a copy of x"
    Xf2, _ = run(None, None, False)
    assert bits_equal(Xf.t, Xf2.t), "Xf differs between xn_out set and NULL"

    # a, d set: xn_out = a x + d in either fp32 evaluation, Xf = transform of the xn_out the kernel stored
    ab, db = Buf((B * Cc,), a), Buf((B * Cc,), d)
    Xf, xn = run(ab, db, True)
    assert ab.unchanged() and db.unchanged()
    a64, d64 = a.double().view(B, Cc, 1, 1), d.double().view(B, Cc, 1, 1)
    ax = a64 * x.double()
    within(xn.t.cpu().double(), ax + d64, 2.0 ** -23 * (ax.abs() + d64.abs()).expand_as(ax), f"rfft xn_out {case.id}")
    ref, S = su.rfft_ref(xn.t.cpu(), mtr)
    within(Xf.t.cpu().double(), ref, su.f32_bound(yard, S), f"rfft affine {case.id}")
    Xf2, _ = run(ab, db, False)
    assert bits_equal(Xf.t, Xf2.t), "Xf (affine) differs between xn_out set and NULL"


# ---- inverse FFT ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", su.FFT_CASES, ids=[c.id for c in su.FFT_CASES])
def test_irfft_lon(case):
    lib, stream = lib_and_stream()
    plan = fft_plan(case)
    B, Cc, K, N, mtr = case.B, case.C, case.nlat, case.nlon, case.mtr
    _, Yf, _, _, bias = su.fft_inputs(case)
    Yb, bb = Buf((mtr, K, B, 2, Cc), Yf), Buf((Cc,), bias)

    def run(bias_buf):
        y = Buf((B, Cc, K, N))
        assert lib.sdy_irfft_lon(plan.handle, Yb.ptr, bias_buf.ptr if bias_buf else None, y.ptr, B, Cc, stream) == 0
        torch.cuda.synchronize()
        assert y.guards_intact() and Yb.unchanged() and bb.unchanged(), "a guard band or an input was written"
        return y.t.cpu()

    ref, S = su.irfft_ref(Yf, N)
    y0 = run(None)
    within(y0.double(), ref, su.f32_bound(su.YARD[("irfft", N)], S), f"irfft {case.id}")
    # the bias is added to the finished ring: the two runs differ by bias[c], rounded once
    y1 = run(bb)
    assert not bool(torch.isnan(y1).any())
    assert torch.equal(y1, y0 + bias.view(1, Cc, 1, 1)), "y with bias is not fl(y without bias + bias[c])"


# ---- Legendre ---------------------------------------------------------------------------------------------------------------
_LEG = [(c, g) for c in su.LEG_CASES for g in su.GRIDS]


@pytest.mark.parametrize("case,grid", _LEG, ids=[f"{c.name}-{g}" for c, g in _LEG])
def test_legendre(case, grid):
    lib, stream = lib_and_stream()
    plan = plan_for(case.nlat, case.nlon, case.lmax, case.mmax, grid, case.gemm_mode)
    leg, _ = kernels_of(plan)
    assert leg == case.leg, f"{case.name} was written for {su.LEG_NAME[case.leg]}, the plan runs {su.LEG_NAME[leg]}"
    mtr, K, L = plan.mtr, case.nlat, case.lmax
    assert mtr == case.mtr
    lgt = (torch.arange(mtr)[None, :] > torch.arange(L)[:, None])          # [l][m]: m > l
    for B, Cc in case.BC:
        N = 2 * B * Cc
        for direction in ("fwd", "inv"):
            X, ref, W = su.leg_case_io(case, grid, B, Cc, direction)
            S, sw, wsx, F = su.leg_sums(direction, W, X)
            xin = Buf(tuple(X.shape), X)
            out = Buf((L, mtr, N) if direction == "fwd" else (mtr, K, N))
            fn = lib.sdy_legendre_fwd if direction == "fwd" else lib.sdy_legendre_inv
            rc = fn(plan.handle, xin.ptr, out.ptr, B, Cc, stream)
            assert rc == 0, (rc, case.name, B, Cc, direction)
            torch.cuda.synchronize()
            assert out.guards_intact() and xin.unchanged(), "a guard band or the input was written"
            got = out.t.cpu().double()
            within(got, ref, su.leg_bound(case, direction, S, sw, wsx, F),
                   f"legendre {direction} {su.LEG_NAME[leg]} {case.name} {grid} B={B} C={Cc}")
            if direction == "fwd":
                assert bool((got[lgt] == 0).all()), "analysis: a coefficient with m > l is not an exact zero"


# ---- refusals: by status code, nothing launched -------------------------------------------------------------------------------
def test_refusals():
    lib, stream = lib_and_stream()
    h = C.c_void_p()
    assert lib.sdy_sht_plan_create_ex(16, 28, 16, 15, 0, 1, C.byref(h)) == su.SDY_ERR_UNSUPPORTED      # factor 7
    assert lib.sdy_sht_plan_create_ex(16, 30, 16, 16, 0, 1, C.byref(h)) == su.SDY_ERR_ALIGN
    assert lib.sdy_sht_plan_create_ex(16, 32, 16, 18, 0, 1, C.byref(h)) == su.SDY_ERR_ARG              # mmax > nlon / 2 + 1
    plan = plan_for(16, 32, 16, 17)
    B, K, N, mtr = 1, 16, 32, plan.mtr

    def bufs(Cc, offset=0):
        return (Buf((B, Cc, K, N), torch.zeros(B, Cc, K, N), offset), Buf((B, Cc, K, N), None, offset),
                Buf((mtr, K, B, 2, Cc), None, offset), Buf((Cc,), torch.zeros(Cc)))

    x, y, Xf, v = bufs(8)
    calls = []
    calls.append((su.SDY_ERR_ARG, lambda: lib.sdy_rfft_lon(plan.handle, x.ptr, v.ptr, None, None, Xf.ptr, B, 8, stream)))
    calls.append((su.SDY_ERR_ARG, lambda: lib.sdy_rfft_lon(plan.handle, x.ptr, None, v.ptr, None, Xf.ptr, B, 8, stream)))
    # C % 4: the float4 runs of four channels
    x6, y6, Xf6, v6 = bufs(6)
    calls.append((su.SDY_ERR_ALIGN, lambda: lib.sdy_rfft_lon(plan.handle, x6.ptr, None, None, None, Xf6.ptr, B, 6, stream)))
    calls.append((su.SDY_ERR_ALIGN, lambda: lib.sdy_irfft_lon(plan.handle, Xf6.ptr, None, y6.ptr, B, 6, stream)))
    # a pointer one float off a 16-byte boundary, one argument at a time
    xo, yo, Xfo, _ = bufs(8, offset=1)
    calls.append((su.SDY_ERR_ALIGN, lambda: lib.sdy_rfft_lon(plan.handle, xo.ptr, None, None, None, Xf.ptr, B, 8, stream)))
    calls.append((su.SDY_ERR_ALIGN, lambda: lib.sdy_rfft_lon(plan.handle, x.ptr, None, None, yo.ptr, Xf.ptr, B, 8, stream)))
    calls.append((su.SDY_ERR_ALIGN, lambda: lib.sdy_rfft_lon(plan.handle, x.ptr, None, None, None, Xfo.ptr, B, 8, stream)))
    calls.append((su.SDY_ERR_ALIGN, lambda: lib.sdy_irfft_lon(plan.handle, Xfo.ptr, None, y.ptr, B, 8, stream)))
    calls.append((su.SDY_ERR_ALIGN, lambda: lib.sdy_irfft_lon(plan.handle, Xf.ptr, None, yo.ptr, B, 8, stream)))
    # odd C in the Legendre stages
    cs = Buf((16, mtr, 2 * B * 8))
    calls.append((su.SDY_ERR_ALIGN, lambda: lib.sdy_legendre_fwd(plan.handle, Xf.ptr, cs.ptr, B, 3, stream)))
    calls.append((su.SDY_ERR_ALIGN, lambda: lib.sdy_legendre_inv(plan.handle, cs.ptr, Xf.ptr, B, 3, stream)))
    for i, (want, call) in enumerate(calls):
        assert call() == want, i
    torch.cuda.synchronize()
    for b in (x, y, Xf, v, x6, y6, Xf6, v6, xo, yo, Xfo, cs):
        assert b.unchanged(), "a refused call wrote something"
