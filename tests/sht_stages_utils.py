"""Cases, float64 references, float32 restatements and tolerances of the four spherical-harmonic stage entry points
(sdy_rfft_lon, sdy_legendre_fwd, sdy_legendre_inv, sdy_irfft_lon; include/sdy_amd.h).  Shared by
tests/test_gpu_sht_stages.py (the kernels, every element against float64) and tests/test_sht_stages_host.py (the constants
below, re-measured on the CPU).

Layouts (csrc/fft.hip, include/sdy_amd.h):  x, y (B, C, nlat, nlon);  Xf, Yf [m][k][b][ri][c], m < mtr;  Cs [l][m][b][ri][c].

Every output element is a sum; its error is taken relative to the float64 sum of the ABSOLUTE values of that element's own
terms (`S` below), so a coefficient whose table entries are small, a tail ring and a tail channel are held as tightly as any
other element:
    forward FFT   S = (2 pi / N) sum_w |x[w]|
    inverse FFT   S = sum_m c_m (|Re Y[m] cos| + |Im Y[m] sin|),  c_m = 1 for DC and Nyquist, else 2
    Legendre      S = sum_k |W[m][l][k]| |X[m][k][n]|

fp32 kernels (generic / <32> / <180> FFT, fft360, LEG_GEMM_F32): |err| <= KERNEL_FACTOR * (YARD * S + F), F = 0 for the FFTs and
float32's underflow floor for the Legendre stages (`leg_sums`).  YARD is not chosen: it is
the largest |err| / S of a plain float32 restatement (torch.fft in float32; a float32 einsum) on exactly the inputs the GPU
tests use, rounded UP to two digits (`python tests/sht_stages_utils.py` prints the table; NOTEBOOK.md 7k).  The factor 4 covers
another summation order and the unfused twiddle products.

Split-fp16 kernels (LEG_PAR, LEG_H3, LEG_GEMM_H3) are not fp32 arithmetic; their bound is derived from csrc/common.h, not
measured on them (`split_bound`):
  * an operand v, scaled by a power of two t, is kept as hi = fp16(t v), lo = fp16(t v - hi).  fp16 rounds to 11 bits, so
    |t v - hi| <= 2^-11 |t v| and the kept value errs by 2^-22 |v| -- unless lo (or hi) is an fp16 subnormal (spacing
    2^-24), where the error is absolute: 2^-25 / t.  Together |dv| <= 2^-22 |v| + 2^-25 / t.
  * activations: t = SDY_ACT_SX = 16 (floor 2^-29).  Tables: t = sdy_h3_scale puts max |W| in [2^12, 2^13), so
    t >= 2^12 / Wmax and the floor is 2^-37 Wmax.
  * three passes hi*hi + hi*lo + lo*hi drop lo*lo, |lo_w lo_x| <= 2^-22 |w x|; the fp16 products are exact in the fp32
    accumulator.
  so per term |w x - computed| <= 3 * 2^-22 |w x| + 2^-29 |w| + 2^-37 Wmax |x|, and per element
      |err| <= (SPLIT_REL + KERNEL_FACTOR * YARD) S + SPLIT_ACT_FLOOR sum_k |W| + SPLIT_TAB_FLOOR Wmax sum_k |X|
  with the fp32 accumulation of the products (and the fp32 fold / unfold of the two hemispheres in leg_par.hip) under the
  same yardstick as the fp32 GEMM.  sum_k |X| runs over the terms the triangle l >= m keeps."""
import ctypes as C
import functools
import math
import zlib
from typing import NamedTuple

import numpy as np
import torch

KERNEL_FACTOR = 4.0
ACT_SX = 16.0                                  # SDY_ACT_SX, csrc/common.h
SPLIT_REL = 3.0 * 2.0 ** -22                   # two operand splits + the dropped lo*lo pass
SPLIT_ACT_FLOOR = 2.0 ** -25 / ACT_SX          # x sum |W|
SPLIT_TAB_FLOOR = 2.0 ** -25 / 2.0 ** 12       # x Wmax sum |X|   (sdy_h3_scale: scale >= 2^12 / Wmax)
FLT_MIN = 2.0 ** -126                          # smallest normal float32
LEG_PAR, LEG_H3, LEG_GEMM_H3, LEG_GEMM_F32 = 0, 1, 2, 3
LEG_NAME = {LEG_PAR: "LEG_PAR", LEG_H3: "LEG_H3", LEG_GEMM_H3: "LEG_GEMM_H3", LEG_GEMM_F32: "LEG_GEMM_F32"}
GRIDS = ("equiangular", "legendre-gauss")
SDY_ERR_ARG, SDY_ERR_UNSUPPORTED, SDY_ERR_ALIGN = -1, -2, -3


# ---- cases ------------------------------------------------------------------------------------------------------------------
class FftCase(NamedTuple):
    path: str        # "generic" | "n32" | "n180" | "fft360"
    nlat: int
    nlon: int
    mmax: int        # lmax = nlat, so mtr = min(mmax, nlat)
    B: int
    C: int

    @property
    def mtr(self):
        return min(self.mmax, self.nlat)

    @property
    def id(self):
        return f"{self.path}-{self.nlat}x{self.nlon}-m{self.mmax}-B{self.B}-C{self.C}"


def _fft_cases():
    out = []
    # generic Stockham loop: n = nlon / 2 -> radices [2] [4] [2,3] [2,5] [4,5] [4,3,3] [2,5,5] [4,3,5] [2,3,3,5]; nlat = n + 1 lets
    # mtr reach the Nyquist bin; C = 4 is below one 16-channel block, C = 20 one block plus a tail
    for nlon in (4, 8, 12, 20, 40, 72, 100, 120, 180):
        n = nlon // 2
        out += [FftCase("generic", n + 1, nlon, n + 1, 3, 4), FftCase("generic", n + 1, nlon, n + 1, 1, 20)]
    out.append(FftCase("generic", 18, 120, 18, 3, 20))                       # truncated: mtr = 18 < 61
    # compile-time paths walk four rings per workgroup: nlat % 4 = 1, 2, 3, 0; the small grids are the truncated ones
    out += [FftCase("n32", 33, 64, 33, 3, 20), FftCase("n32", 18, 64, 18, 1, 4), FftCase("n32", 19, 64, 19, 3, 16),
            FftCase("n32", 20, 64, 20, 1, 20)]
    out += [FftCase("n180", 181, 360, 181, 1, 24), FftCase("n180", 181, 360, 181, 3, 8), FftCase("n180", 18, 360, 18, 3, 24),
            FftCase("n180", 19, 360, 19, 1, 8), FftCase("n180", 20, 360, 20, 1, 24)]
    out += [FftCase("fft360", 181, 360, 181, 1, 48), FftCase("fft360", 181, 360, 181, 3, 16),
            FftCase("fft360", 18, 360, 18, 3, 48), FftCase("fft360", 19, 360, 19, 1, 16), FftCase("fft360", 20, 360, 20, 1, 48)]
    return tuple(out)


FFT_CASES = _fft_cases()


class LegCase(NamedTuple):
    name: str
    leg: int         # the back end the shape was written for
    nlat: int
    nlon: int
    lmax: int
    mmax: int
    gemm_mode: str   # "h3" | "f32"
    BC: tuple        # ((B, C), ...): N = 2 B C columns

    @property
    def mtr(self):
        return min(self.mmax, self.lmax)


_BC = ((1, 2), (1, 6), (2, 16))            # C even is the contract: N = 4, 12, 64
_BC_TAIL = ((3, 22),)                      # N = 132 = 2 * 64 + 4: the column-tile tail
LEG_CASES = (
    LegCase("par16", LEG_PAR, 16, 32, 16, 17, "h3", _BC + _BC_TAIL),        # the smallest leg_par accepts
    LegCase("par180", LEG_PAR, 180, 360, 180, 181, "h3", ((1, 4),)),
    LegCase("par192", LEG_PAR, 192, 360, 120, 40, "h3", _BC),
    LegCase("h3_17", LEG_H3, 17, 32, 17, 17, "h3", _BC + _BC_TAIL),
    LegCase("h3_15", LEG_H3, 15, 32, 15, 15, "h3", _BC),                    # below leg_par's minimum
    LegCase("h3_191", LEG_H3, 191, 360, 100, 50, "h3", _BC),
    LegCase("gemm196", LEG_GEMM_H3, 196, 16, 196, 9, "h3", _BC + _BC_TAIL),  # mtr = 9 keeps it tiny
    LegCase("gemm200", LEG_GEMM_H3, 64, 16, 200, 9, "h3", _BC),
    LegCase("f32_17", LEG_GEMM_F32, 17, 32, 17, 17, "f32", _BC),
    LegCase("f32_180", LEG_GEMM_F32, 180, 360, 180, 181, "f32", ((1, 4),)),
    LegCase("f32_196", LEG_GEMM_F32, 196, 16, 196, 9, "f32", _BC),
)

# Measured by measure_yardsticks() on the CPU (torch float32 against float64 on the inputs below), rounded UP to two digits.
# FFT: (direction, nlon); Legendre: (direction, case name), the largest over both grids and every (B, C) of the case.
YARD = {
    ('fwd', 'f32_17'): 2.1e-07,   # measured 2.026e-07
    ('fwd', 'f32_180'): 3.1e-07,   # measured 3.071e-07
    ('fwd', 'f32_196'): 3.0e-07,   # measured 2.956e-07
    ('fwd', 'gemm196'): 3.2e-07,   # measured 3.179e-07
    ('fwd', 'gemm200'): 2.9e-07,   # measured 2.812e-07
    ('fwd', 'h3_15'): 1.9e-07,   # measured 1.842e-07
    ('fwd', 'h3_17'): 2.3e-07,   # measured 2.296e-07
    ('fwd', 'h3_191'): 4.1e-07,   # measured 4.026e-07
    ('fwd', 'par16'): 2.3e-07,   # measured 2.251e-07
    ('fwd', 'par180'): 3.0e-07,   # measured 2.954e-07
    ('fwd', 'par192'): 3.8e-07,   # measured 3.723e-07
    ('inv', 'f32_17'): 1.8e-07,   # measured 1.704e-07
    ('inv', 'f32_180'): 3.4e-07,   # measured 3.337e-07
    ('inv', 'f32_196'): 2.5e-07,   # measured 2.462e-07
    ('inv', 'gemm196'): 2.9e-07,   # measured 2.827e-07
    ('inv', 'gemm200'): 2.5e-07,   # measured 2.403e-07
    ('inv', 'h3_15'): 1.8e-07,   # measured 1.718e-07
    ('inv', 'h3_17'): 1.8e-07,   # measured 1.764e-07
    ('inv', 'h3_191'): 2.9e-07,   # measured 2.861e-07
    ('inv', 'par16'): 1.7e-07,   # measured 1.656e-07
    ('inv', 'par180'): 2.9e-07,   # measured 2.803e-07
    ('inv', 'par192'): 3.3e-07,   # measured 3.259e-07
    ('irfft', 100): 8.2e-08,   # measured 8.142e-08
    ('irfft', 12): 9.7e-08,   # measured 9.624e-08
    ('irfft', 120): 1.4e-07,   # measured 1.341e-07
    ('irfft', 180): 8.1e-08,   # measured 8.088e-08
    ('irfft', 20): 1.6e-07,   # measured 1.512e-07
    ('irfft', 360): 1.9e-07,   # measured 1.838e-07
    ('irfft', 4): 7.2e-08,   # measured 7.105e-08
    ('irfft', 40): 1.2e-07,   # measured 1.144e-07
    ('irfft', 64): 1.4e-07,   # measured 1.309e-07
    ('irfft', 72): 9.8e-08,   # measured 9.718e-08
    ('irfft', 8): 1.1e-07,   # measured 1.049e-07
    ('rfft', 100): 6.9e-08,   # measured 6.856e-08
    ('rfft', 12): 1.4e-07,   # measured 1.365e-07
    ('rfft', 120): 7.4e-08,   # measured 7.352e-08
    ('rfft', 180): 6.5e-08,   # measured 6.444e-08
    ('rfft', 20): 1.7e-07,   # measured 1.604e-07
    ('rfft', 360): 6.0e-08,   # measured 5.977e-08
    ('rfft', 4): 1.3e-07,   # measured 1.252e-07
    ('rfft', 40): 8.3e-08,   # measured 8.288e-08
    ('rfft', 64): 6.5e-08,   # measured 6.491e-08
    ('rfft', 72): 6.5e-08,   # measured 6.439e-08
    ('rfft', 8): 1.3e-07,   # measured 1.278e-07
}


def round_up2(v):
    """v rounded up to two significant digits."""
    e = math.floor(math.log10(v)) - 1
    return math.ceil(v / 10.0 ** e - 1e-9) * 10.0 ** e


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator(device="cpu").manual_seed(zlib.crc32(repr(key).encode()))


@functools.lru_cache(maxsize=None)
def fft_inputs(case: FftCase):
    """x (B, C, K, N) and a dense Yf (mtr, K, B, 2, C) with non-zero imaginary parts in bin 0 and the Nyquist bin; a, d (B*C)
    of magnitude O(1) and mixed signs with a[0] = 0 and d[1] = 0; bias (C)."""
    g = _gen(1, case.nlat, case.nlon, case.mmax, case.B, case.C)
    x = torch.randn(case.B, case.C, case.nlat, case.nlon, generator=g)
    Yf = torch.randn(case.mtr, case.nlat, case.B, 2, case.C, generator=g)
    a = torch.randn(case.B * case.C, generator=g) * 1.5
    d = torch.randn(case.B * case.C, generator=g) * 1.5
    a[0], d[1] = 0.0, 0.0
    bias = torch.randn(case.C, generator=g)
    return x, Yf, a, d, bias


@functools.lru_cache(maxsize=None)
def leg_inputs(case: LegCase, B, Cc):
    """Xf (mtr, nlat, N) and Cs (lmax, mtr, N), N = 2 B C: normals of magnitude O(1), the last column scaled by 2^-10 (below
    2^-3 / SDY_ACT_SX, where the split keeps an absolute precision only).  Cs is dense: entries with m > l are finite values
    that the synthesis must not use."""
    g = _gen(2, case.name, B, Cc)
    N = 2 * B * Cc
    Xf = torch.randn(case.mtr, case.nlat, N, generator=g)
    Cs = torch.randn(case.lmax, case.mtr, N, generator=g)
    Xf[..., -1] *= 2.0 ** -10
    Cs[..., -1] *= 2.0 ** -10
    return Xf, Cs


# ---- FFT: float64 explicit sums ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _trig(N, mtr):
    """cos, sin of 2 pi m w / N as (N, mtr) float64, the angle reduced in integers first."""
    mw = (torch.arange(N)[:, None] * torch.arange(mtr)[None, :]) % N
    ang = mw.double() * (2.0 * math.pi / N)
    c, s = torch.cos(ang), torch.sin(ang)
    s[(2 * mw) % N == 0] = 0.0        # sin(0) and sin(pi) exactly
    c[(4 * mw) % N == 0] = torch.round(c[(4 * mw) % N == 0])   # cos(pi/2) = 0 exactly, cos(0), cos(pi) = +-1
    return c, s


def to_spec_layout(re, im):
    """(B, C, K, mtr) real and imaginary parts -> [m][k][b][ri][c]."""
    return torch.stack([re.permute(3, 2, 0, 1), im.permute(3, 2, 0, 1)], dim=3).contiguous()


def rfft_ref(x, mtr):
    """X[m] = (2 pi / N) sum_w x[w] e^{-2 pi i m w / N}, m < mtr, from x (B, C, K, N) in float64: (Xf, S) in the layout
    [m][k][b][ri][c]; S = (2 pi / N) sum_w |x[w]| is the same for every m and for both parts."""
    x = x.double()
    N = x.shape[-1]
    c, s = _trig(N, mtr)
    sc = 2.0 * math.pi / N
    re, im = sc * (x @ c), -sc * (x @ s)
    S = (sc * x.abs().sum(dim=-1, keepdim=True)).expand_as(re)
    return to_spec_layout(re, im), to_spec_layout(S, S)


def _irfft_weights(N, mtr):
    cm = torch.full((mtr,), 2.0, dtype=torch.float64)
    cm[0] = 1.0
    if mtr > N // 2:
        cm[N // 2] = 1.0
    return cm


def irfft_ref(Yf, N):
    """The real synthesis sum y[w] = sum_{m < mtr} c_m (Re Y[m] cos(2 pi m w / N) - Im Y[m] sin(2 pi m w / N)), c_m = 1 for
    m = 0 and m = N / 2, else 2, with the imaginary parts of those two bins dropped; orders >= mtr are zero.
    Yf [m][k][b][ri][c] -> (y, S) as (B, C, K, N)."""
    Yf = Yf.double()
    mtr = Yf.shape[0]
    re, im = Yf[:, :, :, 0].permute(2, 3, 1, 0).clone(), Yf[:, :, :, 1].permute(2, 3, 1, 0).clone()   # (B, C, K, mtr)
    im[..., 0] = 0.0
    if mtr > N // 2:
        im[..., N // 2] = 0.0
    cm = _irfft_weights(N, mtr)
    c, s = _trig(N, mtr)
    y = (re * cm) @ c.T - (im * cm) @ s.T
    S = (re.abs() * cm) @ c.abs().T + (im.abs() * cm) @ s.abs().T
    return y, S


# ---- FFT: float32 restatements ----------------------------------------------------------------------------------------------
def rfft_f32(x, mtr):
    X = torch.fft.rfft(x.float(), dim=-1, norm="forward")[..., :mtr] * torch.tensor(2.0 * math.pi, dtype=torch.float32)
    return to_spec_layout(X.real, X.imag)


def irfft_f32(Yf, N):
    mtr = Yf.shape[0]
    re, im = Yf[:, :, :, 0].permute(2, 3, 1, 0).float().clone(), Yf[:, :, :, 1].permute(2, 3, 1, 0).float().clone()
    im[..., 0] = 0.0
    if mtr > N // 2:
        im[..., N // 2] = 0.0
    Y = torch.zeros(*re.shape[:-1], N // 2 + 1, dtype=torch.complex64)
    Y[..., :mtr] = torch.complex(re, im)
    return torch.fft.irfft(Y, n=N, dim=-1, norm="forward")


# ---- Legendre ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def leg_tables(nlat, nlon, lmax, mmax, grid):
    """(Wq, P) [m][l][k], m < mtr, float64 values of the float32 tables the plan uploads: sdy_sht_tables_host in float64, the
    products pct * w and pct cast to float32 (csrc/capi.hip, sdy_sht_plan_create_ex).  Entries with m > l are zero."""
    import sdy_amd
    from sdy_amd._lib import SDY_GRID

    pct = np.zeros((mmax, lmax, nlat), dtype=np.float64)
    w = np.zeros(nlat, dtype=np.float64)
    rc = sdy_amd.lib.sdy_sht_tables_host(nlat, nlon, lmax, mmax, SDY_GRID[grid], pct.ctypes.data_as(C.c_void_p),
                                         w.ctypes.data_as(C.c_void_p), None)
    assert rc == 0, rc
    mtr = min(mmax, lmax)
    pct = pct[:mtr]
    Wq = torch.from_numpy((pct * w[None, None, :]).astype(np.float32).astype(np.float64))
    P = torch.from_numpy(pct.astype(np.float32).astype(np.float64))
    return Wq, P


def leg_fwd(Wq, Xf, dtype=torch.float64):
    """Cs[l][m][n] = sum_k Wq[m][l][k] Xf[m][k][n]."""
    return torch.einsum("mlk,mkn->lmn", Wq.to(dtype), Xf.to(dtype))


def leg_inv(P, Cs, dtype=torch.float64):
    """Yf[m][k][n] = sum_l P[m][l][k] Cs[l][m][n]."""
    return torch.einsum("mlk,lmn->mkn", P.to(dtype), Cs.to(dtype))


def leg_sums(direction, W, X):
    """(S, sum |W|, Wmax sum |X|, F) per output element of `direction` ("fwd": W = Wq, X = Xf; "inv": W = P, X = Cs), float64.
    The sum of |X| runs over the terms whose table entry is structurally non-zero (l >= m).  F = FLT_MIN sum_k (1 + |X|) is
    float32's underflow floor: towards the poles the tables of high orders fall below 2^-126, where an entry or a product
    may be flushed to zero (|w| < FLT_MIN costs at most FLT_MIN |x|, a flushed product at most FLT_MIN)."""
    Wa, Xa = W.abs(), X.double().abs()
    tri = (torch.arange(W.shape[1])[None, :] >= torch.arange(W.shape[0])[:, None]).double()   # [m][l]
    wmax = float(Wa.max())
    if direction == "fwd":
        S = torch.einsum("mlk,mkn->lmn", Wa, Xa)
        sw = Wa.sum(dim=2).T[:, :, None].expand_as(S)                                  # [l][m]
        sx = (Xa.sum(dim=1)[None, :, :] * tri.T[:, :, None]).expand_as(S)              # [m][n], zero where m > l
        F = FLT_MIN * (W.shape[2] + Xa.sum(dim=1))[None, :, :].expand_as(S)
    else:
        S = torch.einsum("mlk,lmn->mkn", Wa, Xa)
        sw = Wa.sum(dim=1)[:, :, None].expand_as(S)                                    # [m][k]
        sx = torch.einsum("ml,lmn->mn", tri, Xa)[:, None, :].expand_as(S)
        F = FLT_MIN * (W.shape[1] + Xa.sum(dim=0))[:, None, :].expand_as(S)
    return S, sw, wmax * sx, F


def f32_bound(yard, S, F=0.0):
    return KERNEL_FACTOR * (yard * S + F)


def split_bound(yard, S, sw, wmax_sx, F):
    return SPLIT_REL * S + SPLIT_ACT_FLOOR * sw + SPLIT_TAB_FLOOR * wmax_sx + f32_bound(yard, S, F)


def leg_bound(case, direction, S, sw, wmax_sx, F):
    yard = YARD[(direction, case.name)]
    return f32_bound(yard, S, F) if case.leg == LEG_GEMM_F32 else split_bound(yard, S, sw, wmax_sx, F)


def leg_case_io(case, grid, B, Cc, direction):
    """(input, float64 reference, W) of one Legendre run."""
    Wq, P = leg_tables(case.nlat, case.nlon, case.lmax, case.mmax, grid)
    Xf, Cs = leg_inputs(case, B, Cc)
    return (Xf, leg_fwd(Wq, Xf), Wq) if direction == "fwd" else (Cs, leg_inv(P, Cs), P)


# ---- the measurement --------------------------------------------------------------------------------------------------------
def _ratio(got, ref, S, F=0.0):
    return float((((got.double() - ref).abs() - F).clamp_min(0.0) / S.clamp_min(1e-300)).max())


def measure_yardsticks():
    """{key: largest |float32 restatement - float64| / S} over the inputs of the GPU tests (unrounded)."""
    out = {}
    for case in FFT_CASES:
        x, Yf, _, _, _ = fft_inputs(case)
        ref, S = rfft_ref(x, case.mtr)
        k = ("rfft", case.nlon)
        out[k] = max(out.get(k, 0.0), _ratio(rfft_f32(x, case.mtr), ref, S))
        ref, S = irfft_ref(Yf, case.nlon)
        k = ("irfft", case.nlon)
        out[k] = max(out.get(k, 0.0), _ratio(irfft_f32(Yf, case.nlon), ref, S))
    for case in LEG_CASES:
        for grid in GRIDS:
            for B, Cc in case.BC:
                for direction in ("fwd", "inv"):
                    X, ref, W = leg_case_io(case, grid, B, Cc, direction)
                    S, _, _, F = leg_sums(direction, W, X)
                    got = (leg_fwd if direction == "fwd" else leg_inv)(W, X, torch.float32)
                    k = (direction, case.name)
                    out[k] = max(out.get(k, 0.0), _ratio(got, ref, S, F))
    return out


# ---- device buffers ---------------------------------------------------------------------------------------------------------
# The guard bands are wider than anything a wrong ring or order bound of these kernels can reach: four rings of a case's rows,
# or one whole m-plane (nlat * 2 B C floats; the largest here is 181 * 2 * 48 = 17376, fft360 181 x 360 with C = 48), so
# such a defect reads or writes NaN guards and not memory outside the allocation.
GUARD, NAN = 20480, float("nan")


class Buf:
    """A device tensor `t` of `shape` inside a larger allocation with GUARD elements of NaN on both sides (`offset` more in
    front: offset = 1 gives a float pointer 4 bytes off a 16-byte boundary that is still in bounds).  `fill`: NaN (an output),
    or a CPU tensor to copy (an input)."""

    def __init__(self, shape, fill=None, offset=0):
        n = math.prod(shape)
        self.raw = torch.full((n + 2 * GUARD + offset,), NAN, dtype=torch.float32, device="cuda")
        self.lo, self.hi = GUARD + offset, GUARD + offset + n
        self.t = self.raw[self.lo:self.hi].view(shape)
        if fill is not None:
            self.t.copy_(fill.reshape(shape).float())
        assert self.t.data_ptr() % 16 == (4 * offset) % 16
        self.before = self.t.clone()

    @property
    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool(torch.isnan(self.raw[:self.lo]).all()) and bool(torch.isnan(self.raw[self.hi:]).all())

    def unchanged(self):
        return self.guards_intact() and bits_equal(self.t, self.before)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32).cpu(), b.contiguous().view(torch.int32).cpu())


def within(got, ref, bound, what):
    """Element by element |got - ref| <= bound (float64 CPU tensors), no NaN left in got; prints and returns the worst ratio."""
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    assert not bool(torch.isnan(got).any()), f"{what}: NaN poison left in the output"
    err = (got - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: worst |err| / bound = {ratio:.3f}, worst |err| = {float(err.max()):.3e}")
    assert bool((err <= bound).all()), f"{what}: |err| / bound up to {ratio:.3f}"
    return ratio


if __name__ == "__main__":
    for key, v in sorted(measure_yardsticks().items(), key=str):
        print(f"    {key!r}: {round_up2(v):.1e},   # measured {v:.3e}")
