"""Float64 restatement, inputs and bounds of the Helmholtz fields of a wind -- relative vorticity, divergence, streamfunction,
velocity potential (sdy_helmholtz_coefficients, sdy_helmholtz_factors_host, include/sdy_amd.h; sdy_amd.helmholtz).  Shared by
tests/test_helmholtz_host.py and tests/test_gpu_helmholtz.py; built on tests/vector_spectrum_utils.py.

The restatement: (s, t) = analysis64(u, v) in float64 numpy, then per degree
    zeta = -sqrt(l (l + 1)) t / a    delta = -sqrt(l (l + 1)) s / a    psi = a t / sqrt(l (l + 1))    chi = a s / sqrt(l (l + 1))
(zero at l = 0 and at l > truncate), then the scalar synthesis y = irfft(sum_l c(l, m) P[m][l][k], norm="forward") with
oracle.sht.legpoly.  It never calls the library.

Two kinds of comparison:

* the kernel alone (`numpy_kernel`): host twin, device kernel and numpy work on the same fp32 numbers.  A component of s or t
  is one rounded sum of two float64 products (exact for a power-of-two scale; one rounding each otherwise, the same in numpy),
  the product with the factor one more rounding, the cast to fp32 the last: numpy reproduces the chain BIT FOR BIT.
* end to end (`bound`), derived in the manner of vector_spectrum_utils.stage_bound, not measured:
    coefficient error per (l, m):  e(l,m) = sqrt(2) (b_D + b_M of the two components, paired as row_distance pairs them)
                                            x |factor(l)| + 2^-24 |c(l,m)|            (the one rounding to fp32)
    through the synthesis:         |delta y(k, .)| <= sum_m w_m sum_l |P[m][l][k]| (e(l,m) + c_syn 2^-24 |c(l,m)|),
                                   c_syn = 2 lmax + 8 ceil(log2 nlon) + 16
  (an fp32 sum of lmax terms in any order, table and product roundings and an inverse FFT of ceil(log2 nlon) levels, each
  doubled as in stage_bound), w_0 = 1, w_m = 2."""
import ctypes as C
import functools
import math

import numpy as np
import torch

import spectrum_utils as su
import vector_spectrum_utils as vu
from oracle.sht import legpoly, quadrature

RADIUS = 6.371e6
OUTPUTS = ("vorticity", "divergence", "streamfunction", "velocity_potential")
PART = {"vorticity": 1, "divergence": 0, "streamfunction": 1, "velocity_potential": 0}      # 0: s, 1: t
KIND = {"vorticity": 0, "divergence": 0, "streamfunction": 1, "velocity_potential": 1}
SDY_ERR_ARG, SDY_ERR_UNSUPPORTED, SDY_ERR_ALIGN = -1, -2, -3
GUARD = 256


# ---- the factor rows ---------------------------------------------------------------------------------------------------------
def factors64(lmax, radius, kind, truncate=None):
    l = np.arange(lmax, dtype=np.float64)
    n = np.sqrt(l * (l + 1.0))
    with np.errstate(divide="ignore"):
        f = -n / radius if kind == 0 else radius / n
    f[0] = 0.0
    if truncate is not None and truncate >= 0:
        f[l > truncate] = 0.0
    return f


def host_factors(lmax, radius, kind, truncate=None):
    """One row of the LIBRARY's table: sdy_helmholtz_factors_host."""
    import sdy_amd

    out = np.full(lmax, np.nan)
    assert sdy_amd.lib.sdy_helmholtz_factors_host(lmax, radius, kind, -1 if truncate is None else truncate, out.ctypes.data) == 0
    return out


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scalar_table(nlat, lmax, mmax, grid):
    theta, _ = quadrature(nlat, grid)
    P = legpoly(mmax, lmax, np.cos(theta))
    P.setflags(write=False)
    return P


def synth64(c, nlat, nlon, grid):
    """Scalar synthesis of coefficients (..., lmax, mmax) complex128 -> (..., nlat, nlon) float64."""
    P = scalar_table(nlat, c.shape[-2], c.shape[-1], grid)
    return np.fft.irfft(np.einsum("...lm,mlk->...km", c, P), n=nlon, axis=-1, norm="forward")


def coefficients64(u, v, grid, outputs=OUTPUTS, radius=RADIUS, truncate=None):
    """{name: (..., lmax, mmax) complex128}: the scalar coefficients of the restatement."""
    s, t = vu.analysis64(u, v, grid)
    lmax = s.shape[-2]
    return {name: (t if PART[name] else s) * factors64(lmax, radius, KIND[name], truncate)[:, None] for name in outputs}


def helmholtz64(u, v, grid, outputs=OUTPUTS, radius=RADIUS, truncate=None):
    nlat, nlon = np.shape(u)[-2:]
    return {name: synth64(c, nlat, nlon, grid) for name, c in coefficients64(u, v, grid, outputs, radius, truncate).items()}


def bound(u, v, grid, outputs=OUTPUTS, radius=RADIUS, truncate=None):
    """{name: (..., nlat, 1)}: the end-to-end bound of the module docstring, per wind and latitude (for every longitude)."""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    nlat, nlon = u.shape[-2:]
    bdu, bmu = vu.stage_bound(u, grid)
    bdv, bmv = vu.stage_bound(v, grid)
    stage = {0: math.sqrt(2.0) * (bdv + bmu), 1: math.sqrt(2.0) * (bdu + bmv)}          # |delta s|, |delta t|
    lmax, mmax = bdu.shape[-2:]
    coef = coefficients64(u, v, grid, outputs, radius, truncate)
    absP = np.abs(scalar_table(nlat, lmax, mmax, grid))
    w = np.where(np.arange(mmax) == 0, 1.0, 2.0)
    c_syn = 2.0 * lmax + 8.0 * math.ceil(math.log2(nlon)) + 16.0
    out = {}
    for name in outputs:
        f = np.abs(factors64(lmax, radius, KIND[name], truncate))[:, None]
        c = np.abs(coef[name])
        e = stage[PART[name]] * f + 2.0 ** -24 * c
        out[name] = (np.einsum("...lm,mlk->...km", e + c_syn * 2.0 ** -24 * c, absP) * w).sum(axis=-1)[..., None]
    return out


def winds(n, nlat, nlon, grid, key="hh"):
    """(u, v) float32 (n, nlat, nlon): the first half white pairs, the second half red winds (l^-3 power)."""
    h = n // 2
    wu, wv = su.white((h,), nlat, nlon, (key, "u")), su.white((h,), nlat, nlon, (key, "v"))
    ru, rv = vu.red_wind((n - h,), nlat, nlon, grid, key)
    return np.concatenate([wu, ru]).astype(np.float32), np.concatenate([wv, rv]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(n, nlat, nlon, grid, truncate=None, key="hh"):
    """(u, v, want, bound) of `winds`: computed once and shared; callers never write."""
    u, v = winds(n, nlat, nlon, grid, key)
    want, bnd = helmholtz64(u, v, grid, truncate=truncate), bound(u, v, grid, truncate=truncate)
    for a in (u, v, *want.values(), *bnd.values()):
        a.setflags(write=False)
    return u, v, want, bnd


def solid_body(nlat, nlon, grid, U=30.0):
    """u = U cos(lat), v = 0, and the latitude of every row."""
    theta, _ = quadrature(nlat, grid)
    lat = 0.5 * np.pi - theta
    return np.repeat((U * np.cos(lat))[:, None], nlon, axis=1), np.zeros((nlat, nlon)), lat


# ---- the kernel alone: layouts, numpy on the same fp32 numbers, the host twin -------------------------------------------------
class Case:
    """One layout of sdy_helmholtz_args: `fields` input fields with the u run at u_offset and the v run at v_offset, `names`
    the outputs, planes out_stride fields apart in a tensor of out_fields fields."""

    def __init__(self, lmax, mtr, fields, u_offset, v_offset, n_winds, names, out_stride, out_fields, scaled):
        self.lmax, self.mtr, self.fields, self.n_winds = lmax, mtr, fields, n_winds
        self.u_offset, self.v_offset = u_offset, v_offset
        self.names, self.out_stride, self.out_fields, self.scaled = tuple(names), out_stride, out_fields, scaled

    @property
    def id(self):
        return (f"l{self.lmax}m{self.mtr}-{self.n_winds}of{self.fields}-{len(self.names)}out-stride{self.out_stride}"
                + ("-scaled" if self.scaled else ""))


# one wind padded to four fields; five winds with the runs apart (padding fields in front, between and behind), planes with a
# quad between them and two behind the last; one and four outputs; with and without scales; full and truncated orders
CASES = [Case(lmax, mtr, *lay, names, *out, scaled)
         for lmax, mtr in ((7, 5), (12, 12))
         for lay, outs in (((8, 0, 4, 1), {1: (4, 4), 4: (4, 16)}), ((24, 4, 16, 5), {1: (0, 12), 4: (12, 52)}))
         for names, out in ((OUTPUTS[2:3], outs[1]), (OUTPUTS, outs[4]))
         for scaled in (False, True)]


def random_inputs(case, key=0):
    """(Cs_d, Cs_m, scale or None, factor): float32 [l][m][ri][fields] with normals in the fields of the two runs, NaN in every
    other field and in every entry with m > l; the library's factor rows [n_out][lmax]."""
    g = su._gen("hhcase", case.id, key)
    used = np.zeros(case.fields, dtype=bool)
    used[case.u_offset:case.u_offset + case.n_winds] = used[case.v_offset:case.v_offset + case.n_winds] = True
    bufs = []
    for _ in range(2):
        cs = torch.randn(case.lmax, case.mtr, 2, case.fields, generator=g).numpy()
        cs[..., ~used] = np.nan
        cs[su.m_weights(case.lmax, case.mtr) == 0] = np.nan
        bufs.append(np.ascontiguousarray(cs, dtype=np.float32))
    scale = None
    if case.scaled:
        e = torch.randint(-3, 21, (case.fields,), generator=g).numpy()
        scale = np.ascontiguousarray(2.0 ** e, dtype=np.float32)
        scale[~used] = np.nan
    factor = np.stack([host_factors(case.lmax, RADIUS, KIND[n]) for n in case.names])
    return bufs[0], bufs[1], scale, factor


def numpy_kernel(case, cd, cm, scale, factor):
    """What `out` must hold, bit for bit: float64 numpy on the same fp32 numbers, rounded once."""
    out = np.zeros((case.lmax, case.mtr, 2, case.out_fields), dtype=np.float32)
    iu = np.arange(case.u_offset, case.u_offset + case.n_winds)
    iv = np.arange(case.v_offset, case.v_offset + case.n_winds)
    d, m = cd.astype(np.float64), cm.astype(np.float64)
    su_, sv_ = (1.0, 1.0) if scale is None else (scale[iu].astype(np.float64), scale[iv].astype(np.float64))
    du, dv, mu, mv = d[..., iu] * su_, d[..., iv] * sv_, m[..., iu] * su_, m[..., iv] * sv_          # [l][m][ri][wind]
    s = (mu[:, :, 1] - dv[:, :, 0], -dv[:, :, 1] - mu[:, :, 0])
    t = (du[:, :, 0] + mv[:, :, 1], du[:, :, 1] - mv[:, :, 0])
    live = (su.m_weights(case.lmax, case.mtr) > 0)[:, :, None] & (np.arange(case.lmax) > 0)[:, None, None]
    for q, name in enumerate(case.names):
        x = t if PART[name] else s
        f0 = q * case.out_stride
        for ri in range(2):
            with np.errstate(invalid="ignore"):
                y = (x[ri] * factor[q][:, None, None]).astype(np.float32)
            out[:, :, ri, f0:f0 + case.n_winds] = np.where(live, y, np.float32(0.0))
    return out


def fill_args(case, cd, cm, scale, factor, out):
    """SdyHelmholtzArgs from raw addresses (host arrays' or device pointers'; scale may be None)."""
    from sdy_amd._lib import SdyHelmholtzArgs

    a = SdyHelmholtzArgs()
    a.Cs_d, a.Cs_m, a.scale, a.factor, a.out = cd, cm, scale, factor, out
    a.lmax, a.mtr = case.lmax, case.mtr
    a.fields, a.u_offset, a.v_offset, a.n_winds = case.fields, case.u_offset, case.v_offset, case.n_winds
    a.out_fields, a.out_stride, a.n_out = case.out_fields, case.out_stride, len(case.names)
    for q, name in enumerate(case.names):
        a.part[q] = PART[name]
    return a


def guarded_out(case):
    """(raw, out, lead): a float32 host array of NaN with at least GUARD floats on either side of `out`
    [l][m][ri][out_fields], which starts at raw[lead] on a 16-byte boundary."""
    n = case.lmax * case.mtr * 2 * case.out_fields
    raw = np.full(n + 2 * GUARD + 4, np.nan, dtype=np.float32)
    lead = GUARD + (-(raw.ctypes.data // 4 + GUARD)) % 4
    return raw, raw[lead:lead + n].reshape(case.lmax, case.mtr, 2, case.out_fields), lead


def guards_intact(raw, lead, n):
    return bool(np.isnan(raw[:lead]).all() and np.isnan(raw[lead + n:]).all())


def aligned_copy(x):
    """A 16-byte aligned host copy of a float32 array (None stays None)."""
    if x is None:
        return None
    raw = np.empty(x.size + 4, dtype=x.dtype)
    lead = (-(raw.ctypes.data // x.itemsize)) % (16 // x.itemsize)
    y = raw[lead:lead + x.size].reshape(x.shape)
    y[...] = x
    return y


def host_run(case, cd, cm, scale, factor, out):
    import sdy_amd

    addr = lambda x: None if x is None else x.ctypes.data      # noqa: E731
    a = fill_args(case, addr(cd), addr(cm), addr(scale), addr(factor), addr(out))
    return sdy_amd.lib.sdy_helmholtz_coefficients_host(C.byref(a))


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))
