"""Float64 restatement, inputs and tolerances of the rotational / divergent kinetic-energy spectra (sdy_vector_degree_power,
sdy_vector_legendre_fwd, sdy_vsht_tables_host, include/sdy_amd.h; sdy_amd.spectrum).  Shared by
tests/test_vector_spectrum_host.py and tests/test_gpu_vector_spectrum.py.

The restatement is numpy on `oracle.sht.quadrature` / `legpoly` and `np.fft.rfft`; it never calls the library's tables.  For
a wind (u eastward, v northward), V_theta = -v, V_lambda = u, and with the tables D = dP/dtheta (ladder form) and
M = m P / sin(theta) (pole rule), both divided by sqrt(l (l + 1)):
    A_T[f](l, m) = sum_k w_k T[m][l][k] f_m(k),        f_m = 2 pi rfft(f, norm="forward")
    s = A_D[V_theta] - i A_M[V_lambda],   t = A_D[V_lambda] + i A_M[V_theta]
    E_div(l) = 1/2 sum_m w_m |s(l, m)|^2,  E_rot(l) the same of t,   w_0 = 1, w_m = 2 for 1 <= m <= l.

Three kinds of bound, none of them measured:

* the reduction alone (`reduction_bound`): host twin, device kernel and numpy combine and sum the same fp32 numbers.  Every
  term is non-negative; a sum of n terms carries at most n - 1 roundings, the combination of four values into a component of
  s or t, its square, the sum of the two squares and (for the error) the difference at most four more per term, the division
  by the row count and the accumulator's addition a few more: relative error <= (n + 8) 2^-53 for the code and as much for
  numpy, 2 (n + 8) 2^-53 between them.
* the stage (`stage_bound`): per real or imaginary part of a coefficient
      |delta| <= c 2^-24 sum_k |w_k T[m][l][k]| (2 pi / nlon) sum_j |x_kj|,      c = 2 nlat + 8 ceil(log2 nlon) + 16.
  The nlat factor covers an fp32 sum of nlat terms in any order; the table and product roundings and an FFT of
  ceil(log2 nlon) levels are each doubled for the float64-to-fp32 cast of the table and for slack.
* end to end (`pooled`): with d_l^2 = sum_m w_m |delta(l, m)|^2 of a row, taken from the stage bound (a component of s or t is
  the sum of two parts of two products, so |delta s|^2 <= 2 (b_D[v] + b_M[u])^2), Cauchy-Schwarz gives
      |delta E(l)| <= sqrt(2 E_ref(l)) d_l + d_l^2 / 2.
  The bound is absolute; the error spectrum's d_l is the sum of the generated row's and its target row's (triangle
  inequality).  The per-field power-of-two pre-scale of the aggregator changes neither side of the stage bound."""
import ctypes as C
import functools
import math

import numpy as np
import torch

import spectrum_utils as su
from oracle.sht import legpoly, quadrature

GRIDS = su.GRIDS
GRID_ID = {"equiangular": 0, "legendre-gauss": 1}
U = 2.0 ** -53
LABELS = ("gen_rot", "gen_div", "target_rot", "target_div", "error_rot", "error_div")


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tables64(nlat, nlon, lmax, mmax, grid):
    """(D, M, theta, w): the two tables [mmax][lmax][nlat] float64, colatitudes and quadrature weights."""
    theta, w = quadrature(nlat, grid)
    P = legpoly(mmax + 1, lmax, np.cos(theta))                      # one order more, for the ladder
    l = np.arange(lmax, dtype=np.float64)[None, :, None]
    m = np.arange(mmax, dtype=np.float64)[:, None, None]
    up, mid = P[1:mmax + 1], P[:mmax]
    down = np.concatenate([np.zeros_like(P[:1]), P[:mmax - 1]]) if mmax > 1 else np.zeros_like(P[:1])
    with np.errstate(invalid="ignore"):
        ladder = 0.5 * (np.sqrt((l - m) * (l + m + 1.0)) * up - np.sqrt((l + m) * (l - m + 1.0)) * down)
    ladder[0] = np.sqrt(l[0] * (l[0] + 1.0)) * P[1]
    ladder = np.where(m > l, 0.0, ladder)
    norm = np.sqrt(l * (l + 1.0))
    norm[:, 0] = np.inf                                             # row l = 0 is identically zero
    D = ladder / norm
    interior = slice(1, nlat - 1) if grid == "equiangular" else slice(None)
    M = np.zeros_like(D)
    M[..., interior] = m * mid[..., interior] / np.sin(theta[interior]) / norm
    if grid == "equiangular" and mmax > 1:                          # the pole rule: only m = 1 survives
        M[1, :, 0], M[1, :, -1] = D[1, :, 0], -D[1, :, -1]
    for a in (D, M, theta, w):
        a.setflags(write=False)
    return D, M, theta, w


def _dims(x, lmax, mmax):
    nlat, nlon = x.shape[-2:]
    return nlat, nlon, lmax or nlat, mmax or nlon // 2 + 1


def products64(x, grid, lmax=None, mmax=None):
    """(A_D[x], A_M[x]) complex128 (..., lmax, mmax) of scalar fields x (..., nlat, nlon)."""
    x = np.asarray(x, dtype=np.float64)
    nlat, nlon, lmax, mmax = _dims(x, lmax, mmax)
    D, M, _, w = tables64(nlat, nlon, lmax, mmax, grid)
    f = 2.0 * np.pi * np.fft.rfft(x, axis=-1, norm="forward")[..., :mmax]          # (..., nlat, mmax)
    return np.einsum("...km,mlk->...lm", f, D * w), np.einsum("...km,mlk->...lm", f, M * w)


def analysis64(u, v, grid, lmax=None, mmax=None):
    """(s, t) complex128 (..., lmax, mmax) of the wind (u, v)."""
    du, mu = products64(u, grid, lmax, mmax)
    dv, mv = products64(v, grid, lmax, mmax)
    return -dv - 1j * mu, du - 1j * mv            # V_theta = -v, V_lambda = u


def energy(c):
    """E(l) = 1/2 sum_m w_m |c(l, m)|^2 of coefficients (..., lmax, mmax)."""
    return 0.5 * su.degree_power(c)


def synthesise64(s, t, nlat, nlon, grid, tables=None):
    """(u, v) float64 (nlat, nlon) from coefficients (lmax, mmax): V_theta = sum s D e^{im lam} - i t M e^{im lam},
    V_lambda = sum i s M e^{im lam} + t D e^{im lam}, real part, m > 0 doubled.  `tables`: (D, M) to use instead of the
    restatement's own (the identity tests feed the library's)."""
    lmax, mmax = s.shape
    D, M = tables if tables is not None else tables64(nlat, nlon, lmax, mmax, grid)[:2]
    vt = np.einsum("lm,mlk->km", s, D) - 1j * np.einsum("lm,mlk->km", t, M)
    vl = 1j * np.einsum("lm,mlk->km", s, M) + np.einsum("lm,mlk->km", t, D)
    wm = np.where(np.arange(mmax) == 0, 1.0, 2.0)
    wave = np.exp(1j * np.outer(np.arange(mmax), 2.0 * np.pi * np.arange(nlon) / nlon))          # [m][j]
    return ((wm * vl) @ wave).real, -((wm * vt) @ wave).real


def analyse_with(u, v, D, M, w, mmax):
    """analysis64 with given tables (the identity tests: the library's host tables)."""
    f = lambda x: 2.0 * np.pi * np.fft.rfft(x, axis=-1, norm="forward")[..., :mmax]      # noqa: E731
    A = lambda x, T: np.einsum("...km,mlk->...lm", f(x), T * w)                            # noqa: E731
    return -A(v, D) - 1j * A(u, M), A(u, D) - 1j * A(v, M)


def random_st(lmax, mmax, key, slope=0.0, below=None):
    """Random (s, t): m <= l, real m = 0, nothing at l = 0 (and nothing at l >= below)."""
    out = []
    for part in ("s", "t"):
        a = su.random_coeffs(lmax, mmax, (key, part), slope=slope)
        a[0] = 0.0
        if below is not None:
            a[below:] = 0.0
        out.append(a)
    return out


def host_tables(nlat, nlon, lmax, mmax, grid):
    """(D, M) of the library: sdy_vsht_tables_host."""
    import sdy_amd

    d, m = np.full((mmax, lmax, nlat), np.nan), np.full((mmax, lmax, nlat), np.nan)
    assert sdy_amd.lib.sdy_vsht_tables_host(nlat, nlon, lmax, mmax, GRID_ID[grid], d.ctypes.data, m.ctypes.data) == 0
    return d, m


# ---- the stage bound -----------------------------------------------------------------------------------------------------------
def stage_bound(x, grid, lmax=None, mmax=None):
    """(b_D, b_M) float64 (..., lmax, mmax): the bound of the module docstring for either part of A_D[x] and A_M[x]."""
    x = np.asarray(x, dtype=np.float64)
    nlat, nlon, lmax, mmax = _dims(x, lmax, mmax)
    D, M, _, w = tables64(nlat, nlon, lmax, mmax, grid)
    c = 2.0 * nlat + 8.0 * math.ceil(math.log2(nlon)) + 16.0
    ring = (2.0 * np.pi / nlon) * np.abs(x).sum(axis=-1)                                    # (..., nlat)
    return tuple(c * 2.0 ** -24 * np.einsum("...k,mlk->...lm", ring, np.abs(T * w)) for T in (D, M))


def row_distance(u, v, grid):
    """d_l (..., lmax) of the rows of a wind: sqrt(sum_m w_m |delta|^2) with |delta s|^2 <= 2 (b_D[v] + b_M[u])^2 and
    |delta t|^2 <= 2 (b_D[u] + b_M[v])^2 -> {"div", "rot"}."""
    bdu, bmu = stage_bound(u, grid)
    bdv, bmv = stage_bound(v, grid)
    w = su.m_weights(*bdu.shape[-2:])
    return {"div": np.sqrt((w * 2.0 * (bdv + bmu) ** 2).sum(axis=-1)), "rot": np.sqrt((w * 2.0 * (bdu + bmv) ** 2).sum(axis=-1))}


# ---- fields of the end-to-end cases ------------------------------------------------------------------------------------------
def red_wind(shape, nlat, nlon, grid, key):
    """Winds synthesised in float64 from (s, t) with l^-3 power, cast to float32: (u, v) of shape (*shape, nlat, nlon)."""
    n = int(np.prod(shape))
    uv = [synthesise64(*random_st(nlat, nlon // 2 + 1, (key, i), slope=-3.0), nlat, nlon, grid) for i in range(n)]
    u = np.stack([a for a, _ in uv]).astype(np.float32).reshape(*shape, nlat, nlon)
    v = np.stack([b for _, b in uv]).astype(np.float32).reshape(*shape, nlat, nlon)
    return u, v


@functools.lru_cache(maxsize=None)
def window_winds(nlat, nlon, grid, M, S, T, key=0):
    """{label: ((gen_u, gen_v) (M, S, T, nlat, nlon), (target_u, target_v) (S, T, nlat, nlon))} float32: a white pair, a red
    pair, and gen = target + 1e-3 noise."""
    out = {}
    wh = lambda shape, k: su.white(shape, nlat, nlon, (key, "wind", k))      # noqa: E731
    out["white"] = ((wh((M, S, T), "gu"), wh((M, S, T), "gv")), (wh((S, T), "tu"), wh((S, T), "tv")))
    out["red"] = (red_wind((M, S, T), nlat, nlon, grid, (key, "g")), red_wind((S, T), nlat, nlon, grid, (key, "t")))
    tu, tv = wh((S, T), "ntu"), wh((S, T), "ntv")
    near = lambda t, k: (t[None] + np.float32(1e-3) * wh((M, S, T), k)).astype(np.float32)      # noqa: E731
    out["near"] = ((near(tu, "ngu"), near(tv, "ngv")), (tu, tv))
    return out


@functools.lru_cache(maxsize=None)
def reference_rows(nlat, nlon, grid, M, S, T, label, key=0):
    """Float64 restatement of every row of pair `label` of window_winds: E of gen (M, S, T, lmax), target (S, T, lmax) and
    gen - target (M, S, T, lmax) per part, and the rows' distances d_l.  Computed once and shared; callers slice, never write."""
    (gu, gv), (tu, tv) = window_winds(nlat, nlon, grid, M, S, T, key)[label]
    sg, tg = analysis64(gu, gv, grid)
    st, tt = analysis64(tu, tv, grid)
    dg, dt = row_distance(gu, gv, grid), row_distance(tu, tv, grid)
    rows = {}
    for part, cg, ct in (("div", sg, st), ("rot", tg, tt)):
        rows[part] = {"gen": energy(cg), "target": energy(ct), "error": energy(cg - ct[None]),
                      "d_gen": dg[part], "d_target": dt[part]}
    for r in rows.values():
        for a in r.values():
            a.setflags(write=False)
    return rows


def pooled(rows, members=slice(None), times=slice(None)):
    """(want, bound), each {label: (T, lmax)} for LABELS: the pooled means the accumulators hold and the Cauchy-Schwarz bound of
    the module docstring, taken per row and averaged over the rows."""
    want, bound = {}, {}
    for part in ("rot", "div"):
        r = rows[part]
        eg, et, ee = r["gen"][members][:, :, times], r["target"][:, times], r["error"][members][:, :, times]
        dg, dt = r["d_gen"][members][:, :, times], r["d_target"][:, times]
        de = dg + dt[None]
        cs = lambda e, d: np.sqrt(2.0 * e) * d + 0.5 * d ** 2      # noqa: E731
        want[f"gen_{part}"], bound[f"gen_{part}"] = eg.mean(axis=(0, 1)), cs(eg, dg).mean(axis=(0, 1))
        want[f"target_{part}"], bound[f"target_{part}"] = et.mean(axis=0), cs(et, dt).mean(axis=0)
        want[f"error_{part}"], bound[f"error_{part}"] = ee.mean(axis=(0, 1)), cs(ee, de).mean(axis=(0, 1))
    return want, bound


# ---- the reduction alone: internal layout, numpy sums, the host twin ---------------------------------------------------------
class Layout(su.Layout):
    """su.Layout of the u rows of `nvars` pairs; the v rows follow as a second, equal run: v field = u field + Fg (Ft), so a
    buffer holds 2 Fg (2 Ft) fields."""

    def __init__(self, *a):
        super().__init__(*a)
        self.g_voff, self.t_voff = self.Fg, self.Ft


ACCS = ("gen_rot", "gen_div", "target_rot", "target_div", "err_rot", "err_div")


def random_case(lay, key, scaled=False):
    """(gen_d, gen_m, target_d, target_m, gen_scale, target_scale): Cs[l][m][ri][field] float32 with normals in the fields the
    layout names (u and v runs), NaN in every padding field and in every entry with m > l."""
    g = su._gen("vcase", lay.lmax, lay.mtr, lay.nvars, lay.n0, lay.n1, lay.T, lay.g_time, key)
    used_g = {lay.gen_field(v, i0, i1, t) for v in range(lay.nvars) for i0 in range(lay.n0) for i1 in range(lay.n1)
              for t in range(lay.T)}
    used_t = {lay.target_field(v, i1, t) for v in range(lay.nvars) for i1 in range(lay.n1) for t in range(lay.T)}
    bufs = []
    for F, used in ((lay.Fg, used_g), (lay.Ft, used_t)):
        pad = np.array([f not in used for f in range(F)] * 2)
        for _ in range(2):
            cs = torch.randn(lay.lmax, lay.mtr, 2, 2 * F, generator=g).numpy()
            cs[..., pad] = np.nan
            cs[su.m_weights(lay.lmax, lay.mtr) == 0] = np.nan
            bufs.append(np.ascontiguousarray(cs, dtype=np.float32))
    scales = [None, None]
    if scaled:
        for i, F in enumerate((lay.Fg, lay.Ft)):
            e = torch.randint(-3, 21, (2 * F,), generator=g).numpy()
            scales[i] = np.ascontiguousarray(2.0 ** e, dtype=np.float32)
    return bufs[0], bufs[1], bufs[2], bufs[3], scales[0], scales[1]


def numpy_reduction(lay, gd, gm, td, tm, sg=None, st=None):
    """The six accumulator contributions (nvars, T, lmax), float64 numpy on the same fp32 numbers."""
    w = 0.5 * su.m_weights(lay.lmax, lay.mtr)[:, :, None]                                    # [l][m][1]
    gd, gm, td, tm = (a.astype(np.float64) for a in (gd, gm, td, tm))
    if sg is not None:
        gd, gm, td, tm = gd * sg.astype(np.float64), gm * sg.astype(np.float64), td * st.astype(np.float64), tm * st.astype(np.float64)

    def st_of(d, m, fields, voff):
        """s and t as (re, im) arrays [l][m][rows] of the rows whose u fields are `fields`."""
        u, v = np.asarray(fields), np.asarray(fields) + voff
        du, dv, mu, mv = d[..., u], d[..., v], m[..., u], m[..., v]                          # [l][m][ri][rows]
        s = (mu[:, :, 1] - dv[:, :, 0], -dv[:, :, 1] - mu[:, :, 0])
        t = (du[:, :, 0] + mv[:, :, 1], du[:, :, 1] - mv[:, :, 0])
        return s, t

    def e_of(c):
        with np.errstate(invalid="ignore"):
            return np.where(w > 0, w * (c[0] ** 2 + c[1] ** 2), 0.0).sum(axis=1).mean(axis=-1)      # [l]

    out = {k: np.zeros((lay.nvars, lay.T, lay.lmax)) for k in ACCS}
    for v in range(lay.nvars):
        for t in range(lay.T):
            tf = [lay.target_field(v, i1, t) for i1 in range(lay.n1)]
            gf = [lay.gen_field(v, i0, i1, t) for i0 in range(lay.n0) for i1 in range(lay.n1)]
            tt = [lay.target_field(v, i1, t) for i0 in range(lay.n0) for i1 in range(lay.n1)]
            (s_g, t_g), (s_t, t_t), (s_r, t_r) = (st_of(gd, gm, gf, lay.g_voff), st_of(td, tm, tf, lay.t_voff),
                                                  st_of(td, tm, tt, lay.t_voff))
            out["gen_div"][v, t], out["gen_rot"][v, t] = e_of(s_g), e_of(t_g)
            out["target_div"][v, t], out["target_rot"][v, t] = e_of(s_t), e_of(t_t)
            out["err_div"][v, t] = e_of((s_g[0] - s_r[0], s_g[1] - s_r[1]))
            out["err_rot"][v, t] = e_of((t_g[0] - t_r[0], t_g[1] - t_r[1]))
    return out


def reduction_bound(lay):
    """Relative bound 2 (n + 8) 2^-53 per (accumulator, degree): n = rows x orders x 2 terms summed into the element."""
    orders = np.minimum(np.arange(lay.lmax), lay.mtr - 1) + 1.0
    n_gen, n_tgt = lay.n0 * lay.n1 * orders * 2.0, lay.n1 * orders * 2.0
    return {k: 2.0 * ((n_tgt if k.startswith("target") else n_gen) + 8.0) * U for k in ACCS}


def fill_args(lay, gd, gm, td, tm, gen_scale, target_scale, t_start, n_timesteps, acc):
    """SdyVectorSpectrumArgs from raw addresses (host arrays or device pointers); acc: six addresses / None in ACCS order."""
    from sdy_amd._lib import SdyVectorSpectrumArgs

    a = SdyVectorSpectrumArgs()
    a.gen_d, a.gen_m, a.target_d, a.target_m = gd, gm, td, tm
    su.fill_rows(a.rows, lay, gen_scale, target_scale, t_start, n_timesteps, components=2)
    a.gen_v_offset, a.target_v_offset = lay.g_voff, lay.t_voff
    a.gen_rot, a.gen_div, a.target_rot, a.target_div, a.err_rot, a.err_div = acc
    return a


def host_accumulate(lay, bufs, t_start, acc, with_error=True):
    """One sdy_vector_degree_power_host call adding to acc = {ACCS: float64 (nvars, n_timesteps, lmax)}."""
    import sdy_amd

    addr = lambda x: None if x is None else x.ctypes.data      # noqa: E731
    accs = tuple(addr(acc[k]) if with_error or not k.startswith("err") else None for k in ACCS)
    a = fill_args(lay, *[addr(b) for b in bufs], t_start, acc["gen_rot"].shape[1], accs)
    return sdy_amd.lib.sdy_vector_degree_power_host(C.byref(a))


REDUCTION_CASES = su.REDUCTION_CASES
case_id = su.case_id
