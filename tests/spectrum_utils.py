"""Float64 restatement, inputs and tolerances of the spherical power spectra (sdy_degree_power, include/sdy_amd.h;
sdy_amd.spectrum).  Shared by tests/test_spectrum_host.py and tests/test_gpu_spectrum.py.

The restatement is oracle.sht.RealSHT in float64 followed by
    P(l) = |a[l,0]|^2 + 2 sum_{m = 1 .. min(l, mmax - 1)} |a[l,m]|^2
in numpy.  Two kinds of bound:

* the reduction alone (`reduction_bound`): host twin, device kernel and numpy sum the same fp32 numbers.  Squares of fp32
  values are exact in float64 and every term is non-negative, so a sum of n terms carries at most (n - 1) roundings of
  relative size 2^-53 each, the rounded products of the error spectrum, the division by the row count and the accumulator's
  addition four more: relative error <= (n + 4) 2^-53 for the code and as much for numpy, 2 (n + 4) 2^-53 between them.
* end to end (`pooled`): the device transform is fp32-class, and with a red spectrum a degree's relative error is not
  bounded by the transform's accuracy.  If the coefficient vector of a row is off by at most d in the weighted L2 norm
  (sum_lm w_m |da|^2 <= d^2), Cauchy-Schwarz gives |dP(l)| <= 2 sqrt(P_ref(l)) d + d^2.  d = EPS_SHT * sqrt(sum_l P_ref(l)).
  EPS_SHT is not chosen: it is the largest relative weighted-L2 distance of `sdy_amd.RealSHT` (unchanged by the spectra) from
  the float64 oracle on the very fields below, measured on an MI355X (NOTEBOOK.md section 7m: 12 x 24 on both grids and
  180 x 360 equiangular, white, red and near-copy fields; largest value EPS_SHT_MEASURED; tests/test_gpu_spectrum.py,
  test_the_yardstick_of_the_transform, prints the same table again), times EPS_SHT_FACTOR = 2 because
  the aggregator pads to another field count than RealSHT and may so run another FFT kernel.  The error spectrum uses the
  same absolute d with P_ref of the difference field (the coefficient error is absolute)."""
import ctypes as C
import functools
import zlib

import numpy as np
import torch

from oracle.sht import InverseRealSHT, RealSHT, quadrature

GRIDS = ("equiangular", "legendre-gauss")
SDY_ERR_ARG, SDY_ERR_UNSUPPORTED = -1, -2
U = 2.0 ** -53

EPS_SHT_MEASURED = 1.95e-07   # measured 1.9428e-07 (180 x 360 equiangular, red, a generated row), rounded up
EPS_SHT_FACTOR = 2.0
EPS_SHT = EPS_SHT_FACTOR * EPS_SHT_MEASURED


def _gen(*key):
    return torch.Generator(device="cpu").manual_seed(zlib.crc32(repr(key).encode()))


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def m_weights(lmax, mmax):
    """w[l][m]: 1 for m = 0, 2 for 1 <= m <= l, 0 above the diagonal."""
    l, m = np.arange(lmax)[:, None], np.arange(mmax)[None, :]
    return np.where(m > l, 0.0, np.where(m == 0, 1.0, 2.0))


def degree_power(a):
    """a (..., lmax, mmax) complex128 -> P (..., lmax)."""
    a = np.asarray(a)
    return (m_weights(*a.shape[-2:]) * (a.real ** 2 + a.imag ** 2)).sum(axis=-1)


@functools.lru_cache(maxsize=None)
def _sht(nlat, nlon, lmax, mmax, grid):
    return RealSHT(nlat, nlon, lmax=lmax, mmax=mmax, grid=grid)


@functools.lru_cache(maxsize=None)
def _isht(nlat, nlon, lmax, mmax, grid):
    return InverseRealSHT(nlat, nlon, lmax=lmax, mmax=mmax, grid=grid)


def coeffs64(x, grid, lmax=None, mmax=None):
    """Float64 coefficients (..., lmax, mmax) complex128 of x (..., nlat, nlon)."""
    x = torch.as_tensor(np.asarray(x)).double()
    return _sht(x.shape[-2], x.shape[-1], lmax, mmax, grid)(x).numpy()


def synthesise64(a, nlat, nlon, grid):
    a = torch.as_tensor(np.asarray(a))
    return _isht(nlat, nlon, a.shape[-2], a.shape[-1], grid)(a).numpy()


def random_coeffs(lmax, mmax, key, slope=0.0):
    """Random coefficients with m <= l and real m = 0; E|a[l,m]|^2 ~ (l + 1)^slope / (2 l + 1), so that P(l) ~ l^slope."""
    g = _gen("coeffs", lmax, mmax, key, slope)
    a = torch.randn(lmax, mmax, 2, generator=g, dtype=torch.float64).numpy()
    a = a[..., 0] + 1j * a[..., 1]
    a[:, 0] = a[:, 0].real
    l = np.arange(lmax)[:, None]
    a = a * np.sqrt((l + 1.0) ** slope / (2.0 * l + 1.0))
    return a * (m_weights(lmax, mmax) > 0)


def sphere_integral_of_square(f, grid):
    """Quadrature of f^2 over the sphere on the transform's own nodes."""
    nlat, nlon = f.shape[-2:]
    _, w = quadrature(nlat, grid)
    return ((f ** 2).sum(axis=-1) * w).sum(axis=-1) * (2.0 * np.pi / nlon)


# ---- fields of the end-to-end cases ------------------------------------------------------------------------------------------
def white(shape, nlat, nlon, key):
    return torch.randn(*shape, nlat, nlon, generator=_gen("white", shape, nlat, nlon, key)).numpy()


def red(shape, nlat, nlon, grid, key):
    """Fields with P(l) ~ l^-3: synthesised in float64 from random coefficients, cast to float32."""
    n = int(np.prod(shape))
    a = np.stack([random_coeffs(nlat, nlon // 2 + 1, (key, i), slope=-3.0) for i in range(n)])
    return synthesise64(a, nlat, nlon, grid).astype(np.float32).reshape(*shape, nlat, nlon)


@functools.lru_cache(maxsize=None)
def window_fields(nlat, nlon, grid, M, S, T, key=0):
    """{name: (gen (M, S, T, nlat, nlon), target (S, T, nlat, nlon))} float32: white noise, a red spectrum, and gen = target +
    1e-3 white noise (a small error spectrum under a large one)."""
    out = {}
    out["white"] = (white((M, S, T), nlat, nlon, (key, "g")), white((S, T), nlat, nlon, (key, "t")))
    out["red"] = (red((M, S, T), nlat, nlon, grid, (key, "g")), red((S, T), nlat, nlon, grid, (key, "t")))
    tgt = white((S, T), nlat, nlon, (key, "nt"))
    out["near"] = ((tgt[None] + np.float32(1e-3) * white((M, S, T), nlat, nlon, (key, "ng"))).astype(np.float32), tgt)
    return out


@functools.lru_cache(maxsize=None)
def reference_coeffs(nlat, nlon, grid, M, S, T, name, key=0):
    """Float64 coefficients of variable `name` of window_fields: gen (M, S, T, lmax, mmax), target (S, T, lmax, mmax)."""
    gen, target = window_fields(nlat, nlon, grid, M, S, T, key)[name]
    ag, at = coeffs64(gen, grid), coeffs64(target, grid)
    ag.setflags(write=False)
    at.setflags(write=False)
    return ag, at


@functools.lru_cache(maxsize=None)
def reference_rows(nlat, nlon, grid, M, S, T, name, key=0):
    """Float64 restatement of every row of variable `name` of window_fields: P of gen (M, S, T, lmax), of target (S, T, lmax)
    and of gen - target (M, S, T, lmax).  Computed once and shared; callers slice, never write."""
    ag, at = reference_coeffs(nlat, nlon, grid, M, S, T, name, key)
    rows = {"gen": degree_power(ag), "target": degree_power(at), "error": degree_power(ag - at[None])}
    for v in rows.values():
        v.setflags(write=False)
    return rows


def pooled(rows, members=slice(None), times=slice(None), eps=None):
    """(want, bound), each {"gen", "target", "error"} (T, lmax), of the chosen members and times: the pooled means the
    accumulators hold and the Cauchy-Schwarz bound of the module docstring, taken per row and averaged over the rows (the
    error rows use their generated row's d, the same absolute d)."""
    eps = EPS_SHT if eps is None else eps
    pg, pt, pe = rows["gen"][members][:, :, times], rows["target"][:, times], rows["error"][members][:, :, times]
    d_gen = eps * np.sqrt(pg.sum(axis=-1, keepdims=True))
    d_tgt = eps * np.sqrt(pt.sum(axis=-1, keepdims=True))
    want = {"gen": pg.mean(axis=(0, 1)), "target": pt.mean(axis=0), "error": pe.mean(axis=(0, 1))}
    bound = {"gen": (2.0 * np.sqrt(pg) * d_gen + d_gen ** 2).mean(axis=(0, 1)),
             "target": (2.0 * np.sqrt(pt) * d_tgt + d_tgt ** 2).mean(axis=0),
             "error": (2.0 * np.sqrt(pe) * d_gen + d_gen ** 2).mean(axis=(0, 1))}
    return want, bound


def sht_distance(a_dev, a_ref):
    """Relative weighted-L2 distance of coefficient tensors (..., lmax, mmax): what EPS_SHT bounds, per field."""
    w = m_weights(*a_ref.shape[-2:])
    num = (w * np.abs(np.asarray(a_dev, dtype=np.complex128) - a_ref) ** 2).sum(axis=(-2, -1))
    den = (w * np.abs(a_ref) ** 2).sum(axis=(-2, -1))
    return np.sqrt(num / den)


# ---- the reduction alone: internal layout, numpy sums, the host twin ---------------------------------------------------------
class Layout:
    """How the rows of (nvars, n0, n1, T) sit in the two coefficient buffers: the rows of one (variable, time) consecutive,
    groups `pad` fields apart from the next multiple of four (pad = None: packed tightly, no padding)."""

    def __init__(self, lmax, mtr, nvars, n0, n1, T, pad):
        self.lmax, self.mtr, self.nvars, self.n0, self.n1, self.T = lmax, mtr, nvars, n0, n1, T
        R = n0 * n1
        self.g_time = R if pad is None else (R + 3) // 4 * 4 + pad
        self.t_time = n1 if pad is None else (n1 + 3) // 4 * 4 + pad
        self.g_var, self.t_var = T * self.g_time, T * self.t_time
        self.Fg, self.Ft = nvars * self.g_var, nvars * self.t_var

    def gen_field(self, v, i0, i1, t):
        return v * self.g_var + t * self.g_time + i0 * self.n1 + i1

    def target_field(self, v, i1, t):
        return v * self.t_var + t * self.t_time + i1


def random_case(lay, key, scaled=False):
    """Coefficient buffers Cs[l][m][ri][field] float32 of a Layout: normals in the fields the layout names, NaN in every
    padding field and in every entry with m > l.  With `scaled`, per-field powers of two between 2^-3 and 2^20."""
    g = _gen("case", lay.lmax, lay.mtr, lay.nvars, lay.n0, lay.n1, lay.T, lay.g_time, key)
    bufs = []
    for F, used in ((lay.Fg, {lay.gen_field(v, i0, i1, t) for v in range(lay.nvars) for i0 in range(lay.n0)
                              for i1 in range(lay.n1) for t in range(lay.T)}),
                    (lay.Ft, {lay.target_field(v, i1, t) for v in range(lay.nvars) for i1 in range(lay.n1)
                              for t in range(lay.T)})):
        cs = torch.randn(lay.lmax, lay.mtr, 2, F, generator=g).numpy()
        pad = np.array([f not in used for f in range(F)])
        cs[..., pad] = np.nan
        cs[m_weights(lay.lmax, lay.mtr) == 0] = np.nan
        bufs.append(np.ascontiguousarray(cs, dtype=np.float32))
    scales = [None, None]
    if scaled:
        for i, F in enumerate((lay.Fg, lay.Ft)):
            e = torch.randint(-3, 21, (F,), generator=g).numpy()
            scales[i] = np.ascontiguousarray(2.0 ** e, dtype=np.float32)
    return bufs[0], bufs[1], scales[0], scales[1]


def numpy_reduction(lay, cg, ct, sg=None, st=None):
    """The three accumulator contributions (nvars, T, lmax) and the cross term, float64 numpy on the same fp32 numbers."""
    w = m_weights(lay.lmax, lay.mtr)[:, :, None]                                       # [l][m][1]
    cg, ct = cg.astype(np.float64), ct.astype(np.float64)
    if sg is not None:
        cg, ct = cg * sg.astype(np.float64), ct * st.astype(np.float64)
    out = {k: np.zeros((lay.nvars, lay.T, lay.lmax)) for k in ("gen", "target", "error", "cross")}
    for v in range(lay.nvars):
        for t in range(lay.T):
            tf = [lay.target_field(v, i1, t) for i1 in range(lay.n1)]
            gf = [lay.gen_field(v, i0, i1, t) for i0 in range(lay.n0) for i1 in range(lay.n1)]
            tt = [lay.target_field(v, i1, t) for i0 in range(lay.n0) for i1 in range(lay.n1)]
            G, Tt, Tr = cg[..., gf], ct[..., tf], ct[..., tt]                           # [l][m][ri][rows]
            with np.errstate(invalid="ignore"):
                pw = lambda a: np.where(w > 0, w * (a ** 2).sum(axis=2), 0.0).sum(axis=1)        # noqa: E731  [l][rows]
                out["gen"][v, t] = pw(G).mean(axis=-1)
                out["target"][v, t] = pw(Tt).mean(axis=-1)
                out["error"][v, t] = pw(G - Tr).mean(axis=-1)
                out["cross"][v, t] = np.where(w > 0, w * (G * Tr).sum(axis=2), 0.0).sum(axis=1).mean(axis=-1)
    return out


def reduction_bound(lay):
    """Relative bound 2 (n + 4) 2^-53 per (label, degree): n = rows x orders x 2 terms summed into the element."""
    orders = np.minimum(np.arange(lay.lmax), lay.mtr - 1) + 1.0
    n_gen, n_tgt = lay.n0 * lay.n1 * orders * 2.0, lay.n1 * orders * 2.0
    return {"gen": 2.0 * (n_gen + 4.0) * U, "target": 2.0 * (n_tgt + 4.0) * U, "error": 2.0 * (n_gen + 4.0) * U}


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def fill_args(lay, gen, target, gen_scale, target_scale, t_start, n_timesteps, acc):
    """SdySpectrumArgs from raw addresses (host arrays or device pointers): gen, target, scales and acc are integers / None."""
    from sdy_amd._lib import SdySpectrumArgs

    a = SdySpectrumArgs()
    a.gen, a.target = gen, target
    fill_rows(a.rows, lay, gen_scale, target_scale, t_start, n_timesteps)
    a.gen_power, a.target_power, a.err_power = acc
    return a


def fill_rows(rows, lay, gen_scale, target_scale, t_start, n_timesteps, components=1):
    """The sdy_coef_rows of a Layout, by the package's own `_fill_rows`; a buffer holds `components` runs of the layout's
    fields (2: the u run and the v run of tests/vector_spectrum_utils.py)."""
    from sdy_amd.spectrum import _fill_rows

    _fill_rows(rows, lay, gen_scale, target_scale, (components * lay.Fg, lay.g_var, lay.g_time),
               (components * lay.Ft, lay.t_var, lay.t_time), lay.nvars, lay.n0, lay.n1, lay.T, t_start, n_timesteps)


def host_accumulate(lay, cg, ct, sg, st, t_start, acc, with_error=True):
    """One sdy_degree_power_host call adding to acc = {"gen", "target", "error"} float64 (nvars, n_timesteps, lmax)."""
    import sdy_amd

    addr = lambda x: None if x is None else x.ctypes.data      # noqa: E731
    a = fill_args(lay, addr(cg), addr(ct), addr(sg), addr(st), t_start, acc["gen"].shape[1],
                  (addr(acc["gen"]), addr(acc["target"]), addr(acc["error"]) if with_error else None))
    return sdy_amd.lib.sdy_degree_power_host(C.byref(a))


# The cases of the reduction: (lmax, mtr) full and truncated orders; (n0, n1, T) an ensemble window and a single row; pad None
# (tight: odd strides, the 4-byte path on the device), 0 (groups on multiples of four: the 16-byte path) and 4 (whole padding
# groups in between); one case with more rows than slots (260 > 256).
REDUCTION_CASES = [(lmax, mtr, n0, n1, T, pad, scaled)
                   for lmax, mtr in ((12, 12), (7, 5)) for n0, n1, T in ((3, 2, 3), (1, 1, 1)) for pad, scaled in
                   ((None, False), (0, False), (4, True))] + [(4, 3, 65, 4, 3, 0, False), (4, 3, 65, 4, 3, None, True)]


def case_id(c):
    lmax, mtr, n0, n1, T, pad, scaled = c
    return f"l{lmax}m{mtr}-{n0}x{n1}x{T}-pad{pad}" + ("-scaled" if scaled else "")
