"""Vorticity, divergence, streamfunction and velocity potential without a GPU: the factor rows of sdy_helmholtz_factors_host
against numpy, the host twin sdy_helmholtz_coefficients_host -- it compiles the header the kernel compiles, csrc/helmholtz.h --
against numpy on the same fp32 numbers BIT FOR BIT, the identities that pin the definition in float64 with the library's own
tables, solid-body rotation (the arbiter of the signs), and every refusal.  Restatement: tests/helmholtz_utils.py."""
import ctypes as C

import numpy as np
import pytest

import helmholtz_utils as hu
import vector_spectrum_utils as vu
from oracle.sht import quadrature
from sdy_amd.helmholtz import OUTPUTS  # noqa: F401  (the feature under test)


# ---- the factor rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lmax,truncate", [(1, None), (12, None), (180, None), (180, 90), (12, 0), (12, 40)])
def test_factor_rows(lmax, truncate):
    rows = [hu.host_factors(lmax, hu.RADIUS, kind, truncate) for kind in (0, 1)]
    for kind, row in enumerate(rows):
        want = hu.factors64(lmax, hu.RADIUS, kind, truncate)
        err = np.abs(row - want) / np.abs(want).clip(1e-300)
        print(f"lmax {lmax} truncate {truncate} kind {kind}: worst relative distance from numpy {err.max():.1e}")
        assert (err <= 2.0 ** -52).all()
        assert row[0] == 0.0
    top = lmax - 1 if truncate is None else min(truncate, lmax - 1)
    assert (rows[0][top + 1:] == 0).all() and (rows[1][top + 1:] == 0).all()
    assert (rows[0][1:top + 1] < 0).all() and (rows[1][1:top + 1] > 0).all()
    assert np.abs(rows[0][1:top + 1] * rows[1][1:top + 1] + 1.0).max(initial=0.0) <= 4.0 * 2.0 ** -53


def test_factor_arguments():
    import sdy_amd

    f = sdy_amd.lib.sdy_helmholtz_factors_host
    out = np.zeros(4)
    assert f(4, hu.RADIUS, 0, -1, out.ctypes.data) == 0
    for bad in ((0, hu.RADIUS, 0, -1, out.ctypes.data), (4, 0.0, 0, -1, out.ctypes.data), (4, -1.0, 0, -1, out.ctypes.data),
                (4, float("nan"), 0, -1, out.ctypes.data), (4, float("inf"), 1, -1, out.ctypes.data),
                (4, hu.RADIUS, 2, -1, out.ctypes.data), (4, hu.RADIUS, -1, -1, out.ctypes.data), (4, hu.RADIUS, 0, -1, None)):
        assert f(*bad) == hu.SDY_ERR_ARG, bad


# ---- the host twin -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", hu.CASES, ids=lambda c: c.id)
def test_host_twin_against_numpy(case):
    cd, cm, scale, factor = hu.random_inputs(case)
    cd, cm, scale = hu.aligned_copy(cd), hu.aligned_copy(cm), hu.aligned_copy(scale)
    raw, out, lead = hu.guarded_out(case)
    assert hu.host_run(case, cd, cm, scale, factor, out) == 0
    want = hu.numpy_kernel(case, cd, cm, scale, factor)
    assert hu.guards_intact(raw, lead, out.size)
    assert not np.isnan(out).any(), "a padding field or an entry with m > l was read, or a field of out was not written"
    assert hu.bits_equal(out, want)
    named = np.zeros(case.out_fields, dtype=bool)
    for q in range(len(case.names)):
        named[q * case.out_stride:q * case.out_stride + case.n_winds] = True
    assert (out[..., ~named] == 0).all()                                               # fields no output names
    assert (out[0] == 0).all()                                                         # row l = 0
    assert (out[vu.su.m_weights(case.lmax, case.mtr) == 0] == 0).all()                 # m > l
    assert (out[1:, 0][..., named] != 0).any()


def test_a_wind_does_not_depend_on_its_company():
    """The first wind of the five-wind layout alone, in the one-wind layout: the same bits."""
    five = next(c for c in hu.CASES if c.n_winds == 5 and len(c.names) == 4 and c.scaled and c.lmax == 12)
    one = next(c for c in hu.CASES if c.n_winds == 1 and len(c.names) == 4 and c.scaled and c.lmax == 12)
    cd, cm, scale, factor = hu.random_inputs(five)
    _, out5, _ = hu.guarded_out(five)
    assert hu.host_run(five, hu.aligned_copy(cd), hu.aligned_copy(cm), hu.aligned_copy(scale), factor, out5) == 0
    pick = [five.u_offset, 0, 0, 0, five.v_offset, 0, 0, 0]
    cd1, cm1, scale1 = (np.ascontiguousarray(a[..., pick]) for a in (cd, cm, scale))
    _, out1, _ = hu.guarded_out(one)
    assert hu.host_run(one, hu.aligned_copy(cd1), hu.aligned_copy(cm1), hu.aligned_copy(scale1), factor, out1) == 0
    for q in range(4):
        assert hu.bits_equal(out5[..., q * five.out_stride], out1[..., q * one.out_stride]), q


# ---- identities in float64 with the library's host tables --------------------------------------------------------------------
def _lg16():
    nlat, nlon, grid = 16, 32, "legendre-gauss"
    lmax, mmax = 16, nlon // 2 + 1
    D, M = vu.host_tables(nlat, nlon, lmax, mmax, grid)
    _, w = quadrature(nlat, grid)
    return nlat, nlon, grid, lmax, mmax, D, M, w


def _scalar_table(nlat, nlon, lmax, mmax, grid):
    """The LIBRARY's scalar table: sdy_sht_tables_host."""
    import sdy_amd

    P = np.full((mmax, lmax, nlat), np.nan)
    assert sdy_amd.lib.sdy_sht_tables_host(nlat, nlon, lmax, mmax, vu.GRID_ID[grid], P.ctypes.data, None, None) == 0
    return P


def _synth(c, P, nlon):
    return np.fft.irfft(np.einsum("lm,mlk->km", c, P), n=nlon, axis=-1, norm="forward")


def test_analysis_and_factors_reproduce_the_definitions():
    nlat, nlon, grid, lmax, mmax, D, M, w = _lg16()
    a = hu.RADIUS
    n = np.sqrt(np.arange(lmax) * (np.arange(lmax) + 1.0))[:, None]
    for key in range(3):
        s, t = vu.random_st(lmax, mmax, ("hh", key), slope=-1.0 * key, below=10)
        u, v = vu.synthesise64(s, t, nlat, nlon, grid, tables=(D, M))
        s2, t2 = vu.analyse_with(u, v, D, M, w, mmax)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = np.where(n > 0, a / n, 0.0)
        for name, got, want in (("vorticity", t2 * hu.host_factors(lmax, a, 0)[:, None], -n * t / a),
                                ("divergence", s2 * hu.host_factors(lmax, a, 0)[:, None], -n * s / a),
                                ("streamfunction", t2 * hu.host_factors(lmax, a, 1)[:, None], inv * t),
                                ("velocity_potential", s2 * hu.host_factors(lmax, a, 1)[:, None], inv * s)):
            err = np.abs(got - want).max() / np.abs(want).max()
            print(f"wind {key} {name}: {err:.1e} of the scale")
            assert err <= 1e-12, name


def test_pure_toroidal_and_pure_spheroidal_winds():
    nlat, nlon, grid, lmax, mmax, D, M, w = _lg16()
    P = _scalar_table(nlat, nlon, lmax, mmax, grid)
    s, t = vu.random_st(lmax, mmax, "hh-pure", below=10)
    zero = np.zeros_like(s)
    f = [hu.host_factors(lmax, hu.RADIUS, kind)[:, None] for kind in (0, 1)]
    for name, (cs, ct) in (("toroidal", (zero, t)), ("spheroidal", (s, zero))):
        u, v = vu.synthesise64(cs, ct, nlat, nlon, grid, tables=(D, M))
        s2, t2 = vu.analyse_with(u, v, D, M, w, mmax)
        fields = {"vorticity": _synth(t2 * f[0], P, nlon), "divergence": _synth(s2 * f[0], P, nlon),
                  "streamfunction": _synth(t2 * f[1], P, nlon), "velocity_potential": _synth(s2 * f[1], P, nlon)}
        pairs = (("divergence", "vorticity"), ("velocity_potential", "streamfunction"))
        for a_, b_ in pairs:
            small, large = (a_, b_) if name == "toroidal" else (b_, a_)
            ratio = np.abs(fields[small]).max() / np.abs(fields[large]).max()
            print(f"{name}: {small} is {ratio:.1e} of {large}")
            assert ratio <= 1e-12


def test_vorticity_is_the_laplacian_of_the_streamfunction():
    """A scalar synthesis of the zeta coefficients equals the synthesis of -l (l + 1) / a^2 times psi's (and delta, chi)."""
    nlat, nlon, grid, lmax, mmax, D, M, w = _lg16()
    P = _scalar_table(nlat, nlon, lmax, mmax, grid)
    s, t = vu.random_st(lmax, mmax, "hh-laplace", slope=-1.0, below=10)
    u, v = vu.synthesise64(s, t, nlat, nlon, grid, tables=(D, M))
    s2, t2 = vu.analyse_with(u, v, D, M, w, mmax)
    f = [hu.host_factors(lmax, hu.RADIUS, kind)[:, None] for kind in (0, 1)]
    lap = -(np.arange(lmax) * (np.arange(lmax) + 1.0))[:, None] / hu.RADIUS ** 2
    for name, x in (("vorticity / streamfunction", t2), ("divergence / velocity potential", s2)):
        got, want = _synth(x * f[0], P, nlon), _synth(lap * (x * f[1]), P, nlon)
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"{name}: {err:.1e} of the scale")
        assert err <= 1e-12 and np.abs(want).max() > 0


@pytest.mark.parametrize("grid", vu.GRIDS)
def test_solid_body_rotation(grid):
    """u = U cos(lat), v = 0: zeta = 2 U sin(lat) / a, psi = -a U sin(lat), delta = chi = 0.  This fixes the signs.

    Degrees up to nlat - 2 are kept (`truncate`): the analysis of this wind at degree l integrates a polynomial of degree l + 1
    in cos(theta), and the equiangular (Clenshaw-Curtis) rule of nlat nodes is exact up to degree nlat - 1 only, so its
    coefficient at l = nlat - 1 is an alias (printed below; the Legendre-Gauss grid has none) -- what DESIGN.md section 7v says
    about lmax = nlat on that grid, and what `truncate` is for."""
    nlat, nlon, U, a = 12, 24, 30.0, hu.RADIUS
    lmax, mmax = nlat, nlon // 2 + 1
    D, M = vu.host_tables(nlat, nlon, lmax, mmax, grid)
    P = _scalar_table(nlat, nlon, lmax, mmax, grid)
    _, w = quadrature(nlat, grid)
    u, v, lat = hu.solid_body(nlat, nlon, grid, U)
    s, t = vu.analyse_with(u, v, D, M, w, mmax)
    want = {"vorticity": 2.0 * U * np.sin(lat) / a, "streamfunction": -a * U * np.sin(lat)}
    scale = {"vorticity": 2.0 * U / a, "divergence": 2.0 * U / a, "streamfunction": a * U, "velocity_potential": a * U}
    for truncate in (None, nlat - 2):
        for name in hu.OUTPUTS:
            c = (t if hu.PART[name] else s) * hu.host_factors(lmax, a, hu.KIND[name], truncate)[:, None]
            got = _synth(c, P, nlon)
            ref = want[name][:, None] if name in want else 0.0
            err = np.abs(got - ref).max() / scale[name]
            print(f"{grid} truncate {truncate} {name}: {err:.1e} of the scale")
            if truncate is not None or grid == "legendre-gauss":
                assert err <= 1e-12, (name, truncate)
    zeta = _synth(t * hu.host_factors(lmax, a, 0, nlat - 2)[:, None], P, nlon)
    assert (zeta[lat > 0.1] > 0).all() and (zeta[lat < -0.1] < 0).all()           # cyclonic in the north for a westerly jet


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_out_untouched():
    import sdy_amd

    case = next(c for c in hu.CASES if c.n_winds == 5 and len(c.names) == 4 and c.scaled and c.lmax == 7)
    cd, cm, scale, factor = hu.random_inputs(case)
    cd, cm, scale = hu.aligned_copy(cd), hu.aligned_copy(cm), hu.aligned_copy(scale)
    raw, out, lead = hu.guarded_out(case)
    addr = lambda x: x.ctypes.data      # noqa: E731

    def args(**kw):
        a = hu.fill_args(case, addr(cd), addr(cm), addr(scale), addr(factor), addr(out))
        for k, v in kw.items():
            if k == "part":
                a.part[v[0]] = v[1]
            else:
                setattr(a, k, v)
        return a

    host, dev = sdy_amd.lib.sdy_helmholtz_coefficients_host, sdy_amd.lib.sdy_helmholtz_coefficients
    ARG, ALIGN = hu.SDY_ERR_ARG, hu.SDY_ERR_ALIGN
    bad = [(dict(Cs_d=None), ARG), (dict(Cs_m=None), ARG), (dict(factor=None), ARG), (dict(out=None), ARG),
           (dict(n_out=0), ARG), (dict(n_out=5), ARG), (dict(part=(0, 2)), ARG), (dict(part=(3, -1)), ARG),
           (dict(u_offset=-4), ARG), (dict(v_offset=-4), ARG), (dict(u_offset=20), ARG), (dict(v_offset=20), ARG),
           (dict(n_winds=0), ARG), (dict(n_winds=9), ARG), (dict(out_fields=40), ARG), (dict(out_stride=4), ARG),
           (dict(out_stride=-4), ARG), (dict(out_stride=16), ARG), (dict(lmax=0), ARG), (dict(mtr=0), ARG),
           (dict(struct_size=0), ARG), (dict(struct_size=C.sizeof(type(args())) + 8), ARG),
           (dict(out=addr(cd)), ARG), (dict(out=addr(cm) + 16), ARG),                     # out overlaps an input
           (dict(fields=22), ALIGN), (dict(out_fields=54), ALIGN), (dict(u_offset=2), ALIGN), (dict(v_offset=18), ALIGN),
           (dict(out_stride=14), ALIGN), (dict(Cs_d=addr(cd) + 4), ALIGN), (dict(Cs_m=addr(cm) + 8), ALIGN),
           (dict(scale=addr(scale) + 4), ALIGN), (dict(out=addr(out) + 4), ALIGN), (dict(factor=addr(factor) + 4), ALIGN)]
    for kw, code in bad:
        assert host(C.byref(args(**kw))) == code, kw
        assert dev(C.byref(args(**kw)), None) == code, kw                                 # refused before anything is launched
    assert host(None) == ARG and dev(None, None) == ARG
    assert np.isnan(raw).all(), "a refused call wrote to out"
    assert np.isnan(cd).any() and host(C.byref(args())) == 0 and not np.isnan(out).any()
    assert host(C.byref(args(scale=None))) == 0                                           # NULL scale is a valid call


def test_the_structure_carries_its_size():
    from sdy_amd import _lib

    a = _lib.SdyHelmholtzArgs()
    assert a.struct_size == C.sizeof(_lib.SdyHelmholtzArgs) and _lib.SdyHelmholtzArgs not in _lib.ABI_STRUCTS
    assert {"sdy_helmholtz_factors_host", "sdy_helmholtz_coefficients", "sdy_helmholtz_coefficients_host"} <= set(_lib.SIGNATURES)


def test_deriver_names_and_chain_without_a_device():
    """What needs no tensor arithmetic: the clash, the skipped pairs, the CPU refusal, and `derived.chain`."""
    import torch

    import sdy_amd
    from sdy_amd.helmholtz import deriver, helmholtz

    names = ["eastward_wind_0", "northward_wind_0", "UGRD10m", "VGRD10m", "eastward_wind_3", "TMP2m"]
    d = deriver(names)
    z = torch.zeros(2, 3, 12, 24)
    same = d({"TMP2m": z, "eastward_wind_0": z})                                          # no complete pair: nothing to do
    assert list(same) == ["TMP2m", "eastward_wind_0"]
    with pytest.raises(ValueError, match="vorticity_0 already exists"):
        d({"eastward_wind_0": z, "northward_wind_0": z, "vorticity_0": z})
    with pytest.raises(RuntimeError, match="GPU only"):
        d({"eastward_wind_0": z, "northward_wind_0": z})
    with pytest.raises(RuntimeError, match="GPU only"):
        helmholtz(z, z)
    with pytest.raises(ValueError, match="outputs"):
        deriver(names, outputs=("vorticity", "shear"))
    with pytest.raises(TypeError, match="unexpected"):
        deriver(names, nlat=12)
    calls = []
    both = sdy_amd.derived.chain(lambda x: calls.append("a") or {**x, "a": 1},
                                 lambda x: calls.append("b") or {**x, "b": x["a"] + 1})
    assert both({"x": 0}) == {"x": 0, "a": 1, "b": 2} and calls == ["a", "b"]
    assert sdy_amd.derived.chain()({"x": 0}) == {"x": 0}
