"""Rotational / divergent kinetic-energy spectra without a GPU: the library's host tables (sdy_vsht_tables_host) against the
float64 restatement and an independent form, the identities that pin the definition (recovery, Parseval, pure toroidal and
spheroidal winds, solid-body rotation), and the host twin sdy_vector_degree_power_host -- it compiles the header the kernel
compiles, csrc/vector_spectrum.h -- against numpy float64 on the same fp32 numbers.  Restatement and bounds:
tests/vector_spectrum_utils.py."""
import ctypes as C

import numpy as np
import pytest

import spectrum_utils as su
import vector_spectrum_utils as vu
from oracle.sht import legpoly, quadrature


@pytest.mark.parametrize("grid", vu.GRIDS)
@pytest.mark.parametrize("nlat,nlon", [(12, 24), (180, 360)])
def test_tables_against_the_restatement(grid, nlat, nlon):
    lmax, mmax = nlat, nlon // 2 + 1
    d, m = vu.host_tables(nlat, nlon, lmax, mmax, grid)
    D, M, _, _ = vu.tables64(nlat, nlon, lmax, mmax, grid)
    for name, got, want in (("D", d, D), ("M", m, M)):
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"{grid} {nlat} x {nlon} {name}: worst |difference| / largest entry = {err:.2e}")
        assert err <= 1e-12
    assert (d[:, 0] == 0).all() and (m[:, 0] == 0).all()          # row l = 0


@pytest.mark.parametrize("grid", vu.GRIDS)
@pytest.mark.parametrize("nlat,nlon", [(12, 24), (180, 360)])
def test_tables_against_an_independent_form(grid, nlat, nlon):
    """At interior nodes dP/dtheta = -[(l + 1) eps_l^m P_{l-1}^m - l eps_{l+1}^m P_{l+1}^m] / sin(theta) with
    eps_l^m = sqrt((l^2 - m^2) / (4 l^2 - 1)), for l < lmax - 1; and m P / sin(theta)."""
    lmax, mmax = nlat, nlon // 2 + 1
    d, m = vu.host_tables(nlat, nlon, lmax, mmax, grid)
    theta, _ = quadrature(nlat, grid)
    P = legpoly(mmax, lmax, np.cos(theta))
    inner = slice(1, nlat - 1) if grid == "equiangular" else slice(None)
    sin = np.sin(theta[inner])
    l = np.arange(lmax, dtype=np.float64)[None, :, None]
    mm = np.arange(mmax, dtype=np.float64)[:, None, None]
    with np.errstate(invalid="ignore"):
        eps = np.where(l >= mm, np.sqrt((l * l - mm * mm) / (4.0 * l * l - 1.0)), 0.0)          # [m][l][1]
    norm = np.sqrt(l * (l + 1.0))
    ls = slice(1, lmax - 1)
    lower = np.concatenate([np.zeros_like(P[:, :1]), P[:, :-1]], axis=1)                          # P_{l-1}
    upper = np.concatenate([P[:, 1:], np.zeros_like(P[:, :1])], axis=1)                           # P_{l+1}
    eps_up = np.concatenate([eps[:, 1:], np.zeros_like(eps[:, :1])], axis=1)
    want_d = (-((l + 1.0) * eps * lower - l * eps_up * upper)[:, ls, inner] / sin / norm[:, ls])
    want_d = np.where(mm > l[:, ls], 0.0, want_d)
    want_m = (mm * P)[:, 1:, inner] / sin / norm[:, 1:]
    scale_d, scale_m = np.abs(d).max(), np.abs(m).max()
    err_d = np.abs(d[:, ls, inner] - want_d).max() / scale_d
    err_m = np.abs(m[:, 1:, inner] - want_m).max() / scale_m
    print(f"{grid} {nlat} x {nlon}: D {err_d:.2e}, M {err_m:.2e} of the largest entry")
    assert err_d <= 1e-12 and err_m <= 1e-12


@pytest.mark.parametrize("nlat,nlon", [(12, 24), (180, 360)])
def test_pole_columns_of_the_equiangular_tables(nlat, nlon):
    lmax, mmax = nlat, nlon // 2 + 1
    d, m = vu.host_tables(nlat, nlon, lmax, mmax, "equiangular")
    for k in (0, nlat - 1):
        assert (m[0, :, k] == 0).all() and (m[2:, :, k] == 0).all()
        assert (d[0, :, k] == 0).all() and (d[2:, :, k] == 0).all()
        assert np.abs(d[1, 1:, k]).min() > 0
    assert np.array_equal(m[1, :, 0], d[1, :, 0]) and np.array_equal(m[1, :, -1], -d[1, :, -1])


def test_table_arguments():
    import sdy_amd

    f = sdy_amd.lib.sdy_vsht_tables_host
    a = np.zeros((5, 4, 8))
    p = a.ctypes.data
    assert f(8, 16, 4, 5, 0, p, p) == 0
    for bad in ((1, 16, 4, 5, 0, p, p), (8, 1, 4, 5, 0, p, p), (8, 16, 0, 5, 0, p, p), (8, 16, 4, 0, 0, p, p),
                (8, 16, 4, 5, 7, p, p), (8, 16, 4, 5, 0, None, p), (8, 16, 4, 5, 0, p, None)):
        assert f(*bad) == su.SDY_ERR_ARG, bad


# ---- identities: the restatement's formulas fed with the library's host tables ----------------------------------------------
def _lg16():
    nlat, nlon, grid = 16, 32, "legendre-gauss"
    lmax, mmax = 16, nlon // 2 + 1
    D, M = vu.host_tables(nlat, nlon, lmax, mmax, grid)
    _, w = quadrature(nlat, grid)
    return nlat, nlon, grid, lmax, mmax, D, M, w


def test_recovery_and_parseval_on_the_legendre_gauss_grid():
    nlat, nlon, grid, lmax, mmax, D, M, w = _lg16()
    for key in range(3):
        s, t = vu.random_st(lmax, mmax, key, slope=-1.0 * key, below=10)
        u, v = vu.synthesise64(s, t, nlat, nlon, grid, tables=(D, M))
        s2, t2 = vu.analyse_with(u, v, D, M, w, mmax)
        scale = max(np.abs(s).max(), np.abs(t).max())
        err = max(np.abs(s2 - s).max(), np.abs(t2 - t).max()) / scale
        total = (vu.energy(s2) + vu.energy(t2)).sum()
        quad = 0.5 * (su.sphere_integral_of_square(u, grid) + su.sphere_integral_of_square(v, grid))
        print(f"wind {key}: coefficients recovered to {err:.1e}; sum E = {total:.16e}, quadrature {quad:.16e}, "
              f"rel {abs(total - quad) / quad:.1e}")
        assert err <= 1e-12
        assert abs(total - quad) <= 1e-12 * quad


def test_pure_toroidal_and_pure_spheroidal_winds():
    nlat, nlon, grid, lmax, mmax, D, M, w = _lg16()
    s, t = vu.random_st(lmax, mmax, "pure", below=10)
    zero = np.zeros_like(s)
    for name, (cs, ct) in (("toroidal", (zero, t)), ("spheroidal", (s, zero))):
        u, v = vu.synthesise64(cs, ct, nlat, nlon, grid, tables=(D, M))
        s2, t2 = vu.analyse_with(u, v, D, M, w, mmax)
        e_div, e_rot = vu.energy(s2).sum(), vu.energy(t2).sum()
        small, large = (e_div, e_rot) if name == "toroidal" else (e_rot, e_div)
        print(f"{name}: the other part holds {small / large:.1e} of the energy")
        assert small <= 1e-24 * large


@pytest.mark.parametrize("grid", vu.GRIDS)
def test_solid_body_rotation(grid):
    nlat, nlon = 12, 24
    lmax, mmax = nlat, nlon // 2 + 1
    D, M = vu.host_tables(nlat, nlon, lmax, mmax, grid)
    theta, w = quadrature(nlat, grid)
    u = np.repeat(np.sin(theta)[:, None], nlon, axis=1)           # cos(latitude)
    v = np.zeros_like(u)
    s, t = vu.analyse_with(u, v, D, M, w, mmax)
    e_rot, e_div = vu.energy(t), vu.energy(s)
    print(f"{grid}: E_rot(1) = {e_rot[1]:.16e}, 4 pi / 3 = {4.0 * np.pi / 3.0:.16e}; largest E_div {e_div.max():.1e}")
    assert abs(e_rot[1] - 4.0 * np.pi / 3.0) <= 1e-12
    assert (e_div == 0).all()


# ---- the host twin -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", vu.REDUCTION_CASES, ids=vu.case_id)
def test_host_twin_against_numpy(case):
    lmax, mtr, n0, n1, T, pad, scaled = case
    lay = vu.Layout(lmax, mtr, 2, n0, n1, T, pad)
    acc = {k: np.zeros((2, 6, lmax)) for k in vu.ACCS}
    want = {k: np.zeros((2, 6, lmax)) for k in vu.ACCS}
    for w, t_start in enumerate((0, 3)):
        bufs = vu.random_case(lay, w, scaled)
        assert vu.host_accumulate(lay, bufs, t_start, acc) == 0
        ref = vu.numpy_reduction(lay, *bufs)
        for k in want:
            want[k][:, t_start:t_start + T] += ref[k]
    bound = vu.reduction_bound(lay)
    untouched = [t for t in range(6) if not (0 <= t < T or 3 <= t < 3 + T)]
    for k in vu.ACCS:
        assert not np.isnan(acc[k]).any(), f"{k}: a padding field or an entry with m > l was read"
        err = np.abs(acc[k] - want[k])
        print(f"{k}: worst |err| / bound = {(err / (bound[k] * want[k]).clip(1e-300)).max():.3f}")
        assert (err <= bound[k] * want[k]).all(), k
        assert (want[k][:, :T, 1:] > 0).all(), k
        assert (acc[k][:, untouched] == 0.0).all(), k


def test_without_the_error_accumulators():
    lay = vu.Layout(7, 5, 2, 3, 2, 3, 0)
    bufs = vu.random_case(lay, 0)
    full = {k: np.zeros((2, 3, 7)) for k in vu.ACCS}
    part = {k: np.zeros((2, 3, 7)) for k in vu.ACCS}
    assert vu.host_accumulate(lay, bufs, 0, full) == 0
    assert vu.host_accumulate(lay, bufs, 0, part, with_error=False) == 0
    for k in vu.ACCS[:4]:
        assert np.array_equal(full[k], part[k]), k
    for k in vu.ACCS[4:]:
        assert (part[k] == 0.0).all() and (full[k] > 0.0).all(), k


def test_error_codes():
    """What the entry points check themselves; the descriptor's fields: tests/test_coef_rows_host.py."""
    import sdy_amd

    lay = vu.Layout(7, 5, 2, 3, 2, 3, 0)
    bufs = vu.random_case(lay, 0)
    acc = {k: np.zeros((2, 6, 7)) for k in vu.ACCS}
    addr = lambda x: None if x is None else x.ctypes.data      # noqa: E731

    def args(**kw):
        a = vu.fill_args(lay, *[addr(b) for b in bufs], 0, 6, tuple(addr(acc[k]) for k in vu.ACCS))
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    host, dev = sdy_amd.lib.sdy_vector_degree_power_host, sdy_amd.lib.sdy_vector_degree_power
    assert host(C.byref(args())) == 0
    before = {k: v.copy() for k, v in acc.items()}
    bad = [{k: None} for k in ("gen_d", "gen_m", "target_d", "target_m", "gen_rot", "gen_div", "target_rot", "target_div",
                               "err_rot", "err_div")]                       # one error accumulator without the other
    bad += [{k: -4} for k in ("gen_v_offset", "target_v_offset")]
    bad += [dict(gen_v_offset=lay.Fg + 4), dict(target_v_offset=lay.Ft + 4), dict(gen_v_offset=2 ** 31 - 1),
            dict(struct_size=0), dict(struct_size=C.sizeof(type(args())) + 8)]
    for kw in bad:
        assert host(C.byref(args(**kw))) == su.SDY_ERR_ARG, kw
        assert dev(C.byref(args(**kw)), None) == su.SDY_ERR_ARG, kw            # refused before anything is launched
    assert host(None) == su.SDY_ERR_ARG and dev(None, None) == su.SDY_ERR_ARG
    assert all(np.array_equal(acc[k], before[k]) for k in acc)
    # error accumulators both NULL is a valid call
    assert host(C.byref(args(err_rot=None, err_div=None))) == 0


def test_the_structure_carries_its_size():
    from sdy_amd import _lib

    a = _lib.SdyVectorSpectrumArgs()
    assert a.struct_size == C.sizeof(_lib.SdyVectorSpectrumArgs) and _lib.SdyVectorSpectrumArgs not in _lib.ABI_STRUCTS
    assert {"sdy_vsht_tables_host", "sdy_vsht_plan_create", "sdy_vsht_plan_destroy", "sdy_vector_legendre_fwd",
            "sdy_vector_degree_power", "sdy_vector_degree_power_host"} <= set(_lib.SIGNATURES)
