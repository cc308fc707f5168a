"""Spherical power spectra without a GPU: the float64 restatement's normalisation (Parseval on the Legendre-Gauss grid), and
the library's host twin sdy_degree_power_host -- it compiles the header the kernel compiles, csrc/spectrum.h -- against
numpy float64 on the same fp32 coefficients.  Bounds: tests/spectrum_utils.py."""
import ctypes as C

import numpy as np
import pytest

import spectrum_utils as su


def test_parseval_on_the_legendre_gauss_grid():
    """sum_l P(l) = integral of f^2 for band-limited fields: pins the m-weights and the normalisation (measured 4e-16)."""
    nlat, nlon, grid = 12, 24, "legendre-gauss"
    for key in range(4):
        a = su.random_coeffs(nlat, nlon // 2 + 1, key, slope=-1.0 * key)
        f = su.synthesise64(a, nlat, nlon, grid)
        total, quad = su.degree_power(a).sum(), su.sphere_integral_of_square(f, grid)
        print(f"field {key}: sum P = {total:.16e}, quadrature = {quad:.16e}, rel {abs(total - quad) / quad:.1e}")
        assert abs(total - quad) <= 1e-12 * quad
        # and the forward restatement returns the coefficients the field was made of
        back = su.degree_power(su.coeffs64(f, grid))
        assert np.abs(back - su.degree_power(a)).max() <= 1e-12 * total


def _two_windows(case, run):
    """Two windows at t_start = 0 and 3 of n_timesteps = 6 through `run(lay, bufs, t_start, acc)`; returns (lay, want, acc)."""
    lmax, mtr, n0, n1, T, pad, scaled = case
    lay = su.Layout(lmax, mtr, 2, n0, n1, T, pad)
    acc = {k: np.zeros((2, 6, lmax)) for k in ("gen", "target", "error")}
    want = {k: np.zeros((2, 6, lmax)) for k in ("gen", "target", "error", "cross")}
    for w, t_start in enumerate((0, 3)):
        bufs = su.random_case(lay, w, scaled)
        assert run(lay, bufs, t_start, acc) == 0
        ref = su.numpy_reduction(lay, *bufs)
        for k in want:
            want[k][:, t_start:t_start + T] += ref[k]
    return lay, want, acc


@pytest.mark.parametrize("case", su.REDUCTION_CASES, ids=su.case_id)
def test_host_twin_against_numpy(case):
    import sdy_amd  # noqa: F401

    lay, want, acc = _two_windows(case, lambda lay, bufs, t0, acc: su.host_accumulate(lay, *bufs, t0, acc))
    T, bound = lay.T, su.reduction_bound(lay)
    for k in ("gen", "target", "error"):
        assert not np.isnan(acc[k]).any(), f"{k}: a padding field or an entry with m > l was read"
        err = np.abs(acc[k] - want[k])
        print(f"{k}: worst |err| / bound = {(err / (bound[k] * want[k]).clip(1e-300)).max():.3f}")
        assert (err <= bound[k] * want[k]).all(), k
        untouched = [t for t in range(6) if not (0 <= t < T or 3 <= t < 3 + T)]
        assert (acc[k][:, untouched] == 0.0).all(), k
    # gen + target - error = 2 cross, within the same relative bound of gen + target
    lhs = acc["gen"] + acc["target"] - acc["error"]
    assert (np.abs(lhs - 2.0 * want["cross"]) <= bound["gen"] * (acc["gen"] + acc["target"])).all()


def test_without_the_error_accumulator():
    lay = su.Layout(7, 5, 2, 3, 2, 3, 0)
    bufs = su.random_case(lay, 0)
    full = {k: np.zeros((2, 3, 7)) for k in ("gen", "target", "error")}
    part = {k: np.zeros((2, 3, 7)) for k in ("gen", "target", "error")}
    assert su.host_accumulate(lay, *bufs, 0, full) == 0
    assert su.host_accumulate(lay, *bufs, 0, part, with_error=False) == 0
    assert np.array_equal(full["gen"], part["gen"]) and np.array_equal(full["target"], part["target"])
    assert (part["error"] == 0.0).all() and (full["error"] > 0.0).all()


def test_a_row_does_not_depend_on_its_company():
    """A row's P(l) computed alone and inside a larger call: the same bits.  Rows of one element meet in a fixed order: two
    rows give exactly (P_a + P_b) / 2."""
    lmax, mtr = 7, 5
    big = su.Layout(lmax, mtr, 2, 1, 1, 3, 4)                      # six rows, one per accumulator element, padding between
    cg, ct, _, _ = su.random_case(big, 7)
    acc = {k: np.zeros((2, 3, lmax)) for k in ("gen", "target", "error")}
    assert su.host_accumulate(big, cg, ct, None, None, 0, acc) == 0
    one = su.Layout(lmax, mtr, 1, 1, 1, 1, None)
    alone = {}
    for v in range(2):
        for t in range(3):
            g1 = np.ascontiguousarray(cg[..., [big.gen_field(v, 0, 0, t)]])
            t1 = np.ascontiguousarray(ct[..., [big.target_field(v, 0, t)]])
            a1 = {k: np.zeros((1, 1, lmax)) for k in ("gen", "target", "error")}
            assert su.host_accumulate(one, g1, t1, None, None, 0, a1) == 0
            alone[v, t] = (g1, t1, a1)
            for k in a1:
                assert np.array_equal(a1[k][0, 0], acc[k][v, t]), (k, v, t)
    pair = su.Layout(lmax, mtr, 1, 2, 1, 1, None)                  # two members against one target row
    g2 = np.ascontiguousarray(np.concatenate([alone[0, 0][0], alone[1, 2][0]], axis=-1))
    t2 = alone[0, 0][1]
    a2 = {k: np.zeros((1, 1, lmax)) for k in ("gen", "target", "error")}
    assert su.host_accumulate(pair, g2, t2, None, None, 0, a2) == 0
    assert np.array_equal(a2["gen"][0, 0], (alone[0, 0][2]["gen"][0, 0] + alone[1, 2][2]["gen"][0, 0]) / 2.0)
    assert np.array_equal(a2["target"][0, 0], alone[0, 0][2]["target"][0, 0])


def test_error_codes():
    """What the entry points check themselves; the descriptor's fields: tests/test_coef_rows_host.py."""
    import sdy_amd

    lay = su.Layout(7, 5, 2, 3, 2, 3, 0)
    cg, ct, _, _ = su.random_case(lay, 0)
    acc = {k: np.zeros((2, 6, 7)) for k in ("gen", "target", "error")}
    addr = lambda x: x.ctypes.data      # noqa: E731

    def args(**kw):
        a = su.fill_args(lay, addr(cg), addr(ct), None, None, 0, 6, (addr(acc["gen"]), addr(acc["target"]), addr(acc["error"])))
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    host, dev = sdy_amd.lib.sdy_degree_power_host, sdy_amd.lib.sdy_degree_power
    assert host(C.byref(args())) == 0
    before = {k: v.copy() for k, v in acc.items()}
    bad = [dict(gen=None), dict(target=None), dict(gen_power=None), dict(target_power=None)]
    for kw in bad:
        assert host(C.byref(args(**kw))) == su.SDY_ERR_ARG, kw
        assert dev(C.byref(args(**kw)), None) == su.SDY_ERR_ARG, kw            # refused before anything is launched
    assert host(None) == su.SDY_ERR_ARG and dev(None, None) == su.SDY_ERR_ARG
    assert all(np.array_equal(acc[k], before[k]) for k in acc)


def test_struct_layout():
    from sdy_amd import _lib

    assert _lib.SdySpectrumArgs in _lib.ABI_STRUCTS      # compared with the library: tests/test_capi_cpu.py
