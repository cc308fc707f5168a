"""Host side of the transient-eddy covariances (no GPU): sdy_time_covariance_accumulate_host / _maps_host / _stats_host -- the
header the kernels compile (csrc/time_covariance.h) -- against the float64 numpy restatement (the same bits) and against exact
rational arithmetic on the fp32 inputs; what the entry points refuse; what `CovarianceGroups` and `EddyCovarianceAggregator`
refuse before they touch a device; and the reduce over ranks.  Bounds: tests/eddy_utils.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import eddy_utils as eu

SDY_ERR_ARG, SDY_ERR_UNSUPPORTED = -1, -2

GROUPS = {"low": {"u": "ua", "v": "va", "T": "ta", "q": "qa"}, "wind": {"v": "va", "w": "wa"}}


@pytest.fixture(scope="module")
def sdy():
    import sdy_amd

    return sdy_amd


@pytest.fixture(scope="module")
def small():
    """3 members, 2 samples, 6 x 8, a group of four and a group of two that share `va`, 12 counted times."""
    return eu.seeded_groups(3, 2, 6, 8, 12, GROUPS, seed=301)


def test_host_twin_is_the_restatement(sdy, small):
    """State and maps over windows cut as (IC alone, 1, 1, 3, times in flight + 1): the same bits; weighted sums: the bound of
    another summation order."""
    assert sum(eu.SPLIT) == small["S"] + 1
    windows = eu.cut(small, eu.SPLIT)
    host, n = eu.host_state(small, windows)
    want, n_want = eu.restate_state(small, windows)
    assert n == n_want == 12 and list(host) == [2, 4] and eu.same_state(host, want)
    one, n_one = eu.host_state(small, eu.cut(small, [13]))
    assert n_one == 12 and eu.same_state(one, host)
    for K, blk in host.items():
        for i in range(K):
            for j in range(i, K):
                cov, corr = eu.host_maps(blk, 0, i, j, n)
                want_cov, want_corr, _, _ = eu.restate_maps(want[K], 0, i, j, n)
                assert np.array_equal(cov, want_cov) and np.array_equal(corr, want_corr, equal_nan=True), (K, i, j)
                assert np.isfinite(corr).all() and (np.abs(corr) <= 1.0).all()
        raw = eu.host_stats(blk, small["weights"], n, small["M"], small["B"])
        want_raw, scales = eu.restate_stats(want[K], small["weights"], n, small["M"], small["B"])
        eu.check_raw(raw, want_raw, scales, eu.weight_total(small), f"K = {K}: host vs restatement")
    # the numbers mean what they say: numpy's own covariance and correlation of the counted times
    x, y = (eu.rows_of(small["target"][v], small["gen"][v])[:, 1:].astype(np.float64) for v in ("va", "ta"))
    dx, dy = x - x.mean(axis=1, keepdims=True), y - y.mean(axis=1, keepdims=True)
    cov, corr = eu.host_maps(host[4], 0, 1, 2, n)
    assert np.allclose(cov, (dx * dy).mean(axis=1), rtol=0.0, atol=1e-11)
    assert np.allclose(corr, (dx * dy).sum(axis=1) / np.sqrt((dx * dx).sum(axis=1) * (dy * dy).sum(axis=1)), rtol=0.0, atol=1e-11)
    # the shared variable's sums are the same bits in both groups
    assert np.array_equal(host[4]["sums"][0, 1], host[2]["sums"][0, 0])
    assert np.array_equal(host[4]["products"][0, eu.pair_index(4, 1, 1)], host[2]["products"][0, 0])
    # a run that starts later counts its first time too
    late, n_late = eu.host_state(small, eu.cut(small, [5, 3], start=2))
    want_late, n_want = eu.restate_state(small, eu.cut(small, [5, 3], start=2))
    assert n_late == n_want == 8 and eu.same_state(late, want_late)
    assert np.array_equal(late[2]["origins"][0, 1], eu.rows_of(small["target"]["wa"], small["gen"]["wa"])[:, 2])


def test_exact_arithmetic_with_large_means(sdy):
    """K = 3, n = 12, means of 1e5, 280 and 0: the shifted sums hold the exact-arithmetic bound at a handful of points; plain
    float64 sums of x y miss it."""
    case = eu.seeded_groups(2, 1, 4, 4, 12, {"g": {"p": "ps", "T": "ta", "v": "va"}}, seed=302,
                            means={"ps": 1.0e5, "ta": 280.0, "va": 0.0})
    st, n = eu.host_state(case, eu.cut(case, [6, 7]))
    assert n == 12
    blk = st[3]
    cov = {(i, j): eu.host_maps(blk, 0, i, j, n)[0] for i in range(3) for j in range(i, 3)}
    x = [eu.rows_of(case["target"][v], case["gen"][v])[:, 1:] for v in ("ps", "ta", "va")]
    missed = 0
    for row, a, b in ((0, 0, 0), (1, 2, 3), (2, 3, 1), (0, 1, 2), (2, 0, 3)):           # members and the target
        xs = [xk[row, :, a, b] for xk in x]
        exact = eu.check_point_exact(xs, {ij: c[row, a, b] for ij, c in cov.items()}, f"row {row} ({a}, {b})")
        e = eu.exact_point(xs)
        for k in range(3):                                                              # the sums themselves
            eu.within(float(abs(eu.Fraction(float(blk["sums"][0, k, row, a, b])) - e["s"][k])), 0.0,
                      float(13 * eu.Fraction(eu.U) * sum(abs(eu.Fraction(float(v)) - eu.Fraction(float(xs[k][0]))) for v in xs[k])),
                      f"row {row} S_{k}")
        # unshifted: sum x y / n - mean x mean y in float64
        sx = sy = sxy = 0.0
        for u, v in zip(xs[0].astype(np.float64), xs[1].astype(np.float64)):
            sx, sy, sxy = sx + u, sy + v, sxy + u * v
        plain = (sxy - sx * sy / n) / n
        want, bound = exact[(0, 1)]
        print(f"  unshifted ps-T: |diff| {abs(plain - want):.3e}, {abs(plain - want) / bound:.1f} of the bound")
        missed += abs(plain - want) > bound
    assert missed >= 4


def test_perfect_correlation_anticorrelation_and_a_constant(sdy):
    """y = 2 x exactly in fp32: corr == 1.0; y = -2 x: corr == -1.0; a constant variable: variance 0 and NaN correlations, the
    point outside the pairs' masks."""
    case = eu.seeded_groups(2, 2, 4, 6, 9, {"g": {"x": "x", "y": "y", "z": "z", "k": "k"}}, seed=303)
    for d in (case["target"], case["gen"]):
        d["y"][...] = 2.0 * d["x"]
        d["z"][...] = -2.0 * d["x"]
        d["k"][...] = 3.25
    st, n = eu.host_state(case, eu.cut(case, [4, 6]))
    blk = st[4]
    cov_xx, corr_xx = eu.host_maps(blk, 0, 0, 0, n)
    cov_xy, corr_xy = eu.host_maps(blk, 0, 0, 1, n)
    cov_xz, corr_xz = eu.host_maps(blk, 0, 0, 2, n)
    cov_yz, corr_yz = eu.host_maps(blk, 0, 1, 2, n)
    assert (corr_xx == 1.0).all() and (corr_xy == 1.0).all() and (corr_xz == -1.0).all() and (corr_yz == -1.0).all()
    assert np.array_equal(cov_xy, 2.0 * cov_xx) and np.array_equal(cov_xz, -2.0 * cov_xx) and (cov_xx > 0.0).all()
    cov_kk, corr_kk = eu.host_maps(blk, 0, 3, 3, n)
    cov_xk, corr_xk = eu.host_maps(blk, 0, 0, 3, n)
    assert (cov_kk == 0.0).all() and np.isnan(corr_kk).all() and (cov_xk == 0.0).all() and np.isnan(corr_xk).all()
    raw = eu.host_stats(blk, case["weights"], n, case["M"], case["B"])
    total = eu.weight_total(case)
    assert np.isfinite(raw).all()
    for i, j, frac, rho in ((0, 1, 1.0, 1.0), (0, 2, 1.0, -1.0), (0, 3, 0.0, None), (3, 3, 0.0, None)):
        q = raw[0, eu.pair_index(4, i, j)]
        eu.within(q[5], frac * total, 1e-12 * total, f"mask weight of pair ({i}, {j})")
        if rho is not None:
            eu.within(q[3], rho * total, 1e-12 * total, f"corr_gen sum of pair ({i}, {j})")
            eu.within(q[4], rho * total, 1e-12 * total, f"corr_target sum of pair ({i}, {j})")
        else:
            assert q[3] == q[4] == q[5] == 0.0
    logs = eu.logs_from_raw({"g": raw[0]}, case["groups"], total)
    assert np.isnan(logs["corr_gen/g/x_k"]) and logs["corr_defined_fraction/g/x_k"] == 0.0 and logs["time_variance_gen/g/k"] == 0.0
    # one counted time: every sum is 0, every covariance 0, every correlation NaN
    st1, n1 = eu.host_state(case, eu.cut(case, [2]))
    assert n1 == 1 and not st1[4]["sums"].any() and not st1[4]["products"].any()
    cov1, corr1 = eu.host_maps(st1[4], 0, 0, 1, n1)
    assert not cov1.any() and np.isnan(corr1).all()


def test_nan_stays_in_its_variable(sdy, small):
    """A NaN in one variable at one point and trajectory: NaN exactly that variable's sums and the products that involve it, in
    every group that has the variable; every other bit is the clean run's."""
    bad = dict(small, gen={k: v.copy() for k, v in small["gen"].items()})
    bad["gen"]["va"][2, 1, 5, 3, 4] = np.nan
    clean, _ = eu.host_state(small, eu.cut(small, [6, 7]))
    dirty, _ = eu.host_state(bad, eu.cut(bad, [6, 7]))
    row = 2 * small["B"] + 1
    for K, k_bad in ((4, 1), (2, 0)):
        hit_s = np.zeros(clean[K]["sums"].shape, bool)
        hit_s[0, k_bad, row, 3, 4] = True
        hit_p = np.zeros(clean[K]["products"].shape, bool)
        for i in range(K):
            for j in range(i, K):
                if k_bad in (i, j):
                    hit_p[0, eu.pair_index(K, i, j), row, 3, 4] = True
        assert hit_p.sum() == K
        for key, hit in (("sums", hit_s), ("products", hit_p)):
            assert np.isnan(dirty[K][key][hit]).all() and np.array_equal(dirty[K][key][~hit], clean[K][key][~hit])
        assert np.array_equal(dirty[K]["origins"], clean[K]["origins"])                # (the origins are another time's values)
    cov, corr = eu.host_maps(dirty[4], 0, 0, 2, 12)                                    # a pair without the variable
    assert np.isfinite(cov).all() and np.isfinite(corr).all()
    cov, corr = eu.host_maps(dirty[4], 0, 1, 2, 12)
    assert np.isnan(cov).sum() == np.isnan(corr).sum() == 1 and np.isnan(cov[row, 3, 4])
    raw = eu.host_stats(dirty[2], small["weights"], 12, small["M"], small["B"])
    assert np.isnan(raw[0, 0, 0]) and np.isfinite(raw[0, 2]).all()                     # the NaN reaches its own pairs' means only


def test_structures_stay_out_of_the_abi_list(sdy):
    from sdy_amd import _lib

    for t in (_lib.SdyTimeCovarianceArgs, _lib.SdyTimeCovarianceMapsArgs, _lib.SdyTimeCovarianceStatsArgs):
        assert t not in _lib.ABI_STRUCTS and t().struct_size == C.sizeof(t)
    assert len(_lib.ABI_STRUCTS) == 25 and _lib.ABI_STRUCTS[-1] is _lib.SdyRankHistArgs
    assert _lib.SDY_TC_SLOTS == eu.SLOTS and _lib.SDY_TC_MAX_K == 4 and _lib.SDY_TC_MAX_GROUPS == 32
    assert {"sdy_time_covariance_accumulate", "sdy_time_covariance_accumulate_host", "sdy_time_covariance_maps",
            "sdy_time_covariance_maps_host", "sdy_time_covariance_stats", "sdy_time_covariance_stats_host",
            "sdy_time_covariance_workspace_bytes"} <= set(_lib.SIGNATURES)


# ---- refusals of the entry points ---------------------------------------------------------------------------------------------
def _small_call(first=1):
    case = eu.seeded_groups(3, 2, 4, 6, 2, {"g": {"a": "a", "b": "b", "c": "c"}, "h": {"c": "c", "a": "a", "d": "d"}}, seed=3)
    st = eu.empty_state(case, fill=7.0)
    _, target, gen = eu.cut(case, [3])[0]
    a, keep = eu.accumulate_args(case, 3, ["g", "h"], target, gen, 1, first, st[3])
    return a, keep, st[3]


def _set(a, field, value):
    for f, v in zip(field, value) if isinstance(field, tuple) else ((field, value),):
        if f in ("gen0", "target0"):
            getattr(a, f[:-1])[0] = None
        elif f.startswith("members"):
            a.members[int(f[7])][int(f[8])] = v
        else:
            setattr(a, f, getattr(a, f) + int(v[1:]) if isinstance(v, str) else v)


@pytest.mark.parametrize("field,value,code", [
    ("struct_size", 0, SDY_ERR_ARG), ("struct_size", "+8", SDY_ERR_ARG),
    ("nvars", 0, SDY_ERR_ARG), ("nvars", 97, SDY_ERR_ARG), ("n0", 0, SDY_ERR_ARG), ("n1", -1, SDY_ERR_ARG),
    ("T", 0, SDY_ERR_ARG), ("HW", 0, SDY_ERR_ARG), ("gs0", -1, SDY_ERR_ARG), ("gs1", -4, SDY_ERR_ARG), ("ts1", -1, SDY_ERR_ARG),
    ("gen0", None, SDY_ERR_ARG), ("target0", None, SDY_ERR_ARG),
    ("K", 1, SDY_ERR_ARG), ("K", 5, SDY_ERR_ARG), ("n_groups", 0, SDY_ERR_ARG), ("n_groups", 33, SDY_ERR_ARG),
    ("members00", -1, SDY_ERR_ARG), ("members12", 4, SDY_ERR_ARG),                # outside 0..nvars-1
    ("members11", 2, SDY_ERR_ARG),                                                # group 1 = (2, 2, 3): a variable twice
    ("nvars", 3, SDY_ERR_ARG),                                                    # group 1's variable 3 is no longer in the window
    ("t0", -1, SDY_ERR_ARG), ("t0", 3, SDY_ERR_ARG),                              # t0 >= T
    ("sums", None, SDY_ERR_ARG), ("products", None, SDY_ERR_ARG), ("origins", None, SDY_ERR_ARG),
    ("sums", "+4", SDY_ERR_ARG), ("products", "+4", SDY_ERR_ARG), ("origins", "+2", SDY_ERR_ARG),
    (("T", "HW"), (2, (1 << 29) + 1), SDY_ERR_UNSUPPORTED),            # T * HW > 2^30
    (("n0", "n1"), (1 << 16, 1 << 15), SDY_ERR_UNSUPPORTED),           # n0 * n1 >= 2^31
    (("n0", "n1", "T", "HW", "t0"), (1 << 20, 1 << 10, 1, 1 << 20, 0), SDY_ERR_UNSUPPORTED),   # state index reaches 2^50
])
def test_accumulate_entry_point_refuses(sdy, field, value, code):
    for first in (1, 0):
        a, keep, blk = _small_call(first)
        assert [list(a.members[g])[:3] for g in range(2)] == [[0, 1, 2], [2, 0, 3]]
        _set(a, field, value)
        # both entry points check before anything else: the device one is refused without a device
        assert sdy.lib.sdy_time_covariance_accumulate_host(C.byref(a)) == code
        assert sdy.lib.sdy_time_covariance_accumulate(C.byref(a), None) == code
        assert all((blk[k] == 7.0).all() for k in ("sums", "products", "origins"))
    assert sdy.lib.sdy_time_covariance_accumulate_host(None) == SDY_ERR_ARG
    assert sdy.lib.sdy_time_covariance_accumulate(None, None) == SDY_ERR_ARG


def test_accumulate_host_accepts_the_unmodified_call(sdy):
    a, keep, blk = _small_call()
    assert sdy.lib.sdy_time_covariance_accumulate_host(C.byref(a)) == 0 and not (blk["sums"] == 7.0).any()


def _small_block(K=3, G=2, rows=8, H=4, W=6):
    return dict(sums=np.zeros((G, K, rows, H, W)), products=np.zeros((G, eu.n_pairs(K), rows, H, W)))


@pytest.mark.parametrize("field,value,code", [
    ("struct_size", 0, SDY_ERR_ARG), ("struct_size", "+8", SDY_ERR_ARG),
    ("K", 1, SDY_ERR_ARG), ("K", 5, SDY_ERR_ARG), ("i", -1, SDY_ERR_ARG), ("j", 3, SDY_ERR_ARG), (("i", "j"), (2, 1), SDY_ERR_ARG),
    ("n_elems", 0, SDY_ERR_ARG), ("sums", None, SDY_ERR_ARG), ("products", None, SDY_ERR_ARG), ("cov", None, SDY_ERR_ARG),
    ("corr", None, SDY_ERR_ARG), ("sums", "+4", SDY_ERR_ARG), ("products", "+4", SDY_ERR_ARG), ("cov", "+4", SDY_ERR_ARG),
    ("corr", "+4", SDY_ERR_ARG),
    ("n_times", 0.0, SDY_ERR_ARG), ("n_times", float("nan"), SDY_ERR_ARG), ("n_times", float("inf"), SDY_ERR_ARG),
    ("n_elems", 1 << 48, SDY_ERR_UNSUPPORTED),
])
def test_maps_entry_point_refuses(sdy, field, value, code):
    blk = _small_block()
    cov, corr = np.full(blk["sums"].shape[2:], 7.0), np.full(blk["sums"].shape[2:], 7.0)
    a = eu.maps_args(blk, 1, 0, 2, 3, cov, corr)
    _set(a, field, value)
    assert sdy.lib.sdy_time_covariance_maps_host(C.byref(a)) == code
    assert sdy.lib.sdy_time_covariance_maps(C.byref(a), None) == code
    assert (cov == 7.0).all() and (corr == 7.0).all()
    assert sdy.lib.sdy_time_covariance_maps_host(None) == SDY_ERR_ARG and sdy.lib.sdy_time_covariance_maps(None, None) == SDY_ERR_ARG


def _small_stats_call():
    blk = _small_block()                                 # rows = (3 + 1) * 2
    out = np.full((2, 6, eu.SLOTS), 7.0)
    a, keep = eu.stats_args(blk, np.ones((4, 6), np.float32), 3, 3, 2, out)
    return a, keep + [blk], out


@pytest.mark.parametrize("field,value,code", [
    ("struct_size", 0, SDY_ERR_ARG), ("struct_size", "+8", SDY_ERR_ARG),
    ("K", 1, SDY_ERR_ARG), ("K", 5, SDY_ERR_ARG), ("n_groups", 0, SDY_ERR_ARG), ("n_groups", 33, SDY_ERR_ARG),
    ("M", 0, SDY_ERR_ARG), ("n1", 0, SDY_ERR_ARG), ("HW", -2, SDY_ERR_ARG),
    ("sums", None, SDY_ERR_ARG), ("products", None, SDY_ERR_ARG), ("weights", None, SDY_ERR_ARG), ("out", None, SDY_ERR_ARG),
    ("n_times", 0.0, SDY_ERR_ARG), ("n_times", float("nan"), SDY_ERR_ARG),
    ("sums", "+4", SDY_ERR_ARG), ("products", "+4", SDY_ERR_ARG), ("out", "+4", SDY_ERR_ARG), ("weights", "+2", SDY_ERR_ARG),
    (("n1", "HW"), (1 << 10, (1 << 20) + 1), SDY_ERR_UNSUPPORTED),
    (("n_groups", "M", "n1", "HW"), (32, 1 << 16, 1 << 10, 1 << 20), SDY_ERR_UNSUPPORTED),   # the state index reaches 2^50
])
def test_stats_entry_point_refuses(sdy, field, value, code):
    a, keep, out = _small_stats_call()
    _set(a, field, value)
    assert sdy.lib.sdy_time_covariance_stats_host(C.byref(a)) == code
    ws = np.zeros(4096)
    a.ws, a.ws_bytes = ws.ctypes.data_as(C.c_void_p).value, ws.nbytes
    assert sdy.lib.sdy_time_covariance_stats(C.byref(a), None) == code
    assert (out == 7.0).all()
    assert sdy.lib.sdy_time_covariance_stats_host(None) == SDY_ERR_ARG and sdy.lib.sdy_time_covariance_stats(None, None) == SDY_ERR_ARG


def test_stats_device_entry_point_needs_its_workspace(sdy):
    a, keep, out = _small_stats_call()
    need = sdy.lib.sdy_time_covariance_workspace_bytes(3, 2, 2, 24)
    assert need == 2 * 1 * 6 * eu.SLOTS * 8                # one chunk of 256 points per group, six pairs of six doubles
    assert sdy.lib.sdy_time_covariance_workspace_bytes(4, 2, 3, 256) == 2 * 3 * 10 * eu.SLOTS * 8
    assert sdy.lib.sdy_time_covariance_workspace_bytes(1, 2, 2, 24) == 0 == sdy.lib.sdy_time_covariance_workspace_bytes(3, 0, 2, 24)
    assert sdy.lib.sdy_time_covariance_stats(C.byref(a), None) == SDY_ERR_ARG             # ws NULL
    ws = np.zeros(need // 8)
    a.ws, a.ws_bytes = ws.ctypes.data_as(C.c_void_p).value, need - 8
    assert sdy.lib.sdy_time_covariance_stats(C.byref(a), None) == SDY_ERR_ARG             # ws too small
    spare = np.zeros(need // 8 + 1)
    a.ws, a.ws_bytes = spare.ctypes.data_as(C.c_void_p).value + 4, need
    assert sdy.lib.sdy_time_covariance_stats(C.byref(a), None) == SDY_ERR_ARG             # ws off an 8-byte boundary
    assert (out == 7.0).all()
    assert sdy.lib.sdy_time_covariance_stats_host(C.byref(a)) == 0 and not (out == 7.0).any()   # the twin needs none


# ---- the Python classes, as far as they go without a device ----------------------------------------------------------------
HEADLINE = [f"{stem}_{k}" for k in range(8) for stem in ("air_temperature", "specific_total_water", "eastward_wind", "northward_wind")]


def test_standard_groups_of_the_headline_variables(sdy):
    groups = sdy.CovarianceGroups.standard(["PRESsfc", "surface_temperature"] + HEADLINE)
    assert groups.labels == [f"level_{k}" for k in range(8)] and len(groups) == 8
    for k in range(8):
        assert list(groups.variables(f"level_{k}").items()) == [("u", f"eastward_wind_{k}"), ("v", f"northward_wind_{k}"),
                                                                ("T", f"air_temperature_{k}"), ("q", f"specific_total_water_{k}")]
    part = sdy.CovarianceGroups.standard(["eastward_wind_10", "northward_wind_10", "eastward_wind_2", "northward_wind_2",
                                          "air_temperature_2", "eastward_wind_3", "air_temperature_3", "specific_total_water_10"])
    assert dict(part) == {"level_2": {"u": "eastward_wind_2", "v": "northward_wind_2", "T": "air_temperature_2"},
                          "level_10": {"u": "eastward_wind_10", "v": "northward_wind_10", "q": "specific_total_water_10"}}
    assert len(sdy.CovarianceGroups.standard(["PRESsfc"])) == 0


def test_groups_refuse(sdy):
    g = sdy.CovarianceGroups().add("a", {"u": "x", "v": "y"})
    with pytest.raises(ValueError, match="twice"):
        g.add("a", {"u": "x", "v": "z"})                                # a label twice
    with pytest.raises(ValueError, match="twice"):
        g.add("b", [("u", "x"), ("u", "y")])                            # a short twice
    with pytest.raises(ValueError, match="twice"):
        g.add("b", {"u": "x", "v": "x"})                                # a variable twice
    with pytest.raises(ValueError, match="2 to 4"):
        g.add("b", {"u": "x"})
    with pytest.raises(ValueError, match="2 to 4"):
        g.add("b", {s: s for s in "abcde"})
    with pytest.raises(ValueError, match="short name"):
        g.add("b", {"u_v": "x", "w": "y"})
    assert g.labels == ["a"]
    with pytest.raises(ValueError, match="at least one group"):
        sdy.EddyCovarianceAggregator(sdy.CovarianceGroups(), torch.ones(4, 6))
    with pytest.raises(ValueError, match="target must be"):
        sdy.EddyCovarianceAggregator(g, torch.ones(4, 6), target="raw")


def _window(M=3, B=2, T=3, H=4, W=6, names=("x", "y", "z")):
    g = torch.Generator().manual_seed(0)
    target = {k: torch.randn(B, T, H, W, generator=g) for k in names}
    gen = {k: torch.randn(M, B, T, H, W, generator=g) for k in names}
    return target, gen


def _record(agg, target, gen, **kw):
    agg.record_batch(loss=0.0, target_data=target, gen_data=gen, target_data_norm=target, gen_data_norm=gen, **kw)


def _groups(sdy):
    return sdy.CovarianceGroups().add("a", {"u": "x", "v": "y", "T": "z"}).add("b", {"v": "y", "T": "z"})


def test_class_refuses_before_it_touches_a_device(sdy):
    agg = sdy.EddyCovarianceAggregator(_groups(sdy), torch.ones(4, 6))
    before = {k: v for k, v in vars(agg).items()}
    with pytest.raises(RuntimeError, match="GPU only"):
        _record(agg, *_window())
    assert {k: v for k, v in vars(agg).items()} == before and agg._names is None and agg.n_times == 0 and agg._next_start is None
    with pytest.raises(ValueError, match="'z' of a group is missing"):
        _record(agg, *_window(names=("x", "y")))
    target, gen = _window()
    with pytest.raises(ValueError, match="group 'a' differ in their grid"):
        _record(agg, dict(target, x=target["x"][..., :5]), dict(gen, x=gen["x"][..., :5]))
    with pytest.raises(ValueError, match="negative"):
        _record(agg, target, gen, i_time_start=-1)
    flat = {k: v.reshape(-1, *v.shape[2:])[:5] for k, v in gen.items()}       # 5 rows of 3 members x 2 samples
    with pytest.raises(ValueError, match="EddyCovarianceAggregator needs member-stacked"):
        _record(agg, target, flat)
    with pytest.raises(ValueError, match="member-stacked"):
        _record(agg, target, gen, sample_weights=[0.5, 0.5])
    for call in (lambda: agg.get_logs("x"), lambda: agg.get_pair_data("a", "u", "v"), lambda: agg.get_means("a"), agg.weighted_sums):
        with pytest.raises(ValueError, match="No data recorded"):
            call()
    # max_bytes is compared before anything is allocated: (K + NP) doubles and K floats per trajectory and point
    need = ((3 + 6) * 8 + 3 * 4 + (2 + 3) * 8 + 2 * 4) * (3 + 1) * 2 * 4 * 6
    assert agg.state_bytes(3, 2, 4, 6) == need
    tight = sdy.EddyCovarianceAggregator(_groups(sdy), torch.ones(4, 6), max_bytes=need - 1)
    with pytest.raises(ValueError, match=f"need {need} bytes"):
        _record(tight, target, gen)
    with pytest.raises(RuntimeError, match="GPU only"):
        _record(sdy.EddyCovarianceAggregator(_groups(sdy), torch.ones(4, 6), max_bytes=need), target, gen)
    with pytest.raises(RuntimeError, match="GPU only"):
        sdy.eddies.time_covariance(torch.zeros(3, 4, 6), torch.zeros(3, 4, 6))
    with pytest.raises(ValueError, match="one shape"):
        sdy.eddies.time_covariance(torch.zeros(3, 4, 6), torch.zeros(3, 4, 5))


def test_inference_aggregator_option_is_off_by_default(sdy):
    w = torch.ones(4, 6)
    off = sdy.metrics.InferenceAggregator(w, n_timesteps=3, n_ensemble_members=2)
    assert "eddy_covariance" not in off._aggregators
    with pytest.raises(KeyError):
        off.get_eddy_covariance_data("a", "u", "v")
    agg = sdy.metrics.InferenceAggregator(w, n_timesteps=3, n_ensemble_members=2, eddy_covariances=_groups(sdy))
    assert isinstance(agg._aggregators["eddy_covariance"], sdy.EddyCovarianceAggregator)
    assert list(agg._aggregators)[-1] == "eddy_covariance" and list(agg._aggregators)[:-1] == list(off._aggregators)


class _Share:
    """One rank of two: `reduce_sum` adds what the other rank hands to its own (the fake of a process group)."""

    def __init__(self):
        self.other, self.sent, self.calls = None, None, 0

    def reduce_sum(self, tensor):
        self.calls += 1
        self.sent = tensor.clone()
        return tensor + self.other.sent if self.other.sent is not None else tensor


def _host_rank(sdy, case, dist):
    """An EddyCovarianceAggregator whose weighted sums come from the _host twins on this rank's share: `get_logs` itself -- the
    packing, the one reduce, the divisions -- runs as it is."""
    st, n = eu.host_state(case, eu.cut(case, [7, 6]))
    raw = eu.per_group(case, st, {K: eu.host_stats(blk, case["weights"], n, case["M"], case["B"]) for K, blk in st.items()})

    class OnHost(sdy.EddyCovarianceAggregator):
        def weighted_sums(self):
            self._check_recorded()
            return {label: torch.from_numpy(raw[label]) for label in case["groups"]}

    groups = sdy.CovarianceGroups()
    for label, g in case["groups"].items():
        groups.add(label, g)
    agg = OnHost(groups, torch.from_numpy(case["weights"]), dist=dist)
    agg._names, agg._job_fixed, agg._n_times = list(case["names"]), (case["M"], case["B"], case["H"], case["W"]), n
    agg._blocks[0].sums = torch.zeros(1, dtype=torch.float64)
    return agg


def test_two_ranks_give_the_logs_of_one(sdy):
    """Two shares of whole initial conditions (2 + 1 samples): raw sums and the total weight are added in ONE reduce before any
    root or division, and the logs are those of the unsharded run within the bound of the weighted sums."""
    whole = eu.seeded_groups(3, 3, 6, 8, 12, GROUPS, seed=355)
    whole["gen"]["wa"][1, 2, :, 0, 0] = 1.5                               # the mask differs between the shares
    share = lambda lo, hi: dict(whole, B=hi - lo, target={k: v[lo:hi] for k, v in whole["target"].items()},     # noqa: E731
                                gen={k: v[:, lo:hi] for k, v in whole["gen"].items()})
    d0, d1 = _Share(), _Share()
    d0.other, d1.other = d1, d0
    r0, r1 = _host_rank(sdy, share(0, 2), d0), _host_rank(sdy, share(2, 3), d1)
    r1.get_logs("")                                                     # (rank 1 reaches the reduce first and posts its share)
    logs = r0.get_logs("")
    assert d0.calls == d1.calls == 1
    st, n = eu.restate_state(whole, eu.cut(whole, [7, 6]))
    stats = {K: eu.restate_stats(blk, whole["weights"], n, 3, 3) for K, blk in st.items()}
    want_raw = eu.per_group(whole, st, {K: v[0] for K, v in stats.items()})
    scales = eu.per_group(whole, st, {K: v[1] for K, v in stats.items()})
    want = eu.logs_from_raw(want_raw, whole["groups"], eu.weight_total(whole))
    assert want["corr_defined_fraction/wind/v_w"] < 1.0 == want["corr_defined_fraction/low/u_v"]
    eu.check_logs(logs, want, whole["groups"], scales, "two ranks vs one")
    assert list(r0.get_logs("val")) == [f"val/{k}" for k in want]
    assert "eke_gen/low" in want and "eke_gen/wind" not in want
    # a rank with fewer than two counted times raises before it reaches the collective
    r1._n_times, calls = 1, d1.calls
    with pytest.raises(ValueError, match="No data recorded"):
        r1.get_logs("")
    assert d1.calls == calls
