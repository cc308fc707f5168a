"""Host side of the time-variability statistics (no GPU): sdy_time_variability_accumulate_host / _maps_host / _stats_host -- the
header the kernels compile (csrc/variability.h) -- against the float64 numpy restatement (the same bits) and the restatement
against exact rational arithmetic on the fp32 inputs; what the entry points refuse; what `TimeVariabilityAggregator` refuses
before it touches a device; and the reduce over ranks.  Bounds: tests/variability_utils.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import variability_utils as vu

SDY_ERR_ARG, SDY_ERR_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def sdy():
    import sdy_amd

    return sdy_amd


@pytest.fixture(scope="module")
def small():
    """3 members, 2 samples, 6 x 8, two variables, 12 counted times."""
    return vu.seeded_series(3, 2, 6, 8, 12, ("a", "b"), seed=101)


SPLIT = [1, 1, 1, 3, vu.IN_FLIGHT + 1]          # the initial condition alone, then windows of 1, 1, 3 and 7 counted times


def test_host_twin_is_the_restatement(sdy, small):
    """State, maps: the same bits; weighted sums: the bound of another summation order."""
    windows = vu.cut(small, [4, 2, 7])
    host, n = vu.host_state(small, windows)
    want, n_want = vu.restate_state(small, windows)
    assert n == n_want == small["S"] == 12
    assert vu.same_state(host, want)
    variance, lag1 = vu.host_maps(host, n)
    _, want_var, want_lag = vu.restate_maps(want, n)
    assert np.array_equal(variance, want_var) and np.array_equal(lag1, want_lag, equal_nan=True)
    assert np.isfinite(lag1).all() and (np.abs(lag1) <= 1.0).all() and (variance > 0.0).all()
    raw = vu.host_stats(host, small["weights"], n, small["M"], small["B"])
    want_raw, scales = vu.restate_stats(want, small["weights"], n, small["M"], small["B"])
    vu.check_raw(raw, want_raw, scales, vu.weight_total(small), "host vs restatement")
    # the numbers mean what they say: numpy's own variance and lag-1 autocorrelation of the counted times
    x = vu.rows_of(small["target"]["a"], small["gen"]["a"])[:, 1:].astype(np.float64)
    dev = x - x.mean(axis=1, keepdims=True)
    assert np.allclose(variance[0], x.var(axis=1), rtol=1e-12, atol=0.0)
    assert np.allclose(lag1[0], (dev[:, :-1] * dev[:, 1:]).sum(axis=1) / (dev * dev).sum(axis=1), rtol=0.0, atol=1e-11)


def test_state_does_not_depend_on_the_windows(sdy, small):
    """12 counted times as one window, and as an IC-only window followed by windows of 1, 1, 3 and 7 times (a single-time
    window takes its lag product from `last` alone): the same bits."""
    assert sum(SPLIT) == small["S"] + 1
    one, n_one = vu.host_state(small, vu.cut(small, [13]))
    many, n_many = vu.host_state(small, vu.cut(small, SPLIT))
    assert n_one == n_many == 12 and vu.same_state(one, many)
    # a run that starts later counts its first time too
    late, n_late = vu.host_state(small, vu.cut(small, [5, 3], start=2))
    want, n_want = vu.restate_state(small, vu.cut(small, [5, 3], start=2))
    assert n_late == n_want == 8 and vu.same_state(late, want)
    assert np.array_equal(late["pair"][0, ..., 0], vu.rows_of(small["target"]["a"], small["gen"]["a"])[:, 2])


def test_restatement_against_exact_arithmetic(small):
    windows = vu.cut(small, [13])
    st, n = vu.restate_state(small, windows)
    _, variance, _ = vu.restate_maps(st, n)
    x = vu.rows_of(small["target"]["b"], small["gen"]["b"])
    for row, i, j in ((0, 0, 0), (3, 2, 5), (5, 5, 7), (7, 3, 1)):            # members and targets
        vu.check_point_exact(x[row, 1:, i, j], st["s1"][1, row, i, j], st["s2"][1, row, i, j], st["p"][1, row, i, j],
                             variance[1, row, i, j], f"small row {row} ({i}, {j})")


def test_long_pressure_like_series_needs_the_shift(sdy):
    """n = 2000 on a 4 x 4 grid, mean 101325, std 50, AR(1) with phi = 0.95: the shifted sums hold the exact-arithmetic bound at
    every point; plain float64 sums of x and x^2 miss the same bound at every point."""
    case = vu.seeded_series(1, 1, 4, 4, 2000, ("ps",), seed=7, mean=101325.0, std=50.0, phi=0.95, bias=5.0, spread=10.0)
    windows = vu.cut(case, [701, 600, 700])
    st, n = vu.restate_state(case, windows)
    host, n_host = vu.host_state(case, windows)
    assert n == n_host == 2000 and vu.same_state(st, host)
    _, variance, lag1 = vu.restate_maps(st, n)
    assert 0.8 < float(lag1.min()) and float(lag1.max()) < 1.0                 # phi = 0.95
    x = vu.rows_of(case["target"]["ps"], case["gen"]["ps"])[:, 1:]
    missed = 0
    for row in range(2):
        for i in range(4):
            for j in range(4):
                xs = x[row, :, i, j]
                exact, bound = vu.check_point_exact(xs, st["s1"][0, row, i, j], st["s2"][0, row, i, j], st["p"][0, row, i, j],
                                                    variance[0, row, i, j], f"long row {row} ({i}, {j})")
                sx = sxx = 0.0
                for v in xs.astype(np.float64):
                    sx, sxx = sx + v, sxx + v * v
                plain = (sxx - sx * sx / n) / n
                print(f"  unshifted: |diff| {abs(plain - exact):.3e}, {abs(plain - exact) / bound:.1f} of the bound")
                missed += abs(plain - exact) > bound
    assert missed == 32


def test_constant_and_nan(sdy, small):
    """A trajectory that is constant at a point: variance exactly 0, lag1 NaN, the point outside the mask; a NaN input stays in
    its own trajectory and point."""
    case = dict(small, gen={k: v.copy() for k, v in small["gen"].items()})
    case["gen"]["a"][0, 0, :, 1, 2] = case["gen"]["a"][0, 0, 0, 1, 2]
    windows = vu.cut(case, [6, 7])
    st, n = vu.host_state(case, windows)
    variance, lag1 = vu.host_maps(st, n)
    assert variance[0, 0, 1, 2] == 0.0 and np.isnan(lag1[0, 0, 1, 2])
    assert np.isnan(lag1).sum() == 1 and (variance > 0.0).sum() == variance.size - 1
    raw = vu.host_stats(st, case["weights"], n, case["M"], case["B"])
    total = vu.weight_total(case)
    assert np.isfinite(raw).all()
    vu.within(raw[0, 5], total - float(case["weights"][1, 2]), 1e-12 * total, "masked weight")
    vu.within(raw[1, 5], total, 1e-12 * total, "full weight")
    logs = vu.logs_from_raw(raw, case["names"], total)
    assert all(np.isfinite(v) for v in logs.values())
    assert logs["lag1_defined_fraction/a"] < 1.0 - 0.5 * float(case["weights"][1, 2]) / total < logs["lag1_defined_fraction/b"]
    # all of a variable's trajectories constant: no NaN in the time_std logs, the lag-1 logs undefined
    flat = vu.seeded_series(2, 1, 4, 6, 5, ("a",), seed=3)
    for d in (flat["target"], flat["gen"]):
        d["a"][...] = 3.25
    st_f, n_f = vu.host_state(flat, vu.cut(flat, [6]))
    raw_f = vu.host_stats(st_f, flat["weights"], n_f, 2, 1)
    logs_f = vu.logs_from_raw(raw_f, ["a"], vu.weight_total(flat))
    assert logs_f["time_std_gen/a"] == logs_f["time_std_target/a"] == logs_f["time_std_rmse/a"] == 0.0
    assert logs_f["lag1_defined_fraction/a"] == 0.0 and np.isnan(logs_f["lag1_gen/a"]) and np.isnan(logs_f["time_std_ratio/a"])
    # NaN
    bad = dict(small, gen={k: v.copy() for k, v in small["gen"].items()})
    bad["gen"]["b"][2, 1, 5, 3, 4] = np.nan
    clean, _ = vu.host_state(small, vu.cut(small, [6, 7]))
    dirty, _ = vu.host_state(bad, vu.cut(bad, [6, 7]))
    row = 2 * small["B"] + 1
    hit = np.zeros(clean["s1"].shape, bool)
    hit[1, row, 3, 4] = True
    for k in ("s1", "s2", "p"):
        assert np.isnan(dirty[k][hit]).all() and np.array_equal(dirty[k][~hit], clean[k][~hit])
    assert np.array_equal(dirty["pair"], clean["pair"])                           # (c, last) are other times' values
    v_bad, l_bad = vu.host_maps(dirty, 12)
    assert np.isnan(v_bad[hit]).all() and np.isnan(l_bad[hit]).all() and np.isfinite(v_bad[~hit]).all() and np.isfinite(l_bad[~hit]).all()


def test_one_counted_time_has_no_lag(sdy, small):
    st, n = vu.host_state(small, vu.cut(small, [2]))
    assert n == 1 and not st["s1"].any() and not st["s2"].any() and not st["p"].any()
    variance, lag1 = vu.host_maps(st, n)
    assert not variance.any() and np.isnan(lag1).all()


def test_struct_sizes(sdy):
    from sdy_amd import _lib

    for t in (_lib.SdyVariabilityArgs, _lib.SdyVariabilityMapsArgs, _lib.SdyVariabilityStatsArgs):
        assert t in _lib.ABI_STRUCTS                                              # tests/test_capi_cpu.py
    assert _lib.SDY_TV_SLOTS == vu.SLOTS == len(vu.LOG_KEYS) - 2


def _small_call(first=1):
    rng = np.random.default_rng(3)
    target = {"a": rng.standard_normal((2, 3, 4, 6)).astype(np.float32)}
    gen = {"a": rng.standard_normal((3, 2, 3, 4, 6)).astype(np.float32)}
    st = vu.empty_state(1, 3, 2, 4, 6, fill=7.0)
    a, keep = vu.accumulate_args(target, gen, ["a"], 1, first, st)
    return a, keep, st


def _set(a, field, value):
    for f, v in zip(field, value) if isinstance(field, tuple) else ((field, value),):
        if f in ("gen0", "target0"):
            getattr(a, f[:-1])[0] = None
        else:
            setattr(a, f, getattr(a, f) + 4 if v == "+4" else v)


@pytest.mark.parametrize("field,value,code", [
    ("nvars", 0, SDY_ERR_ARG), ("nvars", 97, SDY_ERR_ARG), ("n0", 0, SDY_ERR_ARG), ("n1", -1, SDY_ERR_ARG),
    ("T", 0, SDY_ERR_ARG), ("HW", 0, SDY_ERR_ARG), ("gs0", -1, SDY_ERR_ARG), ("gs1", -4, SDY_ERR_ARG), ("ts1", -1, SDY_ERR_ARG),
    ("t0", -1, SDY_ERR_ARG), ("t0", 3, SDY_ERR_ARG),                              # t0 >= T
    ("s1", None, SDY_ERR_ARG), ("s2", None, SDY_ERR_ARG), ("p", None, SDY_ERR_ARG), ("origin_last", None, SDY_ERR_ARG),
    ("gen0", None, SDY_ERR_ARG), ("target0", None, SDY_ERR_ARG),
    ("s1", "+4", SDY_ERR_ARG), ("s2", "+4", SDY_ERR_ARG), ("p", "+4", SDY_ERR_ARG), ("origin_last", "+4", SDY_ERR_ARG),
    (("T", "HW"), (2, (1 << 29) + 1), SDY_ERR_UNSUPPORTED),            # T * HW > 2^30
    (("n0", "n1"), (1 << 16, 1 << 15), SDY_ERR_UNSUPPORTED),           # n0 * n1 >= 2^31
    (("n0", "n1", "T", "HW", "t0"), (1 << 20, 1 << 10, 1, 1 << 20, 0), SDY_ERR_UNSUPPORTED),   # state index reaches 2^50
])
def test_accumulate_entry_point_refuses(sdy, field, value, code):
    for first in (1, 0):
        a, keep, st = _small_call(first)
        _set(a, field, value)
        # both entry points check before anything else: the device one is refused without a device
        assert sdy.lib.sdy_time_variability_accumulate_host(C.byref(a)) == code
        assert sdy.lib.sdy_time_variability_accumulate(C.byref(a), None) == code
        assert all((st[k] == 7.0).all() for k in st)
    assert sdy.lib.sdy_time_variability_accumulate_host(None) == SDY_ERR_ARG
    assert sdy.lib.sdy_time_variability_accumulate(None, None) == SDY_ERR_ARG


@pytest.mark.parametrize("field,value,code", [
    ("n_elems", 0, SDY_ERR_ARG), ("s1", None, SDY_ERR_ARG), ("s2", None, SDY_ERR_ARG), ("p", None, SDY_ERR_ARG),
    ("origin_last", None, SDY_ERR_ARG), ("variance", None, SDY_ERR_ARG), ("lag1", None, SDY_ERR_ARG),
    ("s1", "+4", SDY_ERR_ARG), ("origin_last", "+4", SDY_ERR_ARG), ("variance", "+4", SDY_ERR_ARG), ("lag1", "+4", SDY_ERR_ARG),
    ("n_times", 0.0, SDY_ERR_ARG), ("n_times", float("nan"), SDY_ERR_ARG), ("n_times", float("inf"), SDY_ERR_ARG),
    ("n_elems", 1 << 40, SDY_ERR_UNSUPPORTED),
])
def test_maps_entry_point_refuses(sdy, field, value, code):
    st = vu.empty_state(1, 3, 2, 4, 6)
    variance, lag1 = np.full(st["s1"].shape, 7.0), np.full(st["s1"].shape, 7.0)
    a = vu.maps_args(st, 3, variance, lag1)
    _set(a, field, value)
    assert sdy.lib.sdy_time_variability_maps_host(C.byref(a)) == code
    assert sdy.lib.sdy_time_variability_maps(C.byref(a), None) == code
    assert (variance == 7.0).all() and (lag1 == 7.0).all()
    assert sdy.lib.sdy_time_variability_maps_host(None) == SDY_ERR_ARG


def _small_stats_call():
    st = vu.empty_state(2, 3, 2, 4, 6)
    out = np.full((2, vu.SLOTS), 7.0)
    a, keep = vu.stats_args(st, np.ones((4, 6), np.float32), 3, 3, 2, out)
    return a, keep + [st], out


@pytest.mark.parametrize("field,value,code", [
    ("nvars", 0, SDY_ERR_ARG), ("M", 0, SDY_ERR_ARG), ("n1", 0, SDY_ERR_ARG), ("HW", -2, SDY_ERR_ARG),
    ("s1", None, SDY_ERR_ARG), ("s2", None, SDY_ERR_ARG), ("p", None, SDY_ERR_ARG), ("origin_last", None, SDY_ERR_ARG),
    ("weights", None, SDY_ERR_ARG), ("out", None, SDY_ERR_ARG),
    ("n_times", 0.0, SDY_ERR_ARG), ("n_times", float("nan"), SDY_ERR_ARG),
    ("s1", "+4", SDY_ERR_ARG), ("origin_last", "+4", SDY_ERR_ARG), ("out", "+4", SDY_ERR_ARG),
    ("nvars", 65536, SDY_ERR_UNSUPPORTED),
    (("n1", "HW"), (1 << 10, (1 << 20) + 1), SDY_ERR_UNSUPPORTED),
    (("nvars", "M", "n1", "HW"), (1 << 14, 64, 1 << 10, 1 << 20), SDY_ERR_UNSUPPORTED),   # nvars (M + 1) n1 HW reaches 2^50
])
def test_stats_entry_point_refuses(sdy, field, value, code):
    a, keep, out = _small_stats_call()
    _set(a, field, value)
    assert sdy.lib.sdy_time_variability_stats_host(C.byref(a)) == code
    assert (out == 7.0).all()
    assert sdy.lib.sdy_time_variability_stats_host(None) == SDY_ERR_ARG


def test_stats_device_entry_point_needs_its_workspace(sdy):
    a, keep, out = _small_stats_call()
    need = sdy.lib.sdy_time_variability_workspace_bytes(2, 2, 24)
    assert need == 2 * 1 * vu.SLOTS * 8                  # one block of 256 points per variable, six doubles
    assert sdy.lib.sdy_time_variability_workspace_bytes(2, 3, 256) == 2 * 3 * vu.SLOTS * 8
    assert sdy.lib.sdy_time_variability_workspace_bytes(0, 2, 24) == 0
    assert sdy.lib.sdy_time_variability_stats(C.byref(a), None) == SDY_ERR_ARG             # ws NULL
    ws = np.zeros(need // 8)
    a.ws, a.ws_bytes = ws.ctypes.data_as(C.c_void_p).value, need - 8
    assert sdy.lib.sdy_time_variability_stats(C.byref(a), None) == SDY_ERR_ARG             # ws too small
    spare = np.zeros(need // 8 + 1)
    a.ws, a.ws_bytes = spare.ctypes.data_as(C.c_void_p).value + 4, need
    assert sdy.lib.sdy_time_variability_stats(C.byref(a), None) == SDY_ERR_ARG             # ws off an 8-byte boundary
    assert (out == 7.0).all()


# ---- the Python class, as far as it goes without a device -----------------------------------------------------------------
def _window(M=3, B=2, T=3, H=4, W=6, names=("a", "b")):
    g = torch.Generator().manual_seed(0)
    target = {k: torch.randn(B, T, H, W, generator=g) for k in names}
    gen = {k: torch.randn(M, B, T, H, W, generator=g) for k in names}
    return target, gen


def _record(agg, target, gen, **kw):
    agg.record_batch(loss=0.0, target_data=target, gen_data=gen, target_data_norm=target, gen_data_norm=gen, **kw)


def test_class_refuses_cpu_tensors_and_changes_nothing(sdy):
    agg = sdy.TimeVariabilityAggregator(torch.ones(4, 6))
    before = dict(vars(agg))
    with pytest.raises(RuntimeError, match="GPU only"):
        _record(agg, *_window())
    assert vars(agg) == before and agg._names is None and agg.n_times == 0
    with pytest.raises(RuntimeError, match="GPU only"):            # no job and no start were fixed: anything gets as far again
        _record(agg, *_window(names=("a", "c"), M=4), i_time_start=9)
    with pytest.raises(ValueError, match="No data recorded"):
        agg.get_logs("x")
    with pytest.raises(ValueError, match="No data recorded"):
        agg.get_data()
    with pytest.raises(ValueError, match="negative"):
        _record(agg, *_window(), i_time_start=-1)
    with pytest.raises(ValueError, match="target must be"):
        sdy.TimeVariabilityAggregator(torch.ones(4, 6), target="raw")


def test_class_refuses_another_job(sdy):
    """What record_batch compares a later window with, on host tensors: the variable set, the member count, the sample count and
    the grid.  (Through the class on a device: tests/test_gpu_variability.py.)"""
    from sdy_amd.windows import check_same_job, window_layouts

    def job(**kw):
        target, gen = _window(**kw)
        return list(gen), [sdy.TimeVariabilityAggregator._job(l) for l in window_layouts(target, gen)]

    words = sdy.TimeVariabilityAggregator._job_words
    first = job()
    assert first[1] == [(3, 2, 4, 6)] * 2
    check_same_job(*job(T=2), *first, words)                       # another number of times is the same job
    for other in (dict(names=("a", "c")), dict(names=("b", "a")), dict(names=("a",)), dict(M=4), dict(B=3), dict(H=5)):
        with pytest.raises(ValueError, match="member count, sample count or grids of a window differ from the first window"):
            check_same_job(*job(**other), *first, words)


def test_class_refuses_state_over_max_bytes(sdy):
    need = 32 * 2 * (2 * 4 * 6) * (3 + 1)            # 32 bytes per trajectory and grid point
    agg = sdy.TimeVariabilityAggregator(torch.ones(4, 6), max_bytes=need - 1)
    with pytest.raises(ValueError, match=f"need {need} bytes"):
        _record(agg, *_window())
    agg = sdy.TimeVariabilityAggregator(torch.ones(4, 6), max_bytes=need)
    with pytest.raises(RuntimeError, match="GPU only"):
        _record(agg, *_window())


def test_class_refuses_ragged_shares(sdy):
    agg = sdy.TimeVariabilityAggregator(torch.ones(4, 6))
    target, gen = _window()
    flat = {k: v.reshape(-1, *v.shape[2:])[:5] for k, v in gen.items()}       # 5 rows of 3 members x 2 samples
    with pytest.raises(ValueError, match="TimeVariabilityAggregator needs member-stacked"):
        _record(agg, target, flat)
    with pytest.raises(ValueError, match="member-stacked"):
        _record(agg, {k: v[:1] for k, v in target.items()}, {k: v[:1] for k, v in flat.items()}, sample_weights=[1 / 3])
    assert agg._names is None and agg._next_start is None


def test_inference_aggregator_option_is_off_by_default(sdy):
    w = torch.ones(4, 6)
    off = sdy.metrics.InferenceAggregator(w, n_timesteps=3, n_ensemble_members=2)
    assert "time_variability" not in off._aggregators
    with pytest.raises(KeyError):
        off.get_time_variability_data()
    agg = sdy.metrics.InferenceAggregator(w, n_timesteps=3, n_ensemble_members=2, time_variability_data=True)
    assert isinstance(agg._aggregators["time_variability"], sdy.TimeVariabilityAggregator)
    assert list(agg._aggregators)[-1] == "time_variability"


class _Share:
    """One rank of two: `reduce_sum` adds what the other rank hands to its own (the fake of a process group)."""

    def __init__(self):
        self.other, self.sent, self.calls = None, None, 0

    def reduce_sum(self, tensor):
        self.calls += 1
        self.sent = tensor.clone()
        return tensor + self.other.sent if self.other.sent is not None else tensor


def _host_rank(sdy, case, dist):
    """A TimeVariabilityAggregator whose weighted sums come from the _host twins on this rank's share: `get_logs` itself --
    the packing, the one reduce, the divisions -- runs as it is."""
    st, n = vu.host_state(case, vu.cut(case, [7, 6]))
    raw = vu.host_stats(st, case["weights"], n, case["M"], case["B"])

    class OnHost(sdy.TimeVariabilityAggregator):
        def weighted_sums(self):
            self._check_recorded()
            return {k: torch.from_numpy(raw[j]) for j, k in enumerate(case["names"])}

    agg = OnHost(torch.from_numpy(case["weights"]), dist=dist)
    agg._names, agg._grids = list(case["names"]), [(case["M"], case["B"], case["H"], case["W"])] * len(case["names"])
    agg._acc, agg._n_times = {"s1": torch.zeros(1, dtype=torch.float64)}, n
    return agg


def test_two_ranks_give_the_logs_of_one(sdy):
    """Two shares of whole initial conditions (2 + 1 samples): raw sums and total weights are added in ONE reduce before any
    root or division, and the logs are those of the unsharded run within the bound of the weighted sums."""
    whole = vu.seeded_series(3, 3, 6, 8, 12, ("a", "b"), seed=55)
    whole["gen"]["a"][1, 2, :, 0, 0] = 1.5                               # the mask differs between the shares
    share = lambda lo, hi: dict(whole, B=hi - lo, target={k: v[lo:hi] for k, v in whole["target"].items()},     # noqa: E731
                                gen={k: v[:, lo:hi] for k, v in whole["gen"].items()})
    d0, d1 = _Share(), _Share()
    d0.other, d1.other = d1, d0
    r0, r1 = _host_rank(sdy, share(0, 2), d0), _host_rank(sdy, share(2, 3), d1)
    r1.get_logs("")                                                     # (rank 1 reaches the reduce first and posts its share)
    logs = r0.get_logs("")
    assert d0.calls == d1.calls == 1
    st, n = vu.restate_state(whole, vu.cut(whole, [7, 6]))
    want_raw, scales = vu.restate_stats(st, whole["weights"], n, 3, 3)
    want = vu.logs_from_raw(want_raw, whole["names"], vu.weight_total(whole))
    assert want["lag1_defined_fraction/a"] < 1.0
    vu.check_logs(logs, want, whole["names"], scales, "two ranks vs one")
    assert list(r0.get_logs("val")) == [f"val/{k}" for k in want]
    # a rank with fewer than two counted times raises before it reaches the collective
    r1._n_times, calls = 1, d1.calls
    with pytest.raises(ValueError, match="No data recorded"):
        r1.get_logs("")
    assert d1.calls == calls
