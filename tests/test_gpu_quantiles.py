"""Time quantiles on the device: sdy_time_quantile_append / sdy_time_quantile_select against their host twins bit for bit,
`TimeQuantileAggregator` against the numpy restatement under window cuts and orders, the production grid, the loop closed with
the threshold events, and the other entry points.  Data and comparisons: tests/quantile_utils.py.  Every test is a handful of
launches."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import quantile_utils as qu

pytestmark = pytest.mark.gpu

RUN = 37                                   # times of the run of the aggregator tests: the initial condition and 36 counted
CUTS = ((37,), (1, 36), (5, 7, 25))
NAMES = ("a", "b")


def _contiguous(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _transposed(x):
    """(members, samples, ...) as the window driver hands it over: a transposed view of a sample-major buffer."""
    buf = _contiguous(x).transpose(0, 1).contiguous()
    view = buf.transpose(0, 1)
    assert not view.is_contiguous() or min(x.shape[:2]) == 1
    return view


def _device_series(gen, target, layout=_contiguous, store_gen=1):
    """One window, every time counted, appended on the device -> (n_traj, T, H*W) int32 device tensor."""
    import sdy_amd
    from sdy_amd import _lib
    from sdy_amd.windows import fill_window, window_layouts

    M, B, T, H, W = gen.shape
    series = torch.full((M * B + B if store_gen else B, T, H * W), -1, dtype=torch.int32, device="cuda")
    lay = window_layouts({"x": _contiguous(target)}, {"x": layout(gen)})
    a = _lib.SdyTimeQuantileAppendArgs()
    fill_window(a.win, lay, 0, 1)
    a.H, a.W, a.t0, a.slot0, a.capacity, a.store_gen, a.series = H, W, 0, 0, T, store_gen, series.data_ptr()
    sdy_amd._lib.check(sdy_amd.lib.sdy_time_quantile_append(C.byref(a), sdy_amd._lib.current_stream()))
    return series


def _device_select(series, H, W, group, qs, method):
    from sdy_amd.quantiles import _select

    out, valid = _select(series.data_ptr(), series.device, series.shape[0], series.shape[1], series.shape[1], H, W, *group, qs,
                         qu.METHOD_CODE[method])
    return out.cpu().numpy(), valid.cpu().numpy()


def _keys(series):
    return series.cpu().numpy().view(np.uint32)


# ---- device against host twin ------------------------------------------------------------------------------------------------
def test_smallest_case_first():
    """One member, one counted time, the scalar path: the first launches of the file."""
    gen, target = qu.make_data(1, qu.SAMPLES, 1, 5, 6)
    series = _device_series(gen, target)
    assert np.array_equal(_keys(series), qu.host_series(gen, target))
    out, valid = _device_select(series, 5, 6, qu.groupings(1, qu.SAMPLES)["target"], (0.5,), "linear")
    want, n = qu.host_select(_keys(series), 5, 6, qu.groupings(1, qu.SAMPLES)["target"], (0.5,), "linear")
    assert qu.same_bits(out, want) and np.array_equal(valid, n)


@pytest.mark.parametrize("grid", qu.GRIDS)
@pytest.mark.parametrize("M", qu.MEMBERS)
@pytest.mark.parametrize("n", qu.TIMES)
def test_device_equals_host_twin(grid, M, n):
    H, W = grid
    gen, target = qu.make_data(M, qu.SAMPLES, n, H, W)
    twin = qu.host_series(gen, target)
    series = _device_series(gen, target)
    assert np.array_equal(_keys(series), twin)
    assert torch.equal(_device_series(gen, target, _transposed), series)             # the member-stacked transposed view
    assert np.array_equal(_keys(_device_series(gen, target, store_gen=0)), twin[M * qu.SAMPLES:])
    for which, group in qu.groupings(M, qu.SAMPLES).items():
        for method in qu.METHODS:
            out, valid = _device_select(series, H, W, group, qu.QS, method)
            want, count = qu.host_select(twin, H, W, group, qu.QS, method)
            assert qu.same_bits(out, want) and np.array_equal(valid, count), (which, method)
    # 8 quantiles: two launches
    qs = (0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 1.0)
    group = qu.groupings(M, qu.SAMPLES)["gen"]
    assert qu.same_bits(_device_select(series, H, W, group, qs, "linear")[0], qu.host_select(twin, H, W, group, qs, "linear")[0])


def test_four_points_per_lane_at_the_production_grid():
    """Enough (group, point) items that the select takes 16-byte loads, 4 points per lane: 12 members per member at 180 x 360,
    11 slots (more than a batch of loads in flight), against the host twin."""
    gen, target = qu.make_data(12, 1, 11, 180, 360)
    twin = qu.host_series(gen, target)
    series = _device_series(gen, target, _transposed)
    assert np.array_equal(_keys(series), twin)
    group = qu.groupings(12, 1)["gen_members"]
    for qs, method in (((0.0, 0.5, 0.9), "linear"), ((0.25, 0.75, 0.99, 1.0, 0.125), "higher")):
        out, valid = _device_select(series, 180, 360, group, qs, method)
        want, count = qu.host_select(twin, 180, 360, group, qs, method)
        assert qu.same_bits(out, want) and np.array_equal(valid, count), method


# ---- the aggregator against the restatement ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run():
    """{name: (gen (3, 2, 37, 5, 8), target (2, 37, 5, 8))}: time 0 is the initial condition."""
    return {k: qu.make_data(3, 2, RUN, 5, 8, seed=i) for i, k in enumerate(NAMES)}


def _windows(run, cuts):
    out, at = [], 0
    for T in cuts:
        out.append((at, {k: t[:, at:at + T] for k, (g, t) in run.items()}, {k: g[:, :, at:at + T] for k, (g, t) in run.items()}))
        at += T
    return out


def _feed(agg, windows):
    for start, target, gen in windows:
        agg.record_batch(0.0, {k: _contiguous(v) for k, v in target.items()}, {k: _transposed(v) for k, v in gen.items()},
                         i_time_start=start)
    return agg


def _agg(weights=None, **kw):
    import sdy_amd

    w = torch.ones(5, 8) if weights is None else weights
    return sdy_amd.TimeQuantileAggregator(qu.QS, w.cuda(), n_timesteps=RUN, per_member=True, **kw)


def _want_data(run, times, method="linear", per_member=True):
    """The restatement of `get_data()` over the counted times `times` (indices into the run)."""
    data = {}
    for k, (gen, target) in run.items():
        g, t = gen[:, :, times], target[:, times]
        data[f"gen/{k}"], n = qu.want(g, t, "gen", qu.QS, method)
        data[f"gen_count/{k}"] = n.astype(np.float64)
        if per_member:
            data[f"gen_members/{k}"] = qu.want(g, t, "gen_members", qu.QS, method)[0].reshape(3, 2, len(qu.QS), 5, 8)
        data[f"target/{k}"], n = qu.want(g, t, "target", qu.QS, method)
        data[f"target_count/{k}"] = n.astype(np.float64)
    data["quantiles"] = np.array(qu.QS)
    return data


def _same_data(got, want):
    assert list(got) == list(want)
    for key, v in want.items():
        g = got[key]
        assert g.dtype == torch.float64 and g.is_cuda and tuple(g.shape) == v.shape, key
        assert qu.same_bits(g.cpu().numpy(), v), key


@pytest.fixture(scope="module")
def wanted(run):
    return _want_data(run, list(range(1, RUN)))


@pytest.mark.parametrize("cuts", CUTS)
@pytest.mark.parametrize("reverse", [False, True])
def test_window_cuts_and_orders_give_the_restatement(run, wanted, cuts, reverse):
    windows = _windows(run, cuts)
    agg = _feed(_agg(), windows[::-1] if reverse else windows)
    assert agg.n_times == RUN - 1
    _same_data(agg.get_data(), wanted)


def test_methods_and_a_run_without_gen(run):
    windows = _windows(run, (5, 7, 25))
    for method in ("lower", "higher"):
        _same_data(_feed(_agg(method=method), windows).get_data(), _want_data(run, list(range(1, RUN)), method))
    agg = _feed(_agg_plain(store_gen=False, variables=["b"]), windows)
    want = _want_data({"b": run["b"]}, list(range(1, RUN)), per_member=False)
    _same_data(agg.get_data(), {k: want[k] for k in ("target/b", "target_count/b", "quantiles")})
    assert agg._acc["series"].numel() == 2 * (RUN - 1) * 40


def _agg_plain(**kw):
    import sdy_amd

    return sdy_amd.TimeQuantileAggregator(qu.QS, torch.ones(5, 8).cuda(), n_timesteps=RUN, **kw)


def test_a_partly_recorded_run(run):
    """Slots missing: the restatement over the recorded times only."""
    windows = _windows(run, (5, 7, 25))
    agg = _feed(_agg(), [windows[2], windows[0]])
    assert agg.n_times == 4 + 25
    _same_data(agg.get_data(), _want_data(run, list(range(1, 5)) + list(range(12, RUN))))


def test_refusals_leave_everything_alone(run):
    import sdy_amd

    windows = _windows(run, (5, 7, 25))
    agg = _feed(_agg(), windows[:2])
    before = agg.get_data()
    series, slots = agg._acc["series"].clone(), list(agg._slots)
    start, target, gen = windows[2]
    dev = lambda d: {k: _contiguous(v) for k, v in d.items()}  # noqa: E731
    with pytest.raises(ValueError, match="time 5 is recorded already"):
        agg.record_batch(0.0, dev(windows[1][1]), dev(windows[1][2]), i_time_start=5)
    with pytest.raises(ValueError, match="time 11 is recorded already"):
        agg.record_batch(0.0, dev(target), dev(gen), i_time_start=11)             # overlaps the last recorded time
    with pytest.raises(ValueError, match="times 13..37 outside the aggregator's 37"):
        agg.record_batch(0.0, dev(target), dev(gen), i_time_start=13)
    with pytest.raises(ValueError, match="member count, sample count or grids of a window differ from the first window"):
        agg.record_batch(0.0, dev(target), dev({k: v[:2] for k, v in gen.items()}), i_time_start=12)
    with pytest.raises(ValueError, match="differ from the first window"):
        agg.record_batch(0.0, dev({"a": target["a"]}), dev({"a": gen["a"]}), i_time_start=12)
    flat = {k: v.reshape(-1, *v.shape[2:])[:5] for k, v in gen.items()}
    with pytest.raises(ValueError, match="TimeQuantileAggregator needs member-stacked"):
        agg.record_batch(0.0, dev(target), dev(flat), i_time_start=12)
    with pytest.raises(ValueError, match="member-stacked"):
        agg.record_batch(0.0, dev(target), dev(gen), i_time_start=12, sample_weights=[0.5, 0.5])
    assert torch.equal(agg._acc["series"], series) and agg._slots == slots
    after = agg.get_data()
    assert list(after) == list(before) and all(qu.same_bits(after[k].cpu().numpy(), before[k].cpu().numpy()) for k in before)
    # ... and the run goes on where it was
    _feed(agg, windows[2:])
    _same_data(agg.get_data(), _want_data(run, list(range(1, RUN))))
    # max_bytes too small: refused at the first window, naming the product
    need = 4 * 8 * (RUN - 1) * 40 * 2
    small = _agg(max_bytes=need - 1)
    with pytest.raises(ValueError, match=f"8 trajectories .3 members x 2 samples . 2 targets. x 36 counted times x 5 x 8 grid points "
                                         f"x 2 variables need {need} bytes"):
        _feed(small, windows[:1])
    assert small._names is None and small._acc == {}
    with pytest.raises(ValueError, match="No data recorded."):
        small.get_data()
    _feed(_agg(max_bytes=need), windows[:1])


def test_production_grid():
    """180 x 360: one variable, 2 members, 1 sample, 40 counted times, 4 quantiles, against the restatement bit for bit."""
    import sdy_amd

    gen, target = qu.make_data(2, 1, 41, 180, 360)
    qs = (0.1, 0.5, 0.9, 0.99)
    agg = sdy_amd.TimeQuantileAggregator(qs, torch.ones(180, 360).cuda(), n_timesteps=41)
    agg.record_batch(0.0, {"pr": _contiguous(target[:, :17])}, {"pr": _transposed(gen[:, :, :17])}, i_time_start=0)
    agg.record_batch(0.0, {"pr": _contiguous(target[:, 17:])}, {"pr": _transposed(gen[:, :, 17:])}, i_time_start=17)
    data = agg.get_data()
    for which in ("gen", "target"):
        want, n = qu.want(gen[:, :, 1:], target[:, 1:], which, qs, "linear")
        assert qu.same_bits(data[f"{which}/pr"].cpu().numpy(), want), which
        assert np.array_equal(data[f"{which}_count/pr"].cpu().numpy(), n.astype(np.float64))
    assert np.isnan(want[:, :, 0, 1]).all() and np.isfinite(want[:, :, 100, 200]).all()


# ---- closing the loop with the events ----------------------------------------------------------------------------------------
def test_threshold_map_gives_the_expected_exceedances():
    """Continuous data (no ties, no NaN), n counted times, q = 0.9: the `higher` quantile is the ceil(q (n - 1))-th smallest
    value, so exactly n - 1 - ceil(q (n - 1)) times lie above it, at every grid point."""
    import sdy_amd

    n, q = 24, 0.9
    rng = np.random.default_rng(5)
    x = rng.standard_normal((1, n, 6, 10)).astype(np.float32)
    assert all(len(np.unique(x[0, :, i, j])) == n for i in range(6) for j in range(10))
    agg = sdy_amd.TimeQuantileAggregator((q,), torch.ones(6, 10).cuda(), n_timesteps=n + 1, store_gen=False)
    agg.record_batch(0.0, {"t2m": _contiguous(x)}, {"t2m": _contiguous(x)}, i_time_start=1)
    thr = agg.threshold_map("t2m", q, method="higher")
    assert thr.dtype == torch.float32 and thr.is_cuda and tuple(thr.shape) == (6, 10)
    assert (torch.from_numpy(x[0]).cuda() == thr).sum(dim=0).eq(1).all()               # an input value of every point
    hits = sdy_amd.spells.spell_statistics(_contiguous(x[0]), thr)["hits"]
    assert torch.equal(hits, torch.full_like(hits, n - 1 - math.ceil(q * (n - 1)))) and n - 1 - math.ceil(q * (n - 1)) == 2
    events = sdy_amd.Events().add("t2m", "p90", above=thr)                             # what the map is for
    assert torch.equal(events.of("t2m")[0].map, thr.cpu())
    low = agg.threshold_map("t2m", q, method="lower")
    assert (low < thr).all()
    for bad in (dict(method="linear"), dict(side="gen"), dict(sample=1)):
        with pytest.raises(ValueError):
            agg.threshold_map("t2m", q, **bad)
    with pytest.raises(ValueError, match="no quantiles of 'pr'"):
        agg.threshold_map("pr", q)


# ---- other entry points ------------------------------------------------------------------------------------------------------
def test_one_field_function(run):
    import sdy_amd

    _, target = run["a"]
    x = target[0, 1:]                                                                   # (36, 5, 8)
    agg = _agg_plain(store_gen=False, variables=["a"])
    _feed(agg, _windows(run, (RUN,)))
    got = sdy_amd.quantiles.time_quantiles(_contiguous(x), qu.QS)
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(qu.QS), 5, 8)
    assert torch.equal(got.view(torch.int64), agg.get_data()["target/a"][0].view(torch.int64))
    assert qu.same_bits(got.cpu().numpy(), qu.restate(x, qu.QS, "linear")[0])
    one = sdy_amd.quantiles.time_quantiles(_contiguous(x), 0.5, method="lower")
    assert qu.same_bits(one.cpu().numpy(), qu.restate(x, (0.5,), "lower")[0])


def test_through_inference_aggregator(run, wanted):
    import sdy_amd

    w = sdy_amd.metrics.spherical_area_weights(torch.linspace(-80.0, 80.0, 5), 8).cuda()
    kw = dict(n_timesteps=RUN, n_ensemble_members=3)
    on = sdy_amd.metrics.InferenceAggregator(w, time_quantiles=qu.QS, time_quantile_variables=["b"], **kw)
    off = sdy_amd.metrics.InferenceAggregator(w, **kw)
    finite = {k: (np.nan_to_num(g, nan=0.0, posinf=3.0, neginf=-3.0), np.nan_to_num(t, nan=0.0, posinf=3.0, neginf=-3.0))
              for k, (g, t) in run.items()}
    for start, target, gen in _windows(finite, (5, 7, 25)):
        t, g = {k: _contiguous(v) for k, v in target.items()}, {k: _transposed(v) for k, v in gen.items()}
        for agg in (on, off):
            agg.record_batch(0.0, t, g, t, g, i_time_start=start)
    want = _want_data({"b": finite["b"]}, list(range(1, RUN)), per_member=False)
    _same_data(on.get_time_quantile_data(), want)
    logs_on, logs_off = on.get_logs("inference"), off.get_logs("inference")
    new = [f"inference/time_quantiles/{m}/q{q:g}/b" for q in qu.QS for m in sdy_amd.quantiles.LOG_METRICS]
    assert [k for k in logs_on if k not in logs_off] == new and list(logs_on)[:len(logs_off)] == list(logs_off)
    assert all(isinstance(logs_on[k], float) for k in new)


def test_logs_against_numpy(run, wanted):
    """The logs are the weighted sums of `get_data()`: a float64 numpy evaluation agrees to 1e-12 relative (the sums are a
    handful of torch float64 reductions over 2 x 40 values, in torch's order)."""
    import sdy_amd

    w = sdy_amd.metrics.spherical_area_weights(torch.linspace(-80.0, 80.0, 5), 8).double()
    # (the infinities of the data made finite: a mean over a map with an infinity says nothing; the NaNs stay)
    finite = {k: (np.clip(g, -3.0, 3.0), np.clip(t, -3.0, 3.0)) for k, (g, t) in run.items()}
    agg = _feed(_agg(weights=w), _windows(finite, (5, 7, 25)))
    data = {k: v.cpu().numpy() for k, v in agg.get_data().items()}
    logs = agg.get_logs("tq")
    wn = w.numpy()
    assert list(logs) == [f"tq/{m}/q{q:g}/{k}" for k in NAMES for q in qu.QS for m in sdy_amd.quantiles.LOG_METRICS]
    seen_undefined = False
    for k in NAMES:
        for i, q in enumerate(qu.QS):
            g, t = data[f"gen/{k}"][:, i], data[f"target/{k}"][:, i]                    # (samples, lat, lon)
            both = ~(np.isnan(g) | np.isnan(t))
            ww = np.broadcast_to(wn, g.shape)
            sw = ww[both].sum()
            with np.errstate(invalid="ignore"):
                want = {"quantile_gen": (ww[both] * g[both]).sum() / sw, "quantile_target": (ww[both] * t[both]).sum() / sw,
                        "quantile_bias": ((ww[both] * g[both]).sum() - (ww[both] * t[both]).sum()) / sw,
                        "quantile_rmse": np.sqrt((ww[both] * (g[both] - t[both]) ** 2).sum() / sw),
                        "defined_fraction": sw / ww.sum()}
            seen_undefined |= not both.all()
            assert all(np.isfinite(v) for v in want.values())
            for m, v in want.items():
                # relative to the sums the metric is made of: the bias is a difference of two of them
                scale = max(abs(v), abs(want["quantile_gen"]), abs(want["quantile_target"]))
                assert abs(logs[f"tq/{m}/q{q:g}/{k}"] - v) <= 1e-12 * scale, (m, q, k)
    assert seen_undefined                                                               # the all-NaN point is in the data
