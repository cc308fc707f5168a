"""Time variance and lag-1 autocorrelation on the device (`sdy_amd.TimeVariabilityAggregator`; kernels of csrc/variability.hip)
against the library's _host twins (state and maps: the same bits; weighted sums: the bound of another summation order) and the
float64 restatement: windowing, layouts, members and batch, the grid stride, degenerate data, refusals, the logs, and the way
through run_inference.  Bounds: tests/variability_utils.py.  Every case is a handful of launches."""
import numpy as np
import pytest
import torch

import variability_utils as vu

pytestmark = pytest.mark.gpu


def _contiguous(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _transposed(x):
    """(members, samples, ...) as the window driver hands it over: a transposed view of a sample-major buffer."""
    buf = _contiguous(x).transpose(0, 1).contiguous()
    view = buf.transpose(0, 1)
    assert not view.is_contiguous() or min(x.shape[:2]) == 1
    return view


def _offset(x):
    """A view that starts one element into a larger buffer: 4 bytes off a 16-byte boundary, so the scalar path."""
    buf = torch.zeros(x.size + 1, device="cuda")
    buf[1:] = _contiguous(x).reshape(-1)
    out = buf[1:].view(x.shape)
    assert out.data_ptr() % 16 == 4
    return out


def _feed(agg, windows, layout=_contiguous, target_layout=_contiguous):
    for start, target, gen in windows:
        agg.record_batch(0.0, {k: target_layout(v) for k, v in target.items()}, {k: layout(v) for k, v in gen.items()},
                         i_time_start=start)
    return agg


def _run(case, windows, layout=_contiguous, target_layout=_contiguous, **kw):
    import sdy_amd

    return _feed(sdy_amd.TimeVariabilityAggregator(torch.from_numpy(case["weights"]).cuda(), **kw), windows, layout, target_layout)


def _state(agg, case):
    n, rows, H, W = len(case["names"]), (case["M"] + 1) * case["B"], case["H"], case["W"]
    st = {k: agg._acc[k].view(n, rows, H, W).cpu().numpy() for k in ("s1", "s2", "p")}
    st["pair"] = agg._acc["pair"].view(torch.float32).view(n, rows, H, W, 2).cpu().numpy()
    return st


def _raw(agg):
    sums = agg.weighted_sums()
    return np.stack([sums[k].cpu().numpy() for k in agg._names])


def _check_against_host(agg, case, windows, what):
    """State and maps: the _host twin's bits; weighted sums: the _host twin's and the restatement's within the bound; the logs
    against the restatement's.  -> the device's logs."""
    host, n = vu.host_state(case, windows)
    assert agg.n_times == n
    got = _state(agg, case)
    assert vu.same_state(got, host), what
    M, B, H, W = case["M"], case["B"], case["H"], case["W"]
    variance, lag1 = vu.host_maps(host, n)
    data = agg.get_data()
    assert list(data) == ["gen_time_std", "gen_lag1", "target_time_std", "target_lag1"]
    for j, k in enumerate(case["names"]):
        g_sd, g_lag, t_sd, t_lag = (data[m][k] for m in data)
        assert all(x.dtype == torch.float64 and x.is_cuda for x in (g_sd, g_lag, t_sd, t_lag))
        assert tuple(g_sd.shape) == tuple(g_lag.shape) == (M, B, H, W) and tuple(t_sd.shape) == tuple(t_lag.shape) == (B, H, W)
        assert np.array_equal(g_lag.cpu().numpy(), lag1[j, :M * B].reshape(M, B, H, W), equal_nan=True), what
        assert np.array_equal(t_lag.cpu().numpy(), lag1[j, M * B:], equal_nan=True), what
        # the roots of the _host twin's variances, to the last place of a square root
        for got_sd, var in ((g_sd, variance[j, :M * B].reshape(M, B, H, W)), (t_sd, variance[j, M * B:])):
            want_sd = np.sqrt(var)
            off = np.abs(got_sd.cpu().numpy() - want_sd)
            print(f"{what} {k}: {int((off > 0).sum())} of {off.size} roots differ from numpy's")
            assert np.array_equal(np.isnan(got_sd.cpu().numpy()), np.isnan(want_sd)) and not (off > 2.0 ** -52 * want_sd).any(), what
    host_raw = vu.host_stats(host, case["weights"], n, M, B)
    want_raw, scales = vu.restate_stats(host, case["weights"], n, M, B)
    total = vu.weight_total(case)
    raw = _raw(agg)
    vu.check_raw(raw, host_raw, scales, total, f"{what}: device vs host")
    vu.check_raw(raw, want_raw, scales, total, f"{what}: device vs restatement")
    logs = agg.get_logs("")
    vu.check_logs(logs, vu.logs_from_raw(want_raw, case["names"], total), case["names"], scales, what)
    return logs


@pytest.fixture(scope="module")
def small():
    """3 members, 2 samples, 18 x 36, two variables, 12 counted times."""
    return vu.seeded_series(3, 2, 18, 36, 12, ("a", "b"), seed=202)


# the windowing case: the initial condition alone, then windows of 1, 1, 3 and kTimesInFlight + 1 = 7 counted times
SPLIT = [1, 1, 1, 3, vu.IN_FLIGHT + 1]


def test_state_does_not_depend_on_the_windows(small):
    assert sum(SPLIT) == small["S"] + 1 == 13
    one = _run(small, vu.cut(small, [13]))
    many = _run(small, vu.cut(small, SPLIT))
    assert one.n_times == many.n_times == 12
    assert vu.same_state(_state(one, small), _state(many, small))
    _check_against_host(many, small, vu.cut(small, SPLIT), "windows of 0, 1, 1, 3, 7")
    assert list(many.get_logs("full")) == [f"full/{k}" for k in many.get_logs("")]


def test_layouts_give_the_same_bits(small):
    """Contiguous, the transposed view of a (samples, members, ...) buffer, and views one element into a larger buffer (scalar
    loads): the order of every sum is fixed, so the state is bit-identical."""
    windows = vu.cut(small, [5, 8])
    ref = _state(_run(small, windows), small)
    for layout, target_layout in ((_transposed, _contiguous), (_offset, _contiguous), (_offset, _offset)):
        assert vu.same_state(_state(_run(small, windows, layout, target_layout), small), ref), layout.__name__
    _check_against_host(_run(small, windows, _transposed), small, windows, "transposed")


def test_a_grid_that_is_no_multiple_of_four():
    case = vu.seeded_series(2, 3, 7, 9, 9, ("a", "b", "c"), seed=203)
    windows = vu.cut(case, [3, 7])
    _check_against_host(_run(case, windows, _transposed), case, windows, "7 x 9")


def test_one_member_from_flat_rows():
    """A 4-D gen is one member."""
    case = vu.seeded_series(1, 2, 16, 32, 9, ("a",), seed=204)
    windows = vu.cut(case, [4, 6])
    flat = [(s, t, {k: v[0] for k, v in g.items()}) for s, t, g in windows]
    agg = _run(case, flat)
    assert tuple(agg.get_data()["gen_lag1"]["a"].shape) == (1, 2, 16, 32)
    _check_against_host(agg, case, windows, "one member")


def test_25_members_and_batch_independence():
    """M = 25 on 16 x 32; sample 0's state from the B = 2 run equals that of a run on sample 0 alone, bit for bit."""
    case = vu.seeded_series(25, 2, 16, 32, 8, ("a",), seed=205)
    windows = vu.cut(case, [3, 6])
    agg = _run(case, windows, _transposed)
    _check_against_host(agg, case, windows, "25 members")
    one = dict(case, B=1, target={k: v[:1] for k, v in case["target"].items()}, gen={k: v[:, :1] for k, v in case["gen"].items()})
    alone = _state(_run(one, vu.cut(one, [3, 6]), _transposed), one)
    both = _state(agg, case)
    rows = [2 * m for m in range(25)] + [50]                    # member m of sample 0, and sample 0's target
    assert all(np.array_equal(both[k][:, rows], alone[k]) for k in both)


def test_grid_stride():
    """3 variables, 5 members, 2 samples, 3 times on 180 x 360: 12 rows x 16200 items of four points = 760 blocks per variable
    against the launch's 1024 / 3 = 341 (kBlocksPerLaunch over the variables): every thread strides.  A run that starts at
    time 5 counts all three times."""
    case = vu.seeded_series(5, 2, 180, 360, 7, ("a", "b", "c"), seed=206, mean=101325.0, std=50.0, phi=0.9)
    windows = vu.cut(case, [3], start=5)
    agg = _run(case, windows, _transposed)
    assert agg.n_times == 3
    _check_against_host(agg, case, windows, "180 x 360")
    assert vu.same_state(_state(_run(case, windows, _offset, _offset), case), _state(agg, case))       # the scalar path strides too


def test_constant_and_nan(small):
    case = dict(small, gen={k: v.copy() for k, v in small["gen"].items()})
    case["gen"]["a"][0, 0, :, 1, 2] = case["gen"]["a"][0, 0, 0, 1, 2]
    windows = vu.cut(case, [6, 7])
    agg = _run(case, windows)
    logs = _check_against_host(agg, case, windows, "a constant trajectory")
    data = agg.get_data()
    assert float(data["gen_time_std"]["a"][0, 0, 1, 2]) == 0.0 and bool(torch.isnan(data["gen_lag1"]["a"][0, 0, 1, 2]))
    assert int(torch.isnan(data["gen_lag1"]["a"]).sum()) == 1 and not bool(torch.isnan(data["gen_lag1"]["b"]).any())
    assert all(np.isfinite(v) for v in logs.values())
    assert logs["lag1_defined_fraction/a"] < 1.0 - 0.5 * float(case["weights"][1, 2]) / vu.weight_total(case)
    assert logs["lag1_defined_fraction/a"] < logs["lag1_defined_fraction/b"]
    # a NaN input stays in its own trajectory and point
    bad = dict(small, gen={k: v.copy() for k, v in small["gen"].items()})
    bad["gen"]["b"][2, 1, 5, 3, 4] = np.nan
    clean = _state(_run(small, vu.cut(small, [6, 7])), small)
    agg_bad = _run(bad, vu.cut(bad, [6, 7]))
    dirty = _state(agg_bad, bad)
    host, _ = vu.host_state(bad, vu.cut(bad, [6, 7]))
    assert vu.same_state(dirty, host)
    hit = np.zeros(clean["s1"].shape, bool)
    hit[1, 2 * small["B"] + 1, 3, 4] = True
    for k in ("s1", "s2", "p"):
        assert np.isnan(dirty[k][hit]).all() and np.array_equal(dirty[k][~hit], clean[k][~hit])
    lag = agg_bad.get_data()["gen_lag1"]
    assert int(torch.isnan(lag["b"]).sum()) == 1 and bool(torch.isnan(lag["b"][2, 1, 3, 4])) and not bool(torch.isnan(lag["a"]).any())


def test_refusals_leave_the_state_alone(small):
    import sdy_amd

    dev = lambda d: {k: _contiguous(v) for k, v in d.items()}  # noqa: E731
    windows = vu.cut(small, [4, 3, 6])
    agg = _run(small, windows[:2])
    before, n_before, next_before = _state(agg, small), agg.n_times, agg._next_start
    assert (n_before, next_before) == (6, 7)
    start, target, gen = windows[2]

    def unchanged():
        return vu.same_state(_state(agg, small), before) and (agg.n_times, agg._next_start) == (n_before, next_before)

    for wrong in (start + 1, start - 1, 0):                            # a window that does not start where the last ended
        with pytest.raises(ValueError, match="where the one before ended at 7"):
            agg.record_batch(0.0, dev(target), dev(gen), i_time_start=wrong)
        assert unchanged()
    with pytest.raises(ValueError, match="differ from the first window"):                            # another variable set
        agg.record_batch(0.0, dev({"a": target["a"], "c": target["b"]}), dev({"a": gen["a"], "c": gen["b"]}), i_time_start=start)
    with pytest.raises(ValueError, match="differ from the first window"):                            # another member count
        agg.record_batch(0.0, dev(target), dev({k: v[:2] for k, v in gen.items()}), i_time_start=start)
    with pytest.raises(ValueError, match="differ from the first window"):                            # another grid
        agg.record_batch(0.0, dev({k: v[..., :9, :] for k, v in target.items()}), dev({k: v[..., :9, :] for k, v in gen.items()}),
                         i_time_start=start)
    with pytest.raises(ValueError, match="member-stacked"):                                          # a ragged share
        agg.record_batch(0.0, dev(target), dev({k: v.reshape(-1, *v.shape[2:])[:5] for k, v in gen.items()}), i_time_start=start)
    with pytest.raises(ValueError, match="member-stacked"):
        agg.record_batch(0.0, dev(target), dev(gen), i_time_start=start, sample_weights=[0.5, 0.5])
    assert unchanged()
    _feed(agg, windows[2:])                                            # ... and the run goes on where it was
    host, n = vu.host_state(small, windows)
    assert agg.n_times == n == 12 and vu.same_state(_state(agg, small), host)
    # state above max_bytes: nothing is allocated, and nothing is fixed
    need = 32 * 2 * (3 + 1) * 2 * 18 * 36
    tight = sdy_amd.TimeVariabilityAggregator(torch.from_numpy(small["weights"]).cuda(), max_bytes=need - 1)
    with pytest.raises(ValueError, match=f"need {need} bytes"):
        _feed(tight, windows[:1])
    assert tight._names is None and not tight._acc and tight._next_start is None
    _feed(sdy_amd.TimeVariabilityAggregator(torch.from_numpy(small["weights"]).cuda(), max_bytes=need), windows[:1])
    # get_logs before two counted times: the initial condition alone, then one counted time
    young = _run(small, vu.cut(small, [1]))
    assert young.n_times == 0 and young._next_start == 1
    for more in ([], vu.cut(small, [1], start=1)):
        _feed(young, more)
        with pytest.raises(ValueError, match="No data recorded"):
            young.get_logs("x")
        with pytest.raises(ValueError, match="No data recorded"):
            young.get_data()
    assert young.n_times == 1
    _feed(young, vu.cut(small, [1], start=2))
    assert young.n_times == 2 and len(young.get_logs("x")) == 2 * len(vu.LOG_KEYS)


def test_two_runs_give_the_same_logs(small):
    windows = vu.cut(small, [6, 7])
    a, b = _run(small, windows).get_logs("x"), _run(small, windows).get_logs("x")
    assert list(a) == list(b) and all(a[k] == b[k] for k in a)


def test_two_ranks_give_the_logs_of_one():
    """Two shares of whole initial conditions (2 + 1 samples) behind a fake process group: one reduce, and the logs of the
    unsharded run within the bound of the weighted sums."""
    whole = vu.seeded_series(3, 3, 6, 8, 12, ("a", "b"), seed=55)

    class Share:
        def __init__(self):
            self.other, self.sent, self.calls = None, None, 0

        def reduce_sum(self, tensor):
            self.calls += 1
            self.sent = tensor.clone()
            return tensor + self.other.sent if self.other.sent is not None else tensor

    share = lambda lo, hi: dict(whole, B=hi - lo, target={k: v[lo:hi] for k, v in whole["target"].items()},     # noqa: E731
                                gen={k: v[:, lo:hi] for k, v in whole["gen"].items()})
    d0, d1 = Share(), Share()
    d0.other, d1.other = d1, d0
    s0, s1 = share(0, 2), share(2, 3)
    r0, r1 = _run(s0, vu.cut(s0, [7, 6]), dist=d0), _run(s1, vu.cut(s1, [7, 6]), dist=d1)
    r1.get_logs("")
    logs = r0.get_logs("")
    assert d0.calls == d1.calls == 1
    st, n = vu.restate_state(whole, vu.cut(whole, [7, 6]))
    want_raw, scales = vu.restate_stats(st, whole["weights"], n, 3, 3)
    vu.check_logs(logs, vu.logs_from_raw(want_raw, whole["names"], vu.weight_total(whole)), whole["names"], scales, "two ranks")


def test_through_run_inference():
    """InferenceAggregator(time_variability_data=True) behind run_inference on the tiny synthetic stepper, three windows: the
    state of a bare aggregator fed the same windows, bit for bit, and its logs under <label>/time_variability/; with the flag
    off no log key names it and the maps are a KeyError."""
    import sdy_amd
    from sdy_amd import synthetic

    dev = torch.device("cuda", 0)
    n_out, n_forc, nlat, nlon, window, n_windows, members = 4, 2, 32, 64, 6, 3, 2
    exp, _, _ = synthetic.build_sampler(dev, state_chans=n_out, forcing_chans=n_forc, nlat=nlat, nlon=nlon, embed=16, layers=2,
                                        horizon=6, carried_input_only_channel=True)
    stepper, names, out_names = synthetic.build_stepper(exp, n_out, n_forc, carried_input_only_channel=True)
    steps = window * n_windows
    w = sdy_amd.metrics.spherical_area_weights(torch.linspace(-87.0, 87.0, nlat), nlon).cuda()

    class Tee:
        def __init__(self, *aggs):
            self.aggs = aggs

        def record_batch(self, **kw):
            for a in self.aggs:
                a.record_batch(**kw)

    logs = {}
    for on in (False, True):
        agg = sdy_amd.metrics.InferenceAggregator(w, n_timesteps=steps + 1, n_ensemble_members=members, time_variability_data=on)
        alone = sdy_amd.TimeVariabilityAggregator(w)
        sdy_amd.run_inference(Tee(agg, alone), stepper, synthetic.windows(names, n_windows, window, nlat, nlon, n_ics=2, seed=5),
                              steps, window, n_ensemble_members=members, eval_device=dev)
        logs[on] = agg.get_logs("inference")
        if not on:
            assert not any("time_variability" in k for k in logs[on])
            with pytest.raises(KeyError):
                agg.get_time_variability_data()
    inner = agg._aggregators["time_variability"]
    assert inner.n_times == alone.n_times == steps and inner._names == alone._names and sorted(inner._names) == sorted(out_names)
    for k in ("s1", "s2", "p", "pair"):
        assert torch.equal(inner._acc[k].view(torch.int64), alone._acc[k].view(torch.int64)), k
    new = {f"inference/time_variability/{key}/{n}" for n in out_names for key in vu.LOG_KEYS}
    assert set(logs[True]) - set(logs[False]) == new and set(logs[False]) <= set(logs[True])
    want = alone.get_logs("")
    for k, v in want.items():
        got = logs[True][f"inference/time_variability/{k}"]
        assert type(got) is float and (got == v or (np.isnan(got) and np.isnan(v))), k
    data, want_data = agg.get_time_variability_data(), alone.get_data()
    for m in want_data:
        assert list(data[m]) == list(want_data[m]) == inner._names
        for n in out_names:
            assert tuple(data[m][n].shape) == ((members, 2, nlat, nlon) if m.startswith("gen") else (2, nlat, nlon))
            assert torch.equal(data[m][n].nan_to_num(nan=-7.0), want_data[m][n].nan_to_num(nan=-7.0)), (m, n)
    assert bool((data["gen_time_std"][out_names[0]] > 0).all())
