"""Time means and extremes per time bin on the device (`sdy_amd.BinnedTimeMeanAggregator`, `sdy_amd.time_bins.binned_time_mean`;
kernel of csrc/time_bins.hip) against the library's _host twin (sums and extremes: the same bits) and the numpy float64
restatement (read-outs and logs: 1e-12 of the term scale, the project's bound for float64 restatements): windowing, layouts,
the scalar path, the grid stride, windows longer than one call, pooled members, refusals, and the way through run_inference.
Every case is a handful of launches."""
import numpy as np
import pytest
import torch

import time_bins_utils as tu

pytestmark = pytest.mark.gpu

BOUNDARY = np.array([0] * 6 + [1] * 7 + [2])        # a bin boundary inside a window; bin 2 has no counted time of the run
ROTATING = np.array([t % 4 for t in range(13)])


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


def _run(case, windows, labels, layout=_contiguous, target_layout=_contiguous, names=None, **kw):
    import sdy_amd

    kw.setdefault("extremes", True)
    bins = sdy_amd.TimeBins.from_labels(labels, names)
    return _feed(sdy_amd.BinnedTimeMeanAggregator(bins, torch.from_numpy(case["weights"]).cuda(), **kw), windows, layout, target_layout)


def _state(agg, case):
    """The accumulators of a case whose variables are one run, shaped as tu.empty_state shapes them."""
    n, B, H, W = len(case["names"]), case["B"], case["H"], case["W"]
    out = {}
    for k, buf in {**agg._acc, **agg._ext}.items():
        rows = (case["M"] * B if agg._per_member else B) if k.startswith("gen") else B
        out[k] = buf.view(agg._bins.n_bins, n, rows, H, W).cpu().numpy()
    return out


def _check_against_host(agg, case, windows, labels, what):
    host, counts = tu.host_state(case, windows, labels, agg._bins.n_bins, agg._per_member, agg._extremes)
    keys = tuple(host) if agg._extremes else ("gen_sum", "target_sum")
    assert agg.counts() == counts and tu.same_state(_state(agg, case), host, keys), what


def _check_readouts(agg, case, labels, what):
    """get_bin_means, get_extremes and the logs against the numpy float64 restatement."""
    n_bins, names = agg._bins.n_bins, agg._bins.names
    want, counts = tu.restate_means(case, labels, n_bins, agg._per_member)
    assert agg.counts() == counts
    means = agg.get_bin_means()
    assert list(means) == ["gen", "target"]
    M, B, H, W = case["M"] if agg._per_member else 1, case["B"], case["H"], case["W"]
    scales = {}
    for side in means:
        assert list(means[side]) == case["names"]
        for name, x in means[side].items():
            assert x.dtype == torch.float64 and x.is_cuda
            assert tuple(x.shape) == ((n_bins, M, B, H, W) if side == "gen" else (n_bins, B, H, W))
            got, ref = x.cpu().numpy(), want[side][name]
            assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, side, name)
            for b in range(n_bins):
                assert bool(np.isnan(got[b]).all()) == (counts[b] == 0)
            scales[name] = max(scales.get(name, 0.0), float(np.nanmax(np.abs(ref))))
            err = float(np.nanmax(np.abs(got - ref)))
            print(f"{what} {side} {name}: mean off by {err:.3e} of scale {scales[name]:.3e}")
            assert err <= 1e-12 * scales[name], (what, side, name)
    if agg._extremes:
        ext = agg.get_extremes()
        assert list(ext) == ["gen_max", "gen_min", "target_max", "target_min"]
        for k in ext:
            for name, x in ext[k].items():
                assert x.dtype == torch.float32 and tuple(x.shape) == tuple(want[k][name].shape)
                assert np.array_equal(x.cpu().numpy(), want[k][name], equal_nan=True), (what, k, name)
    logs = agg.get_logs("")
    per_member_means = tu.restate_means(case, labels, n_bins, True)[0] if agg._per_member else want
    want_logs, scales = tu.restate_logs(case, per_member_means, counts, names)
    assert list(logs) == list(want_logs), (what, sorted(set(logs) ^ set(want_logs)))
    for k, v in want_logs.items():
        got, name = logs[k], k.rsplit("/", 1)[1]
        assert type(got) is float
        # a ratio of two such means: the errors of both, relative to the denominator
        tol = 1e-12 * scales[name] * ((1.0 + abs(v)) / want_logs[k.replace("_ratio", "_target")] if "_ratio/" in k else 1.0)
        print(f"{what} {k}: {got!r} against {v!r}, tolerance {tol:.3e}")
        assert abs(got - v) <= tol, (what, k, got, v)
    return logs


@pytest.fixture(scope="module")
def small():
    """3 members, 2 samples, 18 x 36, two variables, 12 counted times."""
    return tu.seeded_case(3, 2, 18, 36, 12, ("a", "b"), seed=302, mean=2.0, std=30.0)


def test_state_equals_the_host_twin_and_does_not_depend_on_the_windows(small):
    labels = BOUNDARY[:13]
    assert sum(tu.SPLIT) == small["S"] + 1 == 13
    one = _run(small, tu.cut(small, [13]), labels)
    many = _run(small, tu.cut(small, tu.SPLIT), labels)
    assert one.counts() == many.counts() == [5, 7]
    assert tu.same_state(_state(one, small), _state(many, small))
    _check_against_host(one, small, tu.cut(small, [13]), labels, "one window")
    _check_against_host(many, small, tu.cut(small, tu.SPLIT), labels, "windows of 0, 1, 1, 3, 7")
    rot_one = _run(small, tu.cut(small, [13]), ROTATING)
    rot_many = _run(small, tu.cut(small, tu.SPLIT), ROTATING)
    assert tu.same_state(_state(rot_one, small), _state(rot_many, small))
    _check_against_host(rot_many, small, tu.cut(small, tu.SPLIT), ROTATING, "rotating labels")
    _check_readouts(many, small, labels, "two bins")
    assert list(many.get_logs("full")) == [f"full/{k}" for k in many.get_logs("")]


def test_layouts_give_the_same_bits(small):
    """Contiguous, the transposed view of a (samples, members, ...) buffer, and views one element into a larger buffer (scalar
    loads): the order of every sum is fixed, so the state is bit-identical."""
    windows = tu.cut(small, [5, 8])
    for per_member in (True, False):
        ref = _state(_run(small, windows, ROTATING, per_member=per_member), small)
        for layout, target_layout in ((_transposed, _contiguous), (_offset, _contiguous), (_offset, _offset)):
            got = _state(_run(small, windows, ROTATING, layout, target_layout, per_member=per_member), small)
            assert tu.same_state(got, ref), (layout.__name__, per_member)
        _check_against_host(_run(small, windows, ROTATING, _transposed, per_member=per_member), small, windows, ROTATING, "transposed")


def test_a_grid_that_is_no_multiple_of_four():
    """5 x 7: scalar loads, fewer items than one block."""
    case = tu.seeded_case(2, 1, 5, 7, 9, ("a", "b", "c"), seed=303)
    labels = np.array([0, 2, -1, 1, 1, 2, -1, 0, 2, 2])
    windows = tu.cut(case, [3, 7])
    agg = _run(case, windows, labels, _transposed, names=["x", "y", "z", "never"])
    _check_against_host(agg, case, windows, labels, "5 x 7")
    logs = _check_readouts(agg, case, labels, "5 x 7")
    assert not any("/never/" in k for k in logs) and "rmse/z/c" in logs and "crps/x/a" in logs
    # without the extremes: the other instantiations, the same sums
    plain = _run(case, windows, labels, _transposed, names=["x", "y", "z", "never"], extremes=False)
    assert not plain._ext and tu.same_state(_state(plain, case), _state(agg, case), ("gen_sum", "target_sum"))
    with pytest.raises(ValueError, match="extremes"):
        plain.get_extremes()


def test_grid_stride():
    """3 variables, 5 members, 2 samples, 3 counted times on 180 x 360: 12 rows x 16200 items of four points = 760 blocks per
    variable against the launch's 1024 / 3 = 341 (kBlocksPerLaunch over the variables): every thread strides."""
    case = tu.seeded_case(5, 2, 180, 360, 3, ("a", "b", "c"), seed=304, mean=101325.0, std=50.0)
    labels = np.array([0, 1, 0, 1])
    windows = tu.cut(case, [3], start=1)
    agg = _run(case, windows, labels, _transposed)
    assert agg.counts() == [1, 2]
    _check_against_host(agg, case, windows, labels, "180 x 360")
    assert tu.same_state(_state(_run(case, windows, labels, _offset, _offset), case), _state(agg, case))      # the scalar path strides too


def test_more_counted_times_than_one_call_takes():
    """A window of 71 times, 70 of them counted: calls of 64 and 6 times; the bits of the host twin fed one time per window."""
    case = tu.seeded_case(2, 1, 4, 8, 70, ("a",), seed=305)
    labels = np.array([t % 3 for t in range(71)])
    agg = _run(case, tu.cut(case, [71]), labels)
    assert agg.counts() == [23, 24, 23]
    _check_against_host(agg, case, tu.cut(case, [1] * 71), labels, "71 times")
    _check_readouts(agg, case, labels, "71 times")


def test_pooled_members_are_the_member_ordered_chain(small):
    windows = tu.cut(small, [4, 9])
    agg = _run(small, windows, ROTATING, _transposed, per_member=False)
    _check_against_host(agg, small, windows, ROTATING, "pooled")
    got = _state(agg, small)["gen_sum"]
    for b in range(4):
        acc = np.zeros((small["B"], small["H"], small["W"]))
        for t in [t for t in range(1, 13) if ROTATING[t] == b]:
            for m in range(small["M"]):
                acc = acc + small["gen"]["b"][m, :, t].astype(np.float64)
        assert np.array_equal(got[b, 1], acc)
    _check_readouts(agg, small, ROTATING, "pooled")


def test_bin_scores_equal_the_ensemble_time_mean_of_the_bin():
    """Integer-valued data (float64 sums are exact in any order): the per-bin rmse / bias / crps are the numbers of
    EnsembleTimeMeanAggregator.get_logs fed only that bin's times, to the bit."""
    import sdy_amd

    case = tu.seeded_case(3, 2, 18, 36, 12, ("a", "b"), seed=306, integer=True)
    labels = np.array([2, 0, -1, 0, 1, -1, -1, 1, 2, 0, 2, -1, 1])
    agg = _run(case, tu.cut(case, [6, 7]), labels, names=["x", "y", "z"])
    logs = agg.get_logs("")
    for b, bin_name in enumerate(agg._bins.names):
        ts = [t for t in tu.counted(case, labels) if labels[t] == b]
        alone = sdy_amd.EnsembleTimeMeanAggregator(torch.from_numpy(case["weights"]).cuda())
        alone.record_batch(0.0, {k: _contiguous(v[:, ts]) for k, v in case["target"].items()},
                           {k: _contiguous(v[:, :, ts]) for k, v in case["gen"].items()}, i_time_start=1)
        want = alone.get_logs("")
        assert len(want) == 10
        for k, v in want.items():
            metric, name = k.split("/")
            assert logs[f"{metric}/{bin_name}/{name}"] == v, (k, bin_name)


def test_refusals_leave_the_state_alone(small):
    import sdy_amd

    dev = lambda d: {k: _contiguous(v) for k, v in d.items()}  # noqa: E731
    labels = BOUNDARY[:12]                                             # (the run's last time is not labelled)
    windows = tu.cut(small, [4, 3, 5, 1])
    bins = lambda: sdy_amd.TimeBins.from_labels(labels, ["x", "y", "z"])  # noqa: E731
    agg = _run(small, windows[:2], labels, names=["x", "y", "z"])
    before, n_before, next_before = _state(agg, small), agg.counts(), agg._next_start
    assert (n_before, next_before) == ([5, 1, 0], 7)
    start, target, gen = windows[2]

    def unchanged():
        return tu.same_state(_state(agg, small), before) and (agg.counts(), agg._next_start) == (n_before, next_before)

    for wrong in (start - 1, 4, 0):                                    # going back in time
        with pytest.raises(ValueError, match="before the end of the last recorded one"):
            agg.record_batch(0.0, dev(target), dev(gen), i_time_start=wrong)
        assert unchanged()
    with pytest.raises(ValueError, match="outside the 12 times the bins label"):                     # times outside the labels
        agg.record_batch(0.0, dev(target), dev(gen), i_time_start=8)
    with pytest.raises(ValueError, match="outside the 12 times"):
        agg.record_batch(0.0, dev(windows[3][1]), dev(windows[3][2]), i_time_start=12)
    with pytest.raises(ValueError, match="differ from the first window"):                            # another variable set
        agg.record_batch(0.0, dev({"a": target["a"], "c": target["b"]}), dev({"a": gen["a"], "c": gen["b"]}), i_time_start=start)
    with pytest.raises(ValueError, match="differ from the first window"):                            # another member count
        agg.record_batch(0.0, dev(target), dev({k: v[:2] for k, v in gen.items()}), i_time_start=start)
    with pytest.raises(ValueError, match="differ from the first window"):                            # another grid
        agg.record_batch(0.0, dev({k: v[..., :9, :] for k, v in target.items()}), dev({k: v[..., :9, :] for k, v in gen.items()}),
                         i_time_start=start)
    with pytest.raises(ValueError, match="member-stacked"):                                          # a ragged share
        agg.record_batch(0.0, dev(target), dev(gen), i_time_start=start, sample_weights=[0.5, 0.5])
    with pytest.raises(RuntimeError, match="GPU only"):                                              # a CPU tensor
        agg.record_batch(0.0, {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in target.items()}, dev(gen), i_time_start=start)
    assert unchanged()
    _feed(agg, windows[2:3])                                           # ... and the run goes on where it was
    host, counts = tu.host_state(small, windows[:3], labels, 3)
    assert agg.counts() == counts == [5, 6, 0] and tu.same_state(_state(agg, small), host)
    # accumulators above max_bytes: nothing is allocated, and nothing is fixed
    need = 3 * 2 * (3 + 1) * 2 * 18 * 36 * 16                          # bins x variables x rows x points; a sum, a maximum, a minimum
    w = torch.from_numpy(small["weights"]).cuda()
    tight = sdy_amd.BinnedTimeMeanAggregator(bins(), w, extremes=True, max_bytes=need - 1)
    with pytest.raises(ValueError, match=f"3 bins x 2 variables x 3 member maps.* need {need} bytes"):
        _feed(tight, windows[:1])
    assert tight._names is None and not tight._acc and not tight._ext and tight._next_start is None
    _feed(sdy_amd.BinnedTimeMeanAggregator(bins(), w, extremes=True, max_bytes=need), windows[:1])
    # variables= selects before anything is laid out
    only = _feed(sdy_amd.BinnedTimeMeanAggregator(bins(), w, variables=["b"], max_bytes=need // 4),
                 windows[:2])
    assert only._names == ["b"] and torch.equal(only._acc["gen_sum"].view(3, 6, 18, 36), agg_first_two(small, labels)[:, 1])
    with pytest.raises(ValueError, match="no generated variable 'q'"):
        _feed(sdy_amd.BinnedTimeMeanAggregator(bins(), w, variables=["q"]), windows[:1])
    # nothing counted yet: the initial condition alone
    young = _run(small, tu.cut(small, [1]), labels, names=["x", "y", "z"])
    assert young.counts() == [0, 0, 0] and young._next_start == 1
    _feed(young, tu.cut(small, [2], start=9))                          # a gap is allowed
    assert young.counts() == [0, 2, 0] and young._next_start == 11 and len(young.get_logs("x")) == 10
    fresh = _run(small, tu.cut(small, [1]), labels, names=["x", "y", "z"])
    for read in (fresh.get_logs, lambda _: fresh.get_bin_means(), lambda _: fresh.get_extremes()):
        with pytest.raises(ValueError, match="No data recorded"):
            read("x")


def agg_first_two(case, labels):
    host, _ = tu.host_state(case, tu.cut(case, [4, 3]), labels, 3, extremes=False)
    return torch.from_numpy(host["gen_sum"]).cuda()


def test_two_ranks_give_the_logs_of_one():
    """Two shares of whole initial conditions (2 + 1 samples) behind a fake process group: one reduce, and the logs of the
    unsharded run."""
    whole = tu.seeded_case(3, 3, 6, 8, 12, ("a", "b"), seed=307)

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
    r0, r1 = _run(s0, tu.cut(s0, [7, 6]), ROTATING, dist=d0), _run(s1, tu.cut(s1, [7, 6]), ROTATING, dist=d1)
    r1.get_logs("")
    logs = r0.get_logs("")
    assert d0.calls == d1.calls == 1
    means, counts = tu.restate_means(whole, ROTATING, 4)
    want, scales = tu.restate_logs(whole, means, counts, r0._bins.names)
    assert list(logs) == list(want)
    for k, v in want.items():
        tol = 1e-12 * scales[k.rsplit("/", 1)[1]] * ((1.0 + abs(v)) / want[k.replace("_ratio", "_target")] if "_ratio/" in k else 1.0)
        assert abs(logs[k] - v) <= tol, (k, logs[k], v)


def test_one_field_function(small):
    from sdy_amd import time_bins

    x = small["gen"]["a"]
    labels = np.array([0, 1, -1, 1, 1, 0, 3, 3, 0, 1, 0, -1, 3])
    out = time_bins.binned_time_mean(_transposed(x), labels, extremes=True)
    assert list(out) == ["mean", "count", "max", "min"] and out["count"].tolist() == [4, 4, 0, 3]
    assert tuple(out["mean"].shape) == (4, 3, 2, 18, 36) and out["mean"].dtype == torch.float64 and out["max"].dtype == torch.float32
    for b in range(4):
        ts = [t for t in range(13) if labels[t] == b]
        if not ts:
            assert all(bool(torch.isnan(out[k][b]).all()) for k in ("mean", "max", "min"))
            continue
        acc = np.zeros(x[:, :, 0].shape)
        for t in ts:
            acc = acc + x[:, :, t].astype(np.float64)
        assert np.array_equal(out["mean"][b].cpu().numpy(), acc / len(ts))
        assert np.array_equal(out["max"][b].cpu().numpy(), x[:, :, ts].max(axis=2))
        assert np.array_equal(out["min"][b].cpu().numpy(), x[:, :, ts].min(axis=2))
    flat = time_bins.binned_time_mean(_contiguous(x[0, 0]), labels)
    assert list(flat) == ["mean", "count"] and torch.equal(flat["mean"].nan_to_num(nan=-7.0), out["mean"][:, 0, 0].nan_to_num(nan=-7.0))
    with pytest.raises(ValueError, match="12 labels for 13 times"):
        time_bins.binned_time_mean(_contiguous(x), labels[:12])


def test_through_run_inference():
    """InferenceAggregator(time_bins=...) behind run_inference on the tiny synthetic stepper, three windows of six steps with
    hour_of_day bins: the state of a bare aggregator fed the same windows, bit for bit, and its logs under
    <label>/time_bins/; with the default no log key names it and the data are a KeyError."""
    import sdy_amd
    from sdy_amd import synthetic

    dev = torch.device("cuda", 0)
    n_out, n_forc, nlat, nlon, window, n_windows, members = 4, 2, 32, 64, 6, 3, 2
    exp, _, _ = synthetic.build_sampler(dev, state_chans=n_out, forcing_chans=n_forc, nlat=nlat, nlon=nlon, embed=16, layers=2,
                                        horizon=6, carried_input_only_channel=True)
    stepper, names, out_names = synthetic.build_stepper(exp, n_out, n_forc, carried_input_only_channel=True)
    steps = window * n_windows
    w = sdy_amd.metrics.spherical_area_weights(torch.linspace(-87.0, 87.0, nlat), nlon).cuda()
    bins = sdy_amd.TimeBins.calendar("hour_of_day", (2001, 1, 1), steps + 1)
    assert bins.n_bins == 4

    class Tee:
        def __init__(self, *aggs):
            self.aggs = aggs

        def record_batch(self, **kw):
            for a in self.aggs:
                a.record_batch(**kw)

    logs = {}
    for on in (False, True):
        agg = sdy_amd.metrics.InferenceAggregator(w, n_timesteps=steps + 1, n_ensemble_members=members,
                                                  time_bins=bins if on else None, time_bin_extremes=on)
        alone = sdy_amd.BinnedTimeMeanAggregator(bins, w, extremes=True)
        sdy_amd.run_inference(Tee(agg, alone), stepper, synthetic.windows(names, n_windows, window, nlat, nlon, n_ics=2, seed=5),
                              steps, window, n_ensemble_members=members, eval_device=dev)
        logs[on] = agg.get_logs("inference")
        if not on:
            assert not any("time_bins" in k for k in logs[on])
            with pytest.raises(KeyError):
                agg.get_time_bin_data()
    inner = agg._aggregators["time_bins"]
    counts = [int(c) for c in np.bincount(bins.labels[1:], minlength=4)]
    assert inner.counts() == alone.counts() == counts and sum(counts) == steps
    assert inner._names == alone._names and sorted(inner._names) == sorted(out_names)
    for k in ("gen_sum", "target_sum"):
        assert torch.equal(inner._acc[k].view(torch.int64), alone._acc[k].view(torch.int64)), k
    for k in inner._ext:
        assert torch.equal(inner._ext[k].view(torch.int32), alone._ext[k].view(torch.int32)), k
    per_bin = ("rmse_member_avg", "bias_member_avg", "rmse", "bias", "crps")
    across = ("bin_range_gen", "bin_range_target", "bin_range_ratio", "bin_std_gen", "bin_std_target", "bin_std_ratio", "centred_rmse")
    new = {f"inference/time_bins/{key}/{b}/{n}" for n in out_names for key in per_bin for b in bins.names}
    new |= {f"inference/time_bins/{key}/{n}" for n in out_names for key in across}
    assert set(logs[True]) - set(logs[False]) == new and set(logs[False]) <= set(logs[True])
    for k, v in alone.get_logs("").items():
        got = logs[True][f"inference/time_bins/{k}"]
        assert type(got) is float and (got == v or (np.isnan(got) and np.isnan(v))), k
    data = agg.get_time_bin_data()
    assert list(data) == ["counts", "means", "extremes"] and data["counts"] == counts
    for n in out_names:
        assert tuple(data["means"]["gen"][n].shape) == (4, members, 2, nlat, nlon)
        assert tuple(data["means"]["target"][n].shape) == (4, 2, nlat, nlon)
        assert torch.equal(data["means"]["gen"][n], alone.get_bin_means()["gen"][n])
        assert bool((data["extremes"]["gen_max"][n] >= data["extremes"]["gen_min"][n]).all())
        mean32 = data["means"]["gen"][n]
        assert bool((data["extremes"]["gen_max"][n].double() >= mean32).all() and (data["extremes"]["gen_min"][n].double() <= mean32).all())
