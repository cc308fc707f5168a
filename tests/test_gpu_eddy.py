"""Transient-eddy covariances on the device (`sdy_amd.EddyCovarianceAggregator`; kernels of csrc/time_covariance.hip) against the
library's _host twins (state and maps: the same bits; weighted sums: the bound of another summation order) and the float64
restatement: windowing, layouts, grids, members and batch, the grid stride, NaN containment, refusals, the logs, and the way
through run_inference.  Bounds: tests/eddy_utils.py.  Every case is a handful of launches."""
import numpy as np
import pytest
import torch

import eddy_utils as eu

pytestmark = pytest.mark.gpu

GROUPS = {"low": {"u": "ua", "v": "va", "T": "ta", "q": "qa"}, "wind": {"v": "va", "w": "wa"}}


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


def _groups(case):
    import sdy_amd

    groups = sdy_amd.CovarianceGroups()
    for label, g in case["groups"].items():
        groups.add(label, g)
    return groups


def _feed(agg, windows, layout=_contiguous, target_layout=_contiguous):
    for start, target, gen in windows:
        agg.record_batch(0.0, {k: target_layout(v) for k, v in target.items()}, {k: layout(v) for k, v in gen.items()},
                         i_time_start=start)
    return agg


def _run(case, windows, layout=_contiguous, target_layout=_contiguous, **kw):
    import sdy_amd

    return _feed(sdy_amd.EddyCovarianceAggregator(_groups(case), torch.from_numpy(case["weights"]).cuda(), **kw), windows, layout,
                 target_layout)


def _state(agg, case):
    rows, H, W = (case["M"] + 1) * case["B"], case["H"], case["W"]
    return {b.K: dict(labels=b.labels, sums=b.sums.view(len(b.labels), b.K, rows, H, W).cpu().numpy(),
                      products=b.products.view(len(b.labels), eu.n_pairs(b.K), rows, H, W).cpu().numpy(),
                      origins=b.origins.view(len(b.labels), b.K, rows, H, W).cpu().numpy()) for b in agg._blocks}


def _raw(agg):
    return {label: s.cpu().numpy() for label, s in agg.weighted_sums().items()}


def _check_against_host(agg, case, windows, what):
    """State and maps: the _host twin's bits; weighted sums: the _host twin's and the restatement's within the bound; the logs
    against the restatement's.  -> the device's logs."""
    host, n = eu.host_state(case, windows)
    assert agg.n_times == n
    got = _state(agg, case)
    assert eu.same_state(got, host), what
    M, B, H, W = case["M"], case["B"], case["H"], case["W"]
    for label, g in case["groups"].items():
        K, shorts = len(g), list(g)
        blk, gi = host[K], host[K]["labels"].index(label)
        for i in range(K):
            for j in range(i, K):
                cov, corr = eu.host_maps(blk, gi, i, j, n)
                data = agg.get_pair_data(label, shorts[j], shorts[i])              # (the order of the shorts does not matter)
                assert list(data) == ["gen_cov", "gen_corr", "target_cov", "target_corr", "gen_cov_zonal", "target_cov_zonal"]
                assert all(x.dtype == torch.float64 and x.is_cuda for x in data.values())
                assert tuple(data["gen_cov"].shape) == tuple(data["gen_corr"].shape) == (M, B, H, W)
                assert tuple(data["target_cov"].shape) == tuple(data["target_corr"].shape) == (B, H, W)
                assert tuple(data["gen_cov_zonal"].shape) == tuple(data["target_cov_zonal"].shape) == (B, H)
                for kind, m in (("cov", cov), ("corr", corr)):
                    assert np.array_equal(data[f"gen_{kind}"].cpu().numpy(), m[:M * B].reshape(M, B, H, W), equal_nan=True), what
                    assert np.array_equal(data[f"target_{kind}"].cpu().numpy(), m[M * B:], equal_nan=True), what
                zonal = cov[:M * B].reshape(M, B, H, W).mean(axis=0).mean(axis=-1)
                scale = float(np.nanmax(np.abs(cov)))
                if np.isfinite(zonal).all():
                    assert np.abs(data["gen_cov_zonal"].cpu().numpy() - zonal).max() <= 1e-12 * scale, what
                    assert np.abs(data["target_cov_zonal"].cpu().numpy() - cov[M * B:].mean(axis=-1)).max() <= 1e-12 * scale, what
    want_stats = {K: eu.restate_stats(blk, case["weights"], n, M, B) for K, blk in host.items()}
    total = eu.weight_total(case)
    raw = _raw(agg)
    for K, blk in host.items():
        dev_raw = np.stack([raw[l] for l in blk["labels"]])
        eu.check_raw(dev_raw, eu.host_stats(blk, case["weights"], n, M, B), want_stats[K][1], total, f"{what}, K = {K}: device vs host")
        eu.check_raw(dev_raw, want_stats[K][0], want_stats[K][1], total, f"{what}, K = {K}: device vs restatement")
    want_raw = eu.per_group(case, host, {K: v[0] for K, v in want_stats.items()})
    scales = eu.per_group(case, host, {K: v[1] for K, v in want_stats.items()})
    logs = agg.get_logs("")
    eu.check_logs(logs, eu.logs_from_raw(want_raw, case["groups"], total), case["groups"], scales, what)
    return logs


@pytest.fixture(scope="module")
def small():
    """3 members, 2 samples, 18 x 36, a K = 4 group and a K = 2 group that share a variable, 12 counted times."""
    return eu.seeded_groups(3, 2, 18, 36, 12, GROUPS, seed=402)


def test_state_does_not_depend_on_the_windows(small):
    """One window against the initial condition alone followed by windows of 1, 1, 3 and 7 counted times; device against host."""
    assert sum(eu.SPLIT) == small["S"] + 1 == 13
    one = _run(small, eu.cut(small, [13]))
    many = _run(small, eu.cut(small, eu.SPLIT))
    assert one.n_times == many.n_times == 12
    assert eu.same_state(_state(one, small), _state(many, small))
    logs = _check_against_host(many, small, eu.cut(small, eu.SPLIT), "windows of 0, 1, 1, 3, 7")
    assert list(many.get_logs("full")) == [f"full/{k}" for k in logs]
    # the prescribed cross-correlation lambda_a lambda_b shows in the logs (12 times per point: a loose look, not a bound)
    lam = small["loading"]
    assert np.sign(logs["corr_target/low/u_v"]) == np.sign(lam["ua"] * lam["va"]) and abs(logs["corr_target/low/u_v"]) > 0.2
    # the time means are the means of the counted times
    means = many.get_means("wind")
    x = small["gen"]["wa"][:, :, 1:].astype(np.float64).mean(axis=2)
    assert list(means) == ["gen", "target"] and list(means["gen"]) == ["v", "w"]
    assert np.allclose(means["gen"]["w"].cpu().numpy(), x, rtol=1e-14, atol=0.0)
    assert np.allclose(means["target"]["v"].cpu().numpy(), small["target"]["va"][:, 1:].astype(np.float64).mean(axis=1), rtol=1e-14, atol=0.0)


def test_layouts_give_the_same_bits(small):
    """Contiguous, the transposed view of a (samples, members, ...) buffer, and views one element into a larger buffer (scalar
    loads): the order of every sum is fixed, so the state is bit-identical."""
    windows = eu.cut(small, [5, 8])
    ref = _state(_run(small, windows), small)
    for layout, target_layout in ((_transposed, _contiguous), (_offset, _contiguous), (_offset, _offset)):
        assert eu.same_state(_state(_run(small, windows, layout, target_layout), small), ref), layout.__name__
    _check_against_host(_run(small, windows, _transposed), small, windows, "transposed")
    # variables of one launch whose strides differ: copied once, the same bits
    mixed = _run(small, [])
    for start, target, gen in windows:
        mixed.record_batch(0.0, {k: _contiguous(v) for k, v in target.items()},
                           {k: (_transposed if k == "va" else _contiguous)(v) for k, v in gen.items()}, i_time_start=start)
    assert eu.same_state(_state(mixed, small), ref)


def test_a_grid_that_is_no_multiple_of_four():
    case = eu.seeded_groups(2, 3, 7, 9, 9, {"g": {"a": "a", "b": "b", "c": "c"}, "h": {"c": "c", "a": "a", "d": "d"}}, seed=403)
    windows = eu.cut(case, [3, 7])
    _check_against_host(_run(case, windows, _transposed), case, windows, "7 x 9")


def test_one_member_from_flat_rows():
    """A 4-D gen is one member."""
    case = eu.seeded_groups(1, 2, 16, 32, 9, {"g": {"u": "u", "v": "v"}}, seed=404)
    windows = eu.cut(case, [4, 6])
    flat = [(s, t, {k: v[0] for k, v in g.items()}) for s, t, g in windows]
    agg = _run(case, flat)
    assert tuple(agg.get_pair_data("g", "u", "v")["gen_corr"].shape) == (1, 2, 16, 32)
    logs = _check_against_host(agg, case, windows, "one member")
    assert "eke_ratio/g" in logs


def test_25_members_and_batch_independence():
    """M = 25 on 16 x 32; sample 0's state from the B = 2 run equals that of a run on sample 0 alone, bit for bit."""
    case = eu.seeded_groups(25, 2, 16, 32, 8, {"g": {"u": "u", "v": "v", "T": "T"}}, seed=405)
    windows = eu.cut(case, [3, 6])
    agg = _run(case, windows, _transposed)
    _check_against_host(agg, case, windows, "25 members")
    one = dict(case, B=1, target={k: v[:1] for k, v in case["target"].items()}, gen={k: v[:, :1] for k, v in case["gen"].items()})
    alone = _state(_run(one, eu.cut(one, [3, 6]), _transposed), one)
    both = _state(agg, case)
    rows = [2 * m for m in range(25)] + [50]                    # member m of sample 0, and sample 0's target
    assert all(np.array_equal(both[3][k][:, :, rows], alone[3][k]) for k in ("sums", "products", "origins"))


def test_grid_stride():
    """Four K = 2 groups in one launch, 2 members, 3 samples, 2 times on 180 x 360, surface-pressure-like data: 9 rows x 16200
    items of four points = 145800 items = 570 blocks per group against the launch's 1024 / 4 = 256 (kBlocksPerLaunch over the
    groups): every thread takes at least two items.  9 is the fewest rows with more than 2 x 256 blocks, (2 + 1) x 3 the fewest
    members and samples that make 9 rows with more than one of each, and two times the fewest that form a product of two
    different deviations.  A run that starts at time 5 counts both times.  The scalar path (64800 items per row, 2279 blocks)
    strides nine times."""
    groups = {"ab": {"a": "a", "b": "b"}, "bc": {"b": "b", "c": "c"}, "ca": {"c": "c", "a": "a"}, "ba": {"b": "b", "a": "a"}}
    case = eu.seeded_groups(2, 3, 180, 360, 6, groups, seed=406, means={k: 101325.0 for k in "abc"}, std=50.0, phi=0.9)
    windows = eu.cut(case, [2], start=5)
    agg = _run(case, windows, _transposed)
    assert agg.n_times == 2 and (9 * 16200 + 255) // 256 == 570 > 2 * (1024 // 4)
    _check_against_host(agg, case, windows, "180 x 360")
    assert eu.same_state(_state(_run(case, windows, _offset, _offset), case), _state(agg, case))       # the scalar path strides too


def test_nan_stays_in_its_variable(small):
    """A NaN in one variable at one point and trajectory makes NaN exactly that variable's sums and the products that involve it;
    every other bit equals the clean run's."""
    bad = dict(small, gen={k: v.copy() for k, v in small["gen"].items()})
    bad["gen"]["va"][2, 1, 5, 3, 4] = np.nan
    clean = _state(_run(small, eu.cut(small, [6, 7])), small)
    agg_bad = _run(bad, eu.cut(bad, [6, 7]))
    dirty = _state(agg_bad, bad)
    host, _ = eu.host_state(bad, eu.cut(bad, [6, 7]))
    assert eu.same_state(dirty, host)
    row = 2 * small["B"] + 1
    for K, k_bad in ((4, 1), (2, 0)):
        hit_s = np.zeros(clean[K]["sums"].shape, bool)
        hit_s[0, k_bad, row, 3, 4] = True
        hit_p = np.zeros(clean[K]["products"].shape, bool)
        for i in range(K):
            for j in range(i, K):
                if k_bad in (i, j):
                    hit_p[0, eu.pair_index(K, i, j), row, 3, 4] = True
        for key, hit in (("sums", hit_s), ("products", hit_p)):
            assert np.isnan(dirty[K][key][hit]).all() and np.array_equal(dirty[K][key][~hit], clean[K][key][~hit])
        assert np.array_equal(dirty[K]["origins"], clean[K]["origins"])
    corr = agg_bad.get_pair_data("low", "v", "T")["gen_corr"]
    assert int(torch.isnan(corr).sum()) == 1 and bool(torch.isnan(corr[2, 1, 3, 4]))
    assert not bool(torch.isnan(agg_bad.get_pair_data("low", "u", "T")["gen_corr"]).any())


def test_refusals_leave_the_state_alone(small):
    import sdy_amd

    dev = lambda d: {k: _contiguous(v) for k, v in d.items()}  # noqa: E731
    windows = eu.cut(small, [4, 3, 6])
    agg = _run(small, windows[:2])
    before, n_before, next_before = _state(agg, small), agg.n_times, agg._next_start
    assert (n_before, next_before) == (6, 7)
    start, target, gen = windows[2]

    def unchanged():
        return eu.same_state(_state(agg, small), before) and (agg.n_times, agg._next_start) == (n_before, next_before)

    for wrong in (start + 1, start - 1, 0):                            # a window that does not start where the last ended
        with pytest.raises(ValueError, match="where the one before ended at 7"):
            agg.record_batch(0.0, dev(target), dev(gen), i_time_start=wrong)
        assert unchanged()
    with pytest.raises(ValueError, match="differ from the first window"):                            # other variables
        agg.record_batch(0.0, dev(dict(target, extra=target["ua"])), dev(dict(gen, extra=gen["ua"])), i_time_start=start)
    with pytest.raises(ValueError, match="differ from the first window"):                            # another member count
        agg.record_batch(0.0, dev(target), dev({k: v[:2] for k, v in gen.items()}), i_time_start=start)
    with pytest.raises(ValueError, match="differ from the first window"):                            # another grid
        agg.record_batch(0.0, dev({k: v[..., :9, :] for k, v in target.items()}), dev({k: v[..., :9, :] for k, v in gen.items()}),
                         i_time_start=start)
    with pytest.raises(ValueError, match="member-stacked"):                                          # a ragged share
        agg.record_batch(0.0, dev(target), dev({k: v.reshape(-1, *v.shape[2:])[:5] for k, v in gen.items()}), i_time_start=start)
    with pytest.raises(ValueError, match="member-stacked"):
        agg.record_batch(0.0, dev(target), dev(gen), i_time_start=start, sample_weights=[0.5, 0.5])
    with pytest.raises(ValueError, match="'qa' of a group is missing"):                              # a group's variable is missing
        agg.record_batch(0.0, dev({k: v for k, v in target.items() if k != "qa"}), dev({k: v for k, v in gen.items() if k != "qa"}),
                         i_time_start=start)
    assert unchanged()
    _feed(agg, windows[2:])                                            # ... and the run goes on where it was
    host, n = eu.host_state(small, windows)
    assert agg.n_times == n == 12 and eu.same_state(_state(agg, small), host)
    # state above max_bytes: nothing is allocated, and nothing is fixed
    need = (128 + 48) * (3 + 1) * 2 * 18 * 36               # 128 bytes per trajectory and point at K = 4, 48 at K = 2
    tight = sdy_amd.EddyCovarianceAggregator(_groups(small), torch.from_numpy(small["weights"]).cuda(), max_bytes=need - 1)
    with pytest.raises(ValueError, match=f"need {need} bytes"):
        _feed(tight, windows[:1])
    assert tight._names is None and tight._blocks[0].sums is None and tight._next_start is None
    _feed(sdy_amd.EddyCovarianceAggregator(_groups(small), torch.from_numpy(small["weights"]).cuda(), max_bytes=need), windows[:1])
    # get_logs before two counted times: the initial condition alone, then one counted time
    young = _run(small, eu.cut(small, [1]))
    assert young.n_times == 0 and young._next_start == 1
    for more in ([], eu.cut(small, [1], start=1)):
        _feed(young, more)
        with pytest.raises(ValueError, match="No data recorded"):
            young.get_logs("x")
        with pytest.raises(ValueError, match="No data recorded"):
            young.get_pair_data("low", "u", "v")
    assert young.n_times == 1
    _feed(young, eu.cut(small, [1], start=2))
    assert young.n_times == 2 and list(young.get_logs("")) == eu.log_keys(small["groups"])


def test_two_runs_give_the_same_logs(small):
    windows = eu.cut(small, [6, 7])
    a, b = _run(small, windows).get_logs("x"), _run(small, windows).get_logs("x")
    assert list(a) == list(b) and all(a[k] == b[k] for k in a)


def test_two_ranks_give_the_logs_of_one():
    """Two shares of whole initial conditions (2 + 1 samples) behind a fake process group: one reduce, and the logs of the
    unsharded run within the bound of the weighted sums."""
    whole = eu.seeded_groups(3, 3, 6, 8, 12, GROUPS, seed=455)

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
    r0, r1 = _run(s0, eu.cut(s0, [7, 6]), dist=d0), _run(s1, eu.cut(s1, [7, 6]), dist=d1)
    r1.get_logs("")
    logs = r0.get_logs("")
    assert d0.calls == d1.calls == 1
    st, n = eu.restate_state(whole, eu.cut(whole, [7, 6]))
    stats = {K: eu.restate_stats(blk, whole["weights"], n, 3, 3) for K, blk in st.items()}
    want_raw = eu.per_group(whole, st, {K: v[0] for K, v in stats.items()})
    scales = eu.per_group(whole, st, {K: v[1] for K, v in stats.items()})
    eu.check_logs(logs, eu.logs_from_raw(want_raw, whole["groups"], eu.weight_total(whole)), whole["groups"], scales, "two ranks")


def test_one_pair_function():
    """sdy_amd.eddies.time_covariance of two (time, lat, lon) fields: the aggregator's arithmetic with every time counted."""
    import sdy_amd

    case = eu.seeded_groups(1, 1, 7, 9, 8, {"g": {"x": "x", "y": "y"}}, seed=407)
    x, y = case["target"]["x"][0], case["target"]["y"][0]
    st, n = eu.host_state(case, eu.cut(case, [9]))                           # the eight times after the initial condition
    cov, corr = eu.host_maps(st[2], 0, 0, 1, n)
    out = sdy_amd.eddies.time_covariance(_contiguous(x[1:]), _contiguous(y[1:]))
    assert n == 8 and list(out) == ["cov", "corr", "mean_x", "mean_y"]
    # row 1 of the run's state is the target, the same series
    assert np.array_equal(out["cov"].cpu().numpy(), cov[1]) and np.array_equal(out["corr"].cpu().numpy(), corr[1])
    assert np.allclose(out["mean_x"].cpu().numpy(), x[1:].astype(np.float64).mean(axis=0), rtol=1e-14, atol=0.0)


def test_through_run_inference():
    """InferenceAggregator(eddy_covariances=...) behind run_inference on the tiny synthetic stepper, three windows: the state of
    a bare aggregator fed the same windows, bit for bit, and its logs under <label>/eddy_covariance/; with the option off no
    log key names it and the getter is a KeyError."""
    import sdy_amd
    from sdy_amd import synthetic

    dev = torch.device("cuda", 0)
    n_out, n_forc, nlat, nlon, window, n_windows, members = 4, 2, 32, 64, 6, 3, 2
    exp, _, _ = synthetic.build_sampler(dev, state_chans=n_out, forcing_chans=n_forc, nlat=nlat, nlon=nlon, embed=16, layers=2,
                                        horizon=6, carried_input_only_channel=True)
    stepper, names, out_names = synthetic.build_stepper(exp, n_out, n_forc, carried_input_only_channel=True)
    steps = window * n_windows
    w = sdy_amd.metrics.spherical_area_weights(torch.linspace(-87.0, 87.0, nlat), nlon).cuda()
    spec = {"winds": {"u": out_names[0], "v": out_names[1], "T": out_names[2]}, "pair": {"T": out_names[2], "q": out_names[3]}}

    def groups():
        g = sdy_amd.CovarianceGroups()
        for label, v in spec.items():
            g.add(label, v)
        return g

    class Tee:
        def __init__(self, *aggs):
            self.aggs = aggs

        def record_batch(self, **kw):
            for a in self.aggs:
                a.record_batch(**kw)

    logs = {}
    for on in (False, True):
        agg = sdy_amd.metrics.InferenceAggregator(w, n_timesteps=steps + 1, n_ensemble_members=members,
                                                  eddy_covariances=groups() if on else None)
        alone = sdy_amd.EddyCovarianceAggregator(groups(), w)
        sdy_amd.run_inference(Tee(agg, alone), stepper, synthetic.windows(names, n_windows, window, nlat, nlon, n_ics=2, seed=5),
                              steps, window, n_ensemble_members=members, eval_device=dev)
        logs[on] = agg.get_logs("inference")
        if not on:
            assert not any("eddy_covariance" in k for k in logs[on])
            with pytest.raises(KeyError):
                agg.get_eddy_covariance_data("winds", "u", "v")
    inner = agg._aggregators["eddy_covariance"]
    assert inner.n_times == alone.n_times == steps and inner._names == alone._names
    for bi, ba in zip(inner._blocks, alone._blocks):
        assert torch.equal(bi.sums.view(torch.int64), ba.sums.view(torch.int64))
        assert torch.equal(bi.products.view(torch.int64), ba.products.view(torch.int64))
        assert torch.equal(bi.origins.view(torch.int32), ba.origins.view(torch.int32))
    new = {f"inference/eddy_covariance/{k}" for k in eu.log_keys(spec)}
    assert set(logs[True]) - set(logs[False]) == new and set(logs[False]) <= set(logs[True])
    assert len(new) == (3 + 1) * len(eu.PAIR_KEYS) + 2 * (3 + 2) + 3
    want = alone.get_logs("")
    for k, v in want.items():
        got = logs[True][f"inference/eddy_covariance/{k}"]
        assert type(got) is float and (got == v or (np.isnan(got) and np.isnan(v))), k
    data, want_data = agg.get_eddy_covariance_data("winds", "v", "T"), alone.get_pair_data("winds", "v", "T")
    for m in want_data:
        assert torch.equal(data[m].nan_to_num(nan=-7.0), want_data[m].nan_to_num(nan=-7.0)), m
    assert tuple(data["gen_cov"].shape) == (members, 2, nlat, nlon) and tuple(data["target_cov_zonal"].shape) == (2, nlat)
    assert bool((agg.get_eddy_covariance_data("winds", "u", "u")["gen_cov"] > 0).all())
