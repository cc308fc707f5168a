"""Regional metric series on the device (`sdy_amd.RegionalMeanAggregator`, `sdy_region_series`; csrc/region_series.hip) against
the reference's MeanAggregator run once per region (tests/golden/fx_region_series.npz), the library's _host twin and the
float64 restatement: the shapes at which the kernel takes another path, layouts, batch independence, determinism, one
production plane, the aggregator's bookkeeping and the way through run_inference.  Bounds: tests/region_series_utils.py.  Every
case is a handful of launches."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import region_series_utils as ru

pytestmark = pytest.mark.gpu


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _transposed(x):
    """(members, samples, ...) as the window driver hands it over: a transposed view of a sample-major buffer."""
    buf = _cuda(x).transpose(0, 1).contiguous()
    return buf.transpose(0, 1)


def device_sums(target, gen, weights):
    """One sdy_region_series launch over device tensors {name: tensor}, read in place -> (nvars, R, S, T, 8) numpy."""
    import sdy_amd
    from sdy_amd._lib import SdyRegionSeriesArgs, check, current_stream, ptr
    from sdy_amd.windows import fill_window, window_layouts

    lay = window_layouts(target, gen)
    assert len({l.extents for l in lay}) == 1
    l = lay[0]
    R, HW = weights.shape[0], l.H * l.W
    w = _cuda(weights.reshape(R, HW))
    out = torch.full((len(lay), R, l.n1, l.T, 8), float("nan"), dtype=torch.float64, device="cuda")
    ws_bytes = sdy_amd.lib.sdy_region_series_workspace_bytes(len(lay), R, l.n1, l.T, HW)
    ws = torch.full((ws_bytes // 8,), float("nan"), dtype=torch.float64, device="cuda")
    a = SdyRegionSeriesArgs()
    fill_window(a.win, lay, 0, len(lay))
    a.HW, a.n_regions, a.weights, a.out, a.ws, a.ws_bytes = HW, R, ptr(w), ptr(out), ptr(ws), ws_bytes
    check(sdy_amd.lib.sdy_region_series(C.byref(a), current_stream()), "sdy_region_series")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _dev(target, gen):
    return {k: _cuda(v) for k, v in target.items()}, {k: _cuda(v) for k, v in gen.items()}


@pytest.mark.parametrize("key", ["ens", "det"])
def test_fixture_against_the_reference_and_the_host_twin(key):
    fx = ru.fixture()
    case, ens = fx["cases"][key], key == "ens"
    names, weights = fx["names"], fx["weights"]
    H, W = fx["area"].shape

    def sums_of(target, gen):
        got = device_sums(*_dev(target, gen), weights)
        _, abs_sums, _ = ru.restate_sums(target, gen, names, weights)
        ru.check_sums_reordered(got, ru.host_sums(target, gen, names, weights), abs_sums, H * W, f"{key} device vs host twin")
        return got

    got = ru.series_from_windows(case["windows"], names, fx["regions"], weights, fx["n_timesteps"], ens, sums_of)
    bounds = ru.series_bounds(case["windows"], names, fx["regions"], weights, fx["n_timesteps"], ens, rel=1e-12)
    ru.check_series(got, case["ref64"], bounds, f"{key} device vs ref64")


# grid, members (0: a deterministic 4-D gen), regions: the scalar path with HW % 4 != 0; the 16-byte path below one chunk;
# three chunks per plane, the last one partial, with sixteen regions; the member bound
SHAPES = [((5, 7), 0, 1), ((6, 10), 2, 3), ((40, 72), 5, 16), ((16, 32), 64, 2)]


@pytest.mark.parametrize("grid,M,R", SHAPES, ids=[f"{h}x{w}_m{m}_r{r}" for (h, w), m, r in SHAPES])
def test_seeded_shapes(grid, M, R):
    (H, W), names = grid, ["a", "b"]
    target, gen = ru.seeded_window(M, 2, 3, H, W, names, seed=100 + H)
    weights = ru.seeded_regions(R, H, W, seed=200 + H)
    if R >= 3 and H * W > 2048:
        assert not weights[2].reshape(-1)[:2048].any()                  # zero over the first two chunks
    got = device_sums(*_dev(target, gen), weights)
    want, abs_sums, scales = ru.restate_sums(target, gen, names, weights)
    ru.check_sums_restated(got, want, scales, weights, f"{H}x{W} device vs restatement")
    ru.check_sums_reordered(got, ru.host_sums(target, gen, names, weights), abs_sums, H * W, f"{H}x{W} device vs host twin")
    if M == 0:                                                          # one member, stacked: the same bits as flat rows
        assert np.array_equal(device_sums(_dev(target, gen)[0], {k: _cuda(v[None]) for k, v in gen.items()}, weights), got)


def test_same_bits_in_any_layout_batch_and_run():
    H, W, names = 40, 72, ["a", "b"]
    target, gen = ru.seeded_window(3, 3, 2, H, W, names, seed=7)
    weights = ru.seeded_regions(4, H, W, seed=8)
    t, g = _dev(target, gen)
    base = device_sums(t, g, weights)
    assert np.isfinite(base).all()
    assert np.array_equal(device_sums(t, g, weights), base)                                        # two runs
    gt = {k: _transposed(v) for k, v in gen.items()}
    assert not gt["a"].is_contiguous()
    assert np.array_equal(device_sums(t, gt, weights), base)                                       # the window driver's view
    for j, k in enumerate(names):                                                                  # one launch per variable
        assert np.array_equal(device_sums({k: t[k]}, {k: g[k]}, weights)[0], base[j])
    alone = device_sums({k: v[1:2] for k, v in t.items()}, {k: v[:, 1:2] for k, v in g.items()}, weights)
    assert np.array_equal(alone[:, :, 0], base[:, :, 1])                                           # a sample alone
    # the scalar path (a view 4 bytes off a 16-byte boundary) adds the same terms in the same order
    off = {}
    for k, v in g.items():
        buf = torch.zeros(v.numel() + 1, device="cuda")
        buf[1:] = v.reshape(-1)
        off[k] = buf[1:].view(v.shape)
        assert off[k].data_ptr() % 16 == 4
    assert np.array_equal(device_sums(t, off, weights), base)
    # fewer regions: a region's sums do not depend on the others
    assert np.array_equal(device_sums(t, g, weights[[2]])[:, 0], base[:, 2])


def test_nan_and_the_zero_weight_rule_on_the_device():
    H, W, names = 40, 72, ["a"]
    target, gen = ru.seeded_window(2, 1, 2, H, W, names, seed=17)
    weights = ru.seeded_regions(4, H, W, seed=18)
    base = device_sums(*_dev(target, gen), weights)
    outside = weights[2] == 0.0
    t2, g2 = {"a": target["a"].copy()}, {"a": gen["a"].copy()}
    t2["a"][..., outside] = np.nan
    g2["a"][..., outside] = np.inf
    dirty = device_sums(*_dev(t2, g2), weights)
    assert np.array_equal(dirty[:, 2], base[:, 2]) and np.isnan(dirty[:, 0]).all()
    g3 = {"a": gen["a"].copy()}
    row, col = np.argwhere(weights[2] > 0)[5]
    g3["a"][1, 0, 1, row, col] = np.nan
    hit = device_sums(*_dev(target, g3), weights)
    assert np.isnan(hit[0, 2, 0, 1, :6]).all() and np.array_equal(hit[0, 2, 0, 1, 6:], base[0, 2, 0, 1, 6:])
    assert np.array_equal(hit[0, :, 0, 0], base[0, :, 0, 0]) and np.array_equal(hit[0, 1], base[0, 1])


def test_production_plane_with_the_standard_regions():
    import sdy_amd

    H, W = 180, 360
    lats = -90.0 + (np.arange(H) + 0.5)
    lons = np.arange(W) + 0.5
    regions = sdy_amd.Regions.standard(lats, lons, sdy_amd.metrics.spherical_area_weights(lats, W))
    weights = regions.stacked()
    target, gen = ru.seeded_window(3, 1, 2, H, W, ["a"], seed=33)
    got = device_sums(*_dev(target, gen), weights)
    want, _, scales = ru.restate_sums(target, gen, ["a"], weights)
    ru.check_sums_restated(got, want, scales, weights, "180x360 device vs restatement")


@pytest.mark.parametrize("key", ["ens", "det"])
def test_aggregator_over_three_windows(key):
    """RegionalMeanAggregator with i_time_start against the fixture's series, and its global region against MeanAggregator
    on the same windows (rtol 1e-6: the fp32 and the float64 per-point chains differ, both sum in float64)."""
    import sdy_amd

    fx = ru.fixture()
    case, ens = fx["cases"][key], key == "ens"
    d = fx["definitions"]
    cell = np.zeros(fx["area"].shape, bool)
    cell[tuple(d["cell"])] = True
    regions = sdy_amd.Regions(fx["lats"], fx["lons"], fx["area"]).add_global().add_lat_band("band", *d["band"])
    regions.add_box("wrap_box", lat=d["wrap_box"]["lat"], lon=d["wrap_box"]["lon"])
    regions.add_fraction("fraction", fx["fraction"]).add_fraction("cell", cell)
    assert np.array_equal(regions.stacked(), fx["weights"])
    agg = sdy_amd.RegionalMeanAggregator(regions, n_timesteps=fx["n_timesteps"], is_ensemble=ens)
    glob = sdy_amd.metrics.MeanAggregator(_cuda(fx["weights"][0]), n_timesteps=fx["n_timesteps"], is_ensemble=ens)
    for i, (start, target, gen) in enumerate(case["windows"]):
        t, g = _dev(target, gen)
        if ens and i == 1:
            g = {k: _transposed(v) for k, v in gen.items()}
        agg.record_batch(0.0, t, g, None, None, i_time_start=start)
        glob.record_batch(0.0, t, g, t, g, i_time_start=start)
    series = agg.get_series()
    assert agg.metric_names == list(ru.METRICS + (ru.METRICS_ENSEMBLE if ens else ()))
    assert list(series) == [f"{m}/{r}/{v}" for m in agg.metric_names for r in fx["regions"] for v in fx["names"]]
    got = {k: v.cpu().numpy() for k, v in series.items()}
    assert all(v.shape == (fx["n_timesteps"],) and v.dtype == np.float64 for v in got.values())
    bounds = ru.series_bounds(case["windows"], fx["names"], fx["regions"], fx["weights"], fx["n_timesteps"], ens, rel=1e-12)
    ru.check_series(got, case["ref64"], bounds, f"{key} aggregator vs ref64")
    for k, v in glob.get_series().items():
        metric, var = k.split("/")
        np.testing.assert_allclose(got[f"{metric}/global/{var}"], v.cpu().numpy(), rtol=1e-6, atol=0.0, err_msg=k)
    logs = agg.get_logs("mean_regional")
    assert list(logs) == ["mean_regional/series"] and list(logs["mean_regional/series"]) == list(series)
    assert all(np.array_equal(logs["mean_regional/series"][k], got[k]) for k in got)
    # a second window at the same times: the series are the mean of the two
    start, target, gen = case["windows"][2]
    t, g = _dev(target, gen)
    agg.record_batch(0.0, t, g, None, None, i_time_start=start)
    again = {k: v.cpu().numpy() for k, v in agg.get_series().items()}
    assert all(np.allclose(again[k], got[k], rtol=1e-14, atol=0.0) for k in got)
    with pytest.raises(ValueError, match="variables"):
        agg.record_batch(0.0, {"a": t["a"]}, {"a": g["a"]}, None, None, i_time_start=start)


class _Recorder:
    """Hands every window on and keeps a copy of what it saw."""

    accepts_sample_weights = True

    def __init__(self, inner):
        self.inner, self.windows = inner, []

    def record_batch(self, loss, target_data, gen_data, target_data_norm, gen_data_norm, i_time_start=0, **kw):
        self.windows.append((i_time_start, {k: v.cpu().numpy() for k, v in target_data.items()},
                             {k: v.cpu().numpy() for k, v in gen_data.items()}))
        self.inner.record_batch(loss=loss, target_data=target_data, gen_data=gen_data, target_data_norm=target_data_norm,
                                gen_data_norm=gen_data_norm, i_time_start=i_time_start, **kw)


def test_through_run_inference():
    """run_inference on the tiny loop fixture (2 windows x 6 steps, 2 samples, 3 members) with InferenceAggregator(regions=...):
    the regional series of the (denormalised) windows the run produced, under <label>/mean_regional/..., and without
    `regions` exactly the parent's keys."""
    import sdy_amd
    from test_gpu_derived import _loop_setup

    _, stepper, windows, sigma, n_total, n_mem, names = _loop_setup(3)
    lats = torch.linspace(-87.0, 87.0, 32)
    lons = np.arange(64) * 360.0 / 64
    w = sdy_amd.metrics.spherical_area_weights(lats, 64)
    regions = sdy_amd.Regions.standard(lats, lons, w)
    logs, rec, agg = {}, None, None
    for on in (False, True):
        agg = sdy_amd.metrics.InferenceAggregator(w.cuda(), n_timesteps=n_total + 1, n_ensemble_members=3,
                                                  regions=regions if on else None)
        rec = _Recorder(agg)
        sdy_amd.run_inference(rec, stepper, types.SimpleNamespace(loader=windows), n_total, n_mem, 3)
        logs[on] = agg.get_logs("inference")
    assert set(logs[True]) - set(logs[False]) == {"inference/mean_regional/series"}
    parent = {"inference/mean/series", "inference/mean_norm/series"}
    assert parent <= set(logs[False]) and not any("regional" in k for k in logs[False])
    out = names["out_names"]
    table = logs[True]["inference/mean_regional/series"]
    metrics = ru.METRICS + ru.METRICS_ENSEMBLE
    want_keys = sorted(f"{m}/{r}/{v}" for m in metrics for r in regions.names for v in out)
    assert table.columns == ["forecast_step"] + want_keys and len(table.data) == n_total + 1
    rows = agg.get_inference_logs("inference")
    assert all(f"inference/mean_regional/{k}" in rows[0] for k in want_keys)
    series = agg.get_regional_series()
    assert sorted(series) == want_keys
    got = {k: v.cpu().numpy() for k, v in series.items()}
    weights = regions.stacked()
    bounds = ru.series_bounds(rec.windows, out, regions.names, weights, n_total + 1, True, rel=1e-12)
    want = ru.series_from_windows(rec.windows, out, regions.names, weights, n_total + 1, True,
                                  lambda t, g: ru.restate_sums(t, g, out, weights)[0])
    # (time 0 is the initial condition: members and target coincide there, rmse = 0 and ssr = 0 / 0)
    for k in want_keys:
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
    finite = {k: np.nan_to_num(v) for k, v in want.items()}
    ru.check_series({k: np.nan_to_num(v) for k, v in got.items()}, finite,
                    {k: np.where(np.isfinite(b), b, 1.0) for k, b in bounds.items()}, "run_inference vs restatement")
    for j, k in enumerate(want_keys):
        assert np.array_equal(np.asarray([row[1 + j] for row in table.data], np.float64), got[k], equal_nan=True)
