"""Wavenumber-frequency spectra on the device: sdy_spacetime_append / sdy_spacetime_segment_power against their host twins bit
for bit, `SpaceTimeSpectrumAggregator` under window cuts against itself (bits) and against the numpy restatement (tolerance),
the production grid, and the other entry points.  Data, restatement and tolerance: tests/spacetime_utils.py.  Every test is a
handful of launches."""
import ctypes as C

import numpy as np
import pytest
import torch

import spacetime_utils as su

pytestmark = pytest.mark.gpu

RUN = 41                                   # times of the run of the aggregator tests: the initial condition and 40 counted
CUTS = ((41,), (1, 40), (5, 7, 29), (1,) * 41)
GRID = (9, 10)                             # of the aggregator tests: an equator row, scalar loads
M, B = 3, 2
BANDS = {"mjo_east": ("symmetric", 1, 3, 1.0, 3.0), "mjo_west": ("symmetric", -3, -1, 1.0, 3.0),
         "anti": ("antisymmetric", -2, 2, 0.5, 1.5), "empty": ("symmetric", 1, 2, 100.0, 200.0)}


def _contiguous(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _transposed(x):
    """(members, samples, ...) as the window driver hands it over: a transposed view of a sample-major buffer."""
    buf = _contiguous(x).transpose(0, 1).contiguous()
    view = buf.transpose(0, 1)
    assert not view.is_contiguous() or min(x.shape[:2]) == 1
    return view


def _off_16_bytes(x):
    """The same values in a buffer that starts 4 bytes past a 16-byte boundary."""
    flat = torch.empty(x.size + 1, dtype=torch.float32, device="cuda")
    view = flat[1:].view(x.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    assert view.data_ptr() % 16 == 4
    return view


def _device_coef(gen, target, lats, K, N, t0, t1, n_first, layout=_contiguous):
    """One append on the device into a ring filled with 7 -> (n_traj, N, R, 2, K + 1, 2) numpy."""
    import sdy_amd
    from sdy_amd import _lib
    from sdy_amd.windows import fill_window, window_layouts

    Mm, Bb, T, H, W = gen.shape
    north, south = su.band(lats, su.LAT_MAX)
    coef = torch.full((Mm * Bb + Bb, N, len(north), 2, K + 1, 2), 7.0, dtype=torch.float64, device="cuda")
    table = torch.from_numpy(su.circle(W)).cuda()
    lay = window_layouts({"x": _contiguous(target)}, {"x": layout(gen)})
    a = _lib.SdySpacetimeAppendArgs()
    fill_window(a.win, lay, 0, 1)
    a.H, a.W, a.R, a.K = H, W, len(north), K
    for p in range(len(north)):
        a.north[p], a.south[p] = north[p], south[p]
    a.lon_table, a.t0, a.t1, a.n_first, a.N, a.coef = table.data_ptr(), t0, t1, n_first, N, coef.data_ptr()
    _lib.check(sdy_amd.lib.sdy_spacetime_append(C.byref(a), _lib.current_stream()))
    return coef.cpu().numpy()


def _host_coef(gen, target, lats, K, N, t0, t1, n_first):
    import sdy_amd

    Mm, Bb, T, H, W = gen.shape
    north, south = su.band(lats, su.LAT_MAX)
    coef = np.full((Mm * Bb + Bb, N, len(north), 2, K + 1, 2), 7.0)
    a, keep = su.append_args(coef, np.ascontiguousarray(target), np.ascontiguousarray(gen), north, south, K, N, t0, t1, n_first,
                             su.circle(W))
    assert sdy_amd.lib.sdy_spacetime_append_host(C.byref(a)) == 0
    return coef


def _power_both(coef, Mm, Bb, N, R, K, first_slot, detrend, p, calls=1):
    """`calls` segment launches on the same accumulators, on the device and by the host twin -> (device acc, host acc)."""
    import sdy_amd
    from sdy_amd import _lib

    w, table = su.taper(N, p), su.circle(N)
    host = np.zeros((2, Bb, 2, N, K + 1))
    a, keep = su.power_args(coef, Mm, Bb, N, R, K, first_slot, detrend, w, table, host)
    for _ in range(calls):
        assert sdy_amd.lib.sdy_spacetime_segment_power_host(C.byref(a)) == 0
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in (("coef", coef), ("w", w), ("table", table))}
    acc = torch.zeros(host.shape, dtype=torch.float64, device="cuda")
    ws_bytes = sdy_amd.lib.sdy_spacetime_workspace_bytes(1, Mm, Bb, N, R, K)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device="cuda")
    a = _lib.SdySpacetimeSegmentPowerArgs()
    a.coef, a.nvars, a.M, a.B, a.N, a.R, a.K = dev["coef"].data_ptr(), 1, Mm, Bb, N, R, K
    a.first_slot, a.detrend = first_slot, su.DETREND_CODE[detrend]
    a.taper, a.time_table, a.acc = dev["w"].data_ptr(), dev["table"].data_ptr(), acc.data_ptr()
    a.ws, a.ws_bytes = ws.data_ptr(), ws_bytes
    for _ in range(calls):
        _lib.check(sdy_amd.lib.sdy_spacetime_segment_power(C.byref(a), _lib.current_stream()))
    return acc.cpu().numpy(), host


# ---- device against host twin ------------------------------------------------------------------------------------------------
def test_smallest_case_first():
    """One member, one sample, one pair, the scalar path, one segment of 4 times: the first launches of the file."""
    H, W, N, K = 6, 18, 4, 2
    gen, target = su.make_data(1, 1, N, H, W)
    lats = su.lats_of(H)
    coef = _device_coef(gen, target, lats, K, N, 0, N, 0)
    assert su.same_bits(coef, _host_coef(gen, target, lats, K, N, 0, N, 0))
    acc, host = _power_both(coef, 1, 1, N, 1, K, 0, "linear", 0.2)
    assert su.same_bits(acc, host) and np.isfinite(acc).all()


@pytest.mark.parametrize("grid", su.GRIDS)
@pytest.mark.parametrize("members", su.MEMBERS)
def test_append_equals_host_twin(grid, members):
    H, W = grid
    lats, K, N = su.lats_of(H), su.k_of(W), 8
    gen, target = su.make_data(members, su.SAMPLES, 7, H, W)
    # window times 2 .. 6 as counted times 13 .. 17: slots 5, 6, 7, 0, 1 (the ring wraps); the other slots stay as they were
    twin = _host_coef(gen, target, lats, K, N, 2, 7, 13)
    assert (twin[:, 2:5] == 7.0).all() and (twin[:, [5, 6, 7, 0, 1]] != 7.0).any()
    for layout in (_contiguous, _transposed, _off_16_bytes):      # 16-byte loads (W = 16), the transposed view, scalar loads
        assert su.same_bits(_device_coef(gen, target, lats, K, N, 2, 7, 13, layout), twin), layout.__name__
    c = su.lon_coefficients(gen[:, :, 2:7], *su.band(lats, su.LAT_MAX), K)          # (M, B, 5, R, 2, K1)
    got = twin[:members * su.SAMPLES][:, [5, 6, 7, 0, 1]].reshape(members, su.SAMPLES, 5, -1, 2, K + 1, 2)
    assert np.abs(got[..., 0] + 1j * got[..., 1] - c).max() <= 1e-12 * np.abs(gen).max()


@pytest.mark.parametrize("N,K,R,members,first_slot", [
    (8, 5, 2, 3, 3),           # one tile of 6 columns: a group of 4 and a group of 2
    (12, 9, 3, 1, 7),          # tiles of 8 and 2 columns
    (300, 6, 1, 1, 123),       # more frequencies than threads; tiles of 6 and 1 columns
    (1024, 2, 1, 1, 1000),     # the longest segment: tiles of 2 and 1 columns
])
def test_segment_power_equals_host_twin(N, K, R, members, first_slot):
    rng = np.random.default_rng(N)
    samples = 2 if N < 100 else 1
    coef = rng.standard_normal((members * samples + samples, N, R, 2, K + 1, 2)) + 0.01 * np.arange(N).reshape(1, N, 1, 1, 1, 1)
    for detrend, p in (("linear", 0.2), ("none", 0.0), ("mean", 1.0)) if N < 100 else (("linear", 0.2),):
        acc, host = _power_both(coef, members, samples, N, R, K, first_slot, detrend, p, calls=2 if N < 100 else 1)
        assert su.same_bits(acc, host) and np.isfinite(acc).all() and acc.max() > 0.0, (detrend, p)
    # against the restatement: the columns in time order
    z = np.roll(coef[..., 0] + 1j * coef[..., 1], -first_slot, axis=1)
    P = su.segment_power(np.moveaxis(z, 1, 0), "linear", su.taper(N, 0.2))           # (N, n_traj, R, 2, K1)
    acc, _ = _power_both(coef, members, samples, N, R, K, first_slot, "linear", 0.2)
    gen = P[:, :members * samples].reshape(N, members, samples, R, 2, K + 1).sum(axis=(1, 3)).transpose(1, 2, 0, 3)
    tgt = P[:, members * samples:].sum(axis=2).transpose(1, 2, 0, 3)
    A = np.abs(coef).max()
    w = su.taper(N, 0.2)
    tol = 1e-12 * 25.0 * A ** 2 * w.sum() ** 2 / (N * (w * w).sum()) * members * R
    assert np.abs(acc[0] - gen).max() <= tol and np.abs(acc[1] - tgt).max() <= tol


def test_a_non_finite_value_makes_its_cells_nan():
    H, W, N, K = 8, 16, 8, 5
    lats = su.lats_of(H)
    gen, target = su.make_data(2, 2, N, H, W)
    gen[1, 0, 3, 3, 7] = np.nan
    coef = _device_coef(gen, target, lats, K, N, 0, N, 0)
    assert su.same_bits(coef, _host_coef(gen, target, lats, K, N, 0, N, 0))
    acc, host = _power_both(coef, 2, 2, N, 2, K, 0, "linear", 0.2)
    assert su.same_bits(acc, host)
    assert np.isnan(acc[0, 0]).all() and np.isfinite(acc[0, 1]).all() and np.isfinite(acc[1]).all()


# ---- the aggregator ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run():
    """{name: (gen (3, 2, 41, 9, 10), target (2, 41, 9, 10))}: time 0 is the initial condition."""
    return {k: su.make_data(M, B, RUN, *GRID, seed=i) for i, k in enumerate(su.NAMES)}


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


def _spec(N=12, hop=5, detrend="linear", taper=0.2, names=su.NAMES, **kw):
    import sdy_amd

    return sdy_amd.SpaceTimeSpectra(su.lats_of(GRID[0]), list(names), N, hop=hop, lat_max=su.LAT_MAX, detrend=detrend, taper=taper,
                                    bands=BANDS, **kw)


def _agg(**kw):
    import sdy_amd

    return sdy_amd.SpaceTimeSpectrumAggregator(_spec(**kw))


def _numpy(data):
    return {k: v.cpu().numpy() for k, v in data.items()}


@pytest.mark.parametrize("N,hop,detrend,taper", [(12, 5, "linear", 0.2), (8, 8, "none", 0.0), (9, 4, "mean", 1.0)])
def test_window_cuts_give_equal_bits_and_the_restatement_is_met(run, N, hop, detrend, taper):
    lats, K = su.lats_of(GRID[0]), GRID[1] // 2
    first = None
    for cuts in CUTS:
        agg = _feed(_agg(N=N, hop=hop, detrend=detrend, taper=taper), _windows(run, cuts))
        assert (agg.n_times, agg.n_segments) == (40, (40 - N) // hop + 1)
        data = _numpy(agg.get_data())
        if first is None:
            first = data
            continue
        assert list(data) == list(first)
        for k in data:
            assert su.same_bits(data[k], first[k]), (cuts, k)
    assert list(first) == ["gen/a", "target/a", "gen/b", "target/b", "frequency", "wavenumber", "n_segments"]
    assert first["n_segments"] == (40 - N) // hop + 1 and np.array_equal(first["wavenumber"], np.arange(-K, K + 1))
    assert np.array_equal(first["frequency"], np.arange(N // 2 + 1) / (N * 0.25))
    for name, (gen, target) in run.items():
        want = su.want(gen[:, :, 1:], target[:, 1:], lats, N, hop, K, su.LAT_MAX, detrend, taper)
        tol = su.tolerance(gen[:, :, 1:], target[:, 1:], lats, N, su.LAT_MAX, taper)
        for side in ("gen", "target"):
            got = first[f"{side}/{name}"]
            assert got.shape == (B, 2, N // 2 + 1, 2 * K + 1) and got.dtype == np.float64
            err = np.abs(got - want[side]).max()
            assert err <= tol, (name, side, err, tol)
            assert got.max() > 1e3 * tol                                                 # (the comparison says something)


def test_windows_in_run_order_and_nothing_before_a_segment(run):
    windows = _windows(run, (5, 7, 29))
    agg = _feed(_agg(), windows[:1])
    for read in (agg.get_data, lambda: agg.get_logs("x")):
        with pytest.raises(ValueError, match="No data recorded: no segment of 12 counted times is complete .4 counted."):
            read()
    before = (agg.n_times, agg.n_segments, agg._next_start, agg._acc["coef"].clone(), agg._acc["acc"].clone())
    with pytest.raises(ValueError, match="SpaceTimeSpectrumAggregator: a window that starts at time 12, where the one before "
                                         "ended at 5: the segments need every window of a run, in order"):
        _feed(agg, windows[2:])
    with pytest.raises(ValueError, match="starts at time 0, where the one before ended at 5"):
        _feed(agg, windows[:1])
    start, target, gen = windows[1]
    with pytest.raises(ValueError, match="member count, sample count or grids of a window differ"):
        agg.record_batch(0.0, {k: _contiguous(v) for k, v in target.items()}, {k: _contiguous(v[:2]) for k, v in gen.items()},
                         i_time_start=start)
    assert (agg.n_times, agg.n_segments, agg._next_start) == before[:3]                # a refused window changes nothing
    assert torch.equal(agg._acc["coef"], before[3]) and torch.equal(agg._acc["acc"], before[4])
    _feed(agg, windows[1:])
    whole = _feed(_agg(), _windows(run, (41,)))
    for k, v in _numpy(agg.get_data()).items():
        assert su.same_bits(v, whole.get_data()[k].cpu().numpy()), k


def test_band_logs_are_sums_of_the_data(run):
    import sdy_amd

    agg = _feed(_agg(), _windows(run, (5, 7, 29)))
    data, logs = _numpy(agg.get_data()), agg.get_logs("st")
    spec = agg._spec
    K = GRID[1] // 2
    want_keys = []
    for name in su.NAMES:
        want_keys += [f"st/{m}/{b}/{name}" for b in BANDS for m in ("power_gen", "power_target", "power_ratio")]
        want_keys += [f"st/east_west_ratio_gen/{name}", f"st/east_west_ratio_target/{name}"]
    assert list(logs) == want_keys and all(isinstance(v, float) for v in logs.values())
    period = 1.0 / data["frequency"][1:]
    for name in su.NAMES:
        power = {}
        for b, (comp, k_min, k_max, p_min, p_max) in BANDS.items():
            rows = np.concatenate([[False], (period >= p_min) & (period <= p_max)])
            cols = (data["wavenumber"] >= k_min) & (data["wavenumber"] <= k_max)
            assert np.array_equal(spec.band_mask(b, K).numpy(), rows[:, None] & cols[None, :])
            for side in ("gen", "target"):
                cells = data[f"{side}/{name}"][:, sdy_amd.spacetime.COMPONENTS.index(comp)][:, rows][:, :, cols]
                got = logs[f"st/power_{side}/{b}/{name}"]
                if cells.size == 0:
                    assert b == "empty" and np.isnan(got) and np.isnan(logs[f"st/power_ratio/{b}/{name}"])
                    continue
                want = cells.sum() / B
                # a torch float64 sum of a few dozen non-negative cells against numpy's: 1e-12 relative, the project's constant
                assert abs(got - want) <= 1e-12 * want and want > 0.0, (b, side)
                power[b, side] = got
            if b != "empty":
                assert logs[f"st/power_ratio/{b}/{name}"] == power[b, "gen"] / power[b, "target"]
        for side in ("gen", "target"):
            assert logs[f"st/east_west_ratio_{side}/{name}"] == power["mjo_east", side] / power["mjo_west", side]
    # the data hold an eastward wave of wavenumber 2 and period 6 steps = 1.5 days: east beats west
    assert logs["st/east_west_ratio_target/a"] > 2.0


def test_one_field_function_equals_the_aggregator(run):
    import sdy_amd

    gen, target = run["b"]
    agg = _feed(_agg(names=("b",)), _windows({"b": run["b"]}, (41,)))
    data = _numpy(agg.get_data())
    lats = su.lats_of(GRID[0])
    for x, want in ((target[1, 1:], data["target/b"][1]),):
        out = sdy_amd.spacetime.space_time_spectrum(_contiguous(x), lats, 12, hop=5, lat_max=su.LAT_MAX)
        assert list(out) == ["power", "frequency", "wavenumber", "n_segments"]
        assert su.same_bits(out["power"].cpu().numpy(), want) and float(out["n_segments"]) == 6.0
        assert su.same_bits(out["frequency"].cpu().numpy(), data["frequency"])
    # one member: gen pooled over its single member is that member's own spectrum
    one = sdy_amd.spacetime.space_time_spectrum(_contiguous(gen[0, 0, 1:]), lats, 12, hop=5, lat_max=su.LAT_MAX)
    alone = _feed(_agg(names=("b",)), _windows({"b": (gen[:1], target)}, (41,)))
    assert su.same_bits(one["power"].cpu().numpy(), alone.get_data()["gen/b"][0].cpu().numpy())


def test_through_inference_aggregator():
    """On 9 x 12: the time means of the default set take 16-byte loads of whole planes only."""
    import sdy_amd

    H, W = 9, 12
    run = {k: su.make_data(M, B, RUN, H, W, seed=i) for i, k in enumerate(su.NAMES)}
    spec = sdy_amd.SpaceTimeSpectra(su.lats_of(H), ["b"], 12, hop=5, lat_max=su.LAT_MAX, bands=BANDS)
    w = sdy_amd.metrics.spherical_area_weights(torch.from_numpy(su.lats_of(H)).float(), W).cuda()
    kw = dict(n_timesteps=RUN, n_ensemble_members=M)
    on = sdy_amd.metrics.InferenceAggregator(w, space_time_spectra=spec, **kw)
    off = sdy_amd.metrics.InferenceAggregator(w, **kw)
    for start, target, gen in _windows(run, (5, 7, 29)):
        t, g = {k: _contiguous(v) for k, v in target.items()}, {k: _transposed(v) for k, v in gen.items()}
        for agg in (on, off):
            agg.record_batch(0.0, t, g, t, g, i_time_start=start)
    alone = _feed(sdy_amd.SpaceTimeSpectrumAggregator(spec), _windows(run, (41,)))
    data = on.get_space_time_spectrum_data()
    for k, v in alone.get_data().items():
        assert su.same_bits(data[k].cpu().numpy(), v.cpu().numpy()), k
    want = su.want(run["b"][0][:, :, 1:], run["b"][1][:, 1:], su.lats_of(H), 12, 5, W // 2, su.LAT_MAX, "linear", 0.2)
    tol = su.tolerance(run["b"][0][:, :, 1:], run["b"][1][:, 1:], su.lats_of(H), 12, su.LAT_MAX, 0.2)
    assert np.abs(data["gen/b"].cpu().numpy() - want["gen"]).max() <= tol
    logs_on, logs_off = on.get_logs("inference"), off.get_logs("inference")
    new = [f"inference/space_time_spectra/{k}" for k in alone.get_logs("")]
    assert len(new) == 3 * len(BANDS) + 2
    assert [k for k in logs_on if k not in logs_off] == new and list(logs_on)[:len(logs_off)] == list(logs_off)
    assert all(isinstance(logs_on[k], float) for k in new)


def test_production_grid_against_restatement():
    """180 x 360 with the default band (30 rows, 15 pairs), K = 32 by default, N = 16, hop = 8: 2 members, 1 sample, one
    variable, 24 counted times (2 segments), held against the restatement."""
    import sdy_amd

    H, W, N, hop = 180, 360, 16, 8
    lats = su.lats_of(H)
    gen, target = su.make_data(2, 1, 25, H, W)
    spec = sdy_amd.SpaceTimeSpectra(lats, ["pr"], N, hop=hop)
    assert spec.n_pairs == 15 and sorted(spec.north + spec.south) == list(range(75, 105))
    agg = sdy_amd.SpaceTimeSpectrumAggregator(spec)
    for start, T in ((0, 12), (12, 13)):
        agg.record_batch(0.0, {"pr": _contiguous(target[:, start:start + T])}, {"pr": _transposed(gen[:, :, start:start + T])},
                         i_time_start=start)
    assert (agg.n_times, agg.n_segments, agg._K) == (24, 2, 32)
    data = _numpy(agg.get_data())
    want = su.want(gen[:, :, 1:], target[:, 1:], lats, N, hop, 32, 15.0, "linear", 0.2)
    tol = su.tolerance(gen[:, :, 1:], target[:, 1:], lats, N, 15.0, 0.2)
    for side in ("gen", "target"):
        got = data[f"{side}/pr"]
        assert got.shape == (1, 2, 9, 65)
        err = np.abs(got - want[side]).max()
        assert err <= tol and got.max() > 1e3 * tol, (side, err, tol)
