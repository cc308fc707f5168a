"""Spell-duration statistics on the device: sdy_event_spell_accumulate against its host twin and the numpy restatement bit
for bit -- layouts, window cuts, runs, batches -- the known answer, the member-hit totals of the event tables, the production
grid, refusals, the one-field function, and the way through InferenceAggregator and run_inference.  Cases and comparisons:
tests/spell_utils.py.  Every test is a handful of launches."""
import types

import numpy as np
import pytest
import torch

import spell_utils as su

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return su.cases()


@pytest.fixture(scope="module")
def wanted(cases):
    """The restatement of every small case, computed once: {name: (states, closed durations)}."""
    return {name: su.restate(case) for name, case in cases.items()}


def _contiguous(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _transposed(x):
    """(members, samples, ...) as the window driver hands it over: a transposed view of a sample-major buffer."""
    if x.ndim != 5:
        return _contiguous(x)
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


def _run(case, layout=_contiguous, windows=None, target_layout=_contiguous, **kw):
    import sdy_amd

    agg = sdy_amd.EventSpellAggregator(su.make_events(case), torch.from_numpy(case["weights"]).cuda(),
                                       n_timesteps=case["n_timesteps"], **kw)
    for start, target, gen in (case["windows"] if windows is None else windows):
        agg.record_batch(0.0, {k: target_layout(v) for k, v in target.items()}, {k: layout(v) for k, v in gen.items()},
                         i_time_start=start)
    return agg


def _bits(agg, case):
    """-> (states {var: (E, 4, rows, H, W) uint32}, closed durations {var: (E, 2, H, 16) float64}) as numpy."""
    assert agg._acc["state"].dtype == torch.float64 and agg._acc["durations"].dtype == torch.float64
    states, closed = {}, {}
    for i, k in enumerate(su.event_names(case)):
        states[k] = agg._state(i).cpu().numpy().view(np.uint32)
        closed[k] = agg._durations(i).cpu().numpy()
    return states, closed


def _same_data(got, want):
    assert list(got) == list(want)
    for key, v in want.items():
        g = got[key]
        assert g.dtype == torch.float64 and g.is_cuda and tuple(g.shape) == v.shape, key
        assert np.array_equal(g.cpu().numpy(), v, equal_nan=True), key


def test_smallest_case_first(cases, wanted):
    """One variable, one event, one window of the smallest case: the first launch of the file."""
    case = dict(cases["m5_b2_6x8"])
    case["names"], case["events"] = ["b"], {"b": cases["m5_b2_6x8"]["events"]["b"]}
    windows = [(s, {"b": t["b"]}, {"b": g["b"]}) for s, t, g in case["windows"][:1]]
    got = _bits(_run(case, windows=windows), case)
    want = su.restate(case, windows)
    assert su.same(got[0], want[0]) and su.same(got[1], want[1])


@pytest.mark.parametrize("name", su.SMALL)
def test_device_equals_host_equals_restatement(cases, wanted, name):
    case = cases[name]
    agg = _run(case)
    got, twin, want = _bits(agg, case), su.host(case), wanted[name]
    assert su.same(got[0], twin[0]) and su.same(got[0], want[0])
    assert su.same(got[1], twin[1]) and su.same(got[1], want[1])
    assert agg.n_times == 23
    want_data = su.readout(case, *want)
    _same_data(agg.get_data(), want_data)
    want_logs, bounds = su.restate_logs(case, want_data, 23)
    su.close_logs(agg.get_logs(""), want_logs, bounds, name)
    assert list(agg.get_logs("sp")) == [f"sp/{k}" for k in want_logs]


def test_known_answer_on_the_device(cases):
    case = cases["known_m5_b2_6x8"]
    agg = _run(case)
    data = agg.get_data()
    for k in ("a", "b"):
        assert (data[f"gen_longest/on/{k}"] == 20).all() and (data[f"gen_spells/on/{k}"] == 2).all()
        assert (data[f"gen_hits/on/{k}"] == 22).all() and (data[f"target_longest/on/{k}"] == 3).all()
        assert (data[f"target_spells/on/{k}"] == 3).all() and (data[f"target_hits/on/{k}"] == 5).all()
        want = np.zeros((2, 6, 16))
        want[0, :, 5], want[0, :, 1] = 80, 80              # 20 times -> the bin of 17..32; open at the end: 2 times
        want[1, :, 0], want[1, :, 2] = 32, 16              # 1 time, closed and open; 3 times
        assert np.array_equal(data[f"durations_gen/on/{k}"].cpu().numpy(), want[0])
        assert np.array_equal(data[f"durations_target/on/{k}"].cpu().numpy(), want[1])
        assert data[f"duration_edges/on/{k}"].tolist() == su.EDGES.tolist()
    logs = agg.get_logs("")
    assert logs["mean_duration_gen/on/a"] == pytest.approx(11.0) and logs["longest_bias/on/b"] == pytest.approx(17.0)


@pytest.mark.parametrize("name", ["m5_b2_6x8", "m25_b1_4x360", "nan_m5_b2_6x8", "e8_m5_b1_6x8"])
def test_layouts_give_the_same_bits(cases, wanted, name):
    """Contiguous, the transposed view of a (samples, members, ...) buffer, and views one element into a larger buffer (scalar
    loads), for gen and for target: integers, so identical."""
    case = cases[name]
    for layout, target_layout in ((_transposed, _contiguous), (_offset, _contiguous), (_contiguous, _offset)):
        got = _bits(_run(case, layout, target_layout=target_layout), case)
        assert su.same(got[0], wanted[name][0]) and su.same(got[1], wanted[name][1]), (layout.__name__, target_layout.__name__)


@pytest.mark.parametrize("name", ["m5_b2_6x8", "nan_m5_b2_6x8"])
def test_window_cuts_give_the_same_bits(cases, wanted, name):
    case = cases[name]
    for cuts in (((0, su.N_TIMES),), tuple((t, t + 1) for t in range(su.N_TIMES)), ((0, 1), (1, 9), (9, 24))):
        agg = _run(case, windows=su.recut(case, cuts))
        got = _bits(agg, case)
        assert su.same(got[0], wanted[name][0]) and su.same(got[1], wanted[name][1]), cuts
        assert agg.n_times == 23


def test_two_runs_give_the_same_bits(cases):
    case = cases["m25_b1_4x360"]
    a, b = _run(case), _run(case)
    assert all(torch.equal(a._acc[s], b._acc[s]) for s in ("state", "durations")) and a.get_logs("x") == b.get_logs("x")


def test_a_sample_alone_and_in_a_batch(cases, wanted):
    """Batch independence: the state of sample 0's trajectories is the same alone and in the batch of 2."""
    case = cases["m5_b2_6x8"]
    one = dict(case, B=1)
    windows = [(s, {k: v[:1] for k, v in t.items()}, {k: v[:, :1] for k, v in g.items()}) for s, t, g in case["windows"]]
    alone, _ = _bits(_run(one, windows=windows), one)
    M = case["M"]
    rows = [2 * m for m in range(M)] + [2 * M]              # (member, sample 0) of the batch, then target sample 0
    for k in su.event_names(case):
        assert np.array_equal(alone[k], wanted["m5_b2_6x8"][0][k][:, :, rows])


def test_hits_add_up_to_the_event_tables(cases):
    """NaN-free data: gen_hits summed over members, samples and a latitude's longitudes is the member-hit total of
    EventVerificationAggregator's table of the same windows: sum over slots, o and k of k x table[slot, lat, o, k]."""
    import sdy_amd

    case = cases["m5_b2_6x8"]
    spells = _run(case).get_data()
    ev = sdy_amd.EventVerificationAggregator(su.make_events(case), torch.from_numpy(case["weights"]).cuda(),
                                             n_timesteps=case["n_timesteps"])
    for start, target, gen in case["windows"]:
        ev.record_batch(0.0, {k: _contiguous(v) for k, v in target.items()}, {k: _contiguous(v) for k, v in gen.items()},
                        i_time_start=start)
    tables = ev.get_data()
    k_of = torch.arange(case["M"] + 1, dtype=torch.float64, device="cuda")
    for k in su.event_names(case):
        for name, _, _ in case["events"][k]:
            want = (tables[f"table/{name}/{k}"] * k_of).sum(dim=(0, 2, 3))
            got = spells[f"gen_hits/{name}/{k}"].sum(dim=(0, 1, 3))
            assert torch.equal(got, want) and float(got.sum()) > 0
            assert torch.equal(spells[f"rows/{name}/{k}"][0, :, 0], want)


def test_production_grid():
    """180 x 360, 25 members, 2 variables, 2 events (one a map with NaN points), 3 windows, against the host twin: from 16-byte
    accesses (the transposed view) and from views one element into a larger buffer (scalar loads)."""
    case = su.production_case()
    twin = su.host(case)
    assert all(twin[1][k].sum() > 1e5 for k in ("a", "b"))
    for layout in (_transposed, _offset):
        agg = _run(case, layout, target_layout=_contiguous if layout is _transposed else _offset)
        got = _bits(agg, case)
        assert su.same(got[0], twin[0]) and su.same(got[1], twin[1]), layout.__name__
    data = agg.get_data()
    want_data = su.readout(case, *twin)
    for key in ("rows/cool/a", "durations_gen/cool/b", "durations_target/wet/a", "target_longest/cool/a"):
        assert np.array_equal(data[key].cpu().numpy(), want_data[key], equal_nan=True), key
    assert np.isnan(want_data["target_longest/cool/a"]).sum() == 3
    want_logs, bounds = su.restate_logs(case, want_data, 8)
    su.close_logs(agg.get_logs(""), want_logs, bounds, "production")


def test_refusals_on_the_device_leave_everything_alone(cases):
    """A window out of order, another member count, another variable set, a ragged share: ValueError, and state and durations
    stay what they were."""
    import sdy_amd

    case = cases["m5_b2_6x8"]
    agg = _run(case, windows=case["windows"][:2])
    before = {s: v.clone() for s, v in agg._acc.items()}
    n_before, next_before = agg.n_times, agg._next_start
    start, target, gen = case["windows"][2]
    dev = lambda d: {k: _contiguous(v) for k, v in d.items()}  # noqa: E731
    for wrong in (6, 18, 0):
        with pytest.raises(ValueError, match=f"a window that starts at time {wrong}, where the one before ended at 12"):
            agg.record_batch(0.0, dev(target), dev(gen), i_time_start=wrong)
    with pytest.raises(ValueError, match="member count, sample count or grids of a window differ from the first window"):
        agg.record_batch(0.0, dev(target), dev({k: v[:2] for k, v in gen.items()}), i_time_start=12)
    with pytest.raises(ValueError, match="differ from the first window"):
        agg.record_batch(0.0, dev({"a": target["a"]}), dev({"a": gen["a"]}), i_time_start=12)
    flat = {k: v.reshape(-1, *v.shape[2:])[:7] for k, v in gen.items()}
    with pytest.raises(ValueError, match="EventSpellAggregator needs member-stacked"):
        agg.record_batch(0.0, dev(target), dev(flat), i_time_start=12)
    with pytest.raises(ValueError, match="member-stacked"):
        agg.record_batch(0.0, dev(target), dev(gen), i_time_start=12, sample_weights=[0.5, 0.5])
    with pytest.raises(ValueError, match="outside the aggregator's 24"):
        agg.record_batch(0.0, dev({k: np.concatenate([v, v, v], axis=1) for k, v in target.items()}),
                         dev({k: np.concatenate([v, v, v], axis=2) for k, v in gen.items()}), i_time_start=12)
    assert all(torch.equal(agg._acc[s], before[s]) for s in before)
    assert (agg.n_times, agg._next_start) == (n_before, next_before)
    # ... and the run goes on where it was
    for s, t, g in case["windows"][2:]:
        agg.record_batch(0.0, dev(t), dev(g), i_time_start=s)
    got, want = _bits(agg, case), su.restate(case)
    assert su.same(got[0], want[0]) and su.same(got[1], want[1])
    # max_bytes too small: refused at the first window, with the size in words
    need = 8 * sum(2 * len(case["events"][k]) * 12 * 48 + len(case["events"][k]) * 2 * 6 * 16 for k in ("a", "b"))
    small = sdy_amd.EventSpellAggregator(su.make_events(case), torch.from_numpy(case["weights"]).cuda(), n_timesteps=24,
                                         max_bytes=need - 1)
    s, t, g = case["windows"][0]
    with pytest.raises(ValueError, match=f"4 events of 2 variables, 5 members x 2 samples need {need} bytes"):
        small.record_batch(0.0, dev(t), dev(g), i_time_start=s)
    assert small._names is None and small._acc == {}
    with pytest.raises(ValueError, match="No data recorded."):
        small.get_logs("x")
    _run(case, max_bytes=need)


def test_a_window_with_the_initial_condition_only_counts_nothing(cases):
    import sdy_amd

    case = cases["m5_b2_6x8"]
    agg = _run(case, windows=su.recut(case, ((0, 1),)))
    assert agg.n_times == 0 and float(agg._acc["state"].abs().sum()) == 0.0
    with pytest.raises(ValueError, match="No data recorded."):
        agg.get_data()


def test_one_field_function(cases):
    import sdy_amd

    case = cases["m5_b2_6x8"]
    x = case["series"][0]["a"][0]                                    # (time, lat, lon)
    one = dict(M=1, B=1, H=6, W=8, names=["a"], events={"a": [("dry", "below", -0.3)]})
    want, _ = su.restate(one, [(5, {"a": x[None]}, {"a": x[None]})])
    got = sdy_amd.spells.spell_statistics(torch.from_numpy(x).cuda(), -0.3, below=True)
    assert list(got) == ["longest", "spells", "hits"]
    for w, key in ((1, "longest"), (2, "spells"), (3, "hits")):
        assert got[key].dtype == torch.float64 and np.array_equal(got[key].cpu().numpy(), want["a"][0, w, 0].astype(np.float64))
    thr = case["events"]["a"][2][2].copy()
    thr[2, 3] = np.nan
    one["events"] = {"a": [("anomaly", "above", thr)]}
    want, _ = su.restate(one, [(5, {"a": x[None]}, {"a": x[None]})])
    got = sdy_amd.spells.spell_statistics(torch.from_numpy(x).cuda(), torch.from_numpy(thr))
    expect = want["a"][0, 1, 0].astype(np.float64)
    expect[2, 3] = np.nan
    assert np.array_equal(got["longest"].cpu().numpy(), expect, equal_nan=True)


class _Recorder:
    """Hands every window on and keeps a copy of what it saw."""

    accepts_sample_weights = True

    def __init__(self, inner):
        self.inner, self.windows = inner, []

    def record_batch(self, loss, target_data, gen_data, target_data_norm, gen_data_norm, i_time_start=0, **kw):
        self.windows.append((i_time_start, {k: v.clone() for k, v in target_data.items()},
                             {k: v.clone() for k, v in gen_data.items()},
                             {k: v.clone() for k, v in target_data_norm.items()},
                             {k: v.clone() for k, v in gen_data_norm.items()}))
        self.inner.record_batch(loss=loss, target_data=target_data, gen_data=gen_data, target_data_norm=target_data_norm,
                                gen_data_norm=gen_data_norm, i_time_start=i_time_start, **kw)


def test_through_inference_aggregator_and_run_inference():
    """One pass of run_inference on the tiny loop fixture (2 windows x 6 steps, 2 samples, 3 members) with `events=...,
    event_spells=True` on two of its output variables: the data are the restatement's of the windows the run produced, and
    the logs gain exactly the `spells/...` keys over an aggregator with the events alone that is fed the same windows."""
    import sdy_amd
    from test_gpu_derived import _loop_setup

    _, stepper, windows, sigma, n_total, n_mem, names = _loop_setup(3)
    out = names["out_names"][:2]
    spec = {}
    for k in out:
        y = torch.cat([w.data[k][:, 1:] for w in windows], dim=1).numpy()
        spec[k] = [("above_mean_map", "above", y.mean(axis=(0, 1)).astype(np.float32)),
                   ("below_median", "below", float(np.median(y)))]
    events = sdy_amd.Events()
    for k in out:
        for name, direction, thr in spec[k]:
            events.add(k, name, **{direction: thr})
    w = sdy_amd.metrics.spherical_area_weights(torch.linspace(-87.0, 87.0, 32), 64).cuda()
    on = sdy_amd.metrics.InferenceAggregator(w, n_timesteps=n_total + 1, n_ensemble_members=3, events=events, event_spells=True)
    rec = _Recorder(on)
    sdy_amd.run_inference(rec, stepper, types.SimpleNamespace(loader=windows), n_total, n_mem, 3)
    off = sdy_amd.metrics.InferenceAggregator(w, n_timesteps=n_total + 1, n_ensemble_members=3, events=events)
    for start, target, gen, target_norm, gen_norm in rec.windows:
        off.record_batch(0.0, target, gen, target_norm, gen_norm, i_time_start=start)
    logs_on, logs_off = on.get_logs("inference"), off.get_logs("inference")
    order = [k for k in rec.windows[0][2] if k in spec]                        # the window's order of the variables with events
    new = [f"inference/spells/{m}/{name}/{k}" for k in order for name, _, _ in spec[k] for m in su.LOG_METRICS]
    assert [k for k in logs_on if k not in logs_off] == new and list(logs_on)[:len(logs_off)] == list(logs_off)
    assert all(isinstance(logs_on[k], float) for k in new)
    seen = dict(M=3, B=2, H=32, W=64, names=order, weights=w.cpu().numpy(), events=spec,
                windows=[(s, {k: t[k].cpu().numpy() for k in out}, {k: g[k].cpu().numpy() for k in out})
                         for s, t, g, _, _ in rec.windows])
    assert all(g[k].ndim == 5 and g[k].shape[0] == 3 for _, _, g in seen["windows"] for k in out)
    n = su.counted_times(seen["windows"])
    assert n == on._aggregators["spells"].n_times and n >= n_total - 1
    want_data = su.readout(seen, *su.restate(seen))
    _same_data(on.get_spell_data(), want_data)
    want_logs, bounds = su.restate_logs(seen, want_data, n, label="inference/spells")
    su.close_logs({k: logs_on[k] for k in new}, want_logs, bounds, "run_inference")
    assert sum(float(want_data[f"rows/{name}/{k}"][:, :, 1].sum()) for k in out for name, _, _ in spec[k]) > 0
