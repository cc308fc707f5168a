"""Threshold-event verification on the device (`sdy_amd.EventVerificationAggregator`; kernels of csrc/event_verif.hip) against
the library's _host twins and the numpy restatement, count for count; layouts, batch independence, determinism, pooled times,
frequency maps, refusals, the production grid, the logs, and the way through InferenceAggregator and run_inference.  Cases
and comparisons: tests/event_verif_utils.py.  Every test is a handful of launches."""
import types

import numpy as np
import pytest
import torch

import event_verif_utils as eu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return eu.cases()


@pytest.fixture(scope="module")
def wanted(cases):
    """The restatement of every small case, computed once: {(name, pool): (tables, maps)}."""
    return {(name, pool): eu.restate(case, pool) for name, case in cases.items() for pool in (False, True)}


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


def _run(case, layout=_contiguous, windows=None, pool=False, target_layout=_contiguous, maps=True):
    import sdy_amd

    agg = sdy_amd.EventVerificationAggregator(eu.make_events(case), torch.from_numpy(case["weights"]).cuda(),
                                              n_timesteps=case["n_timesteps"], pool_times=pool, frequency_maps=maps)
    for start, target, gen in (case["windows"] if windows is None else windows):
        agg.record_batch(0.0, {k: target_layout(v) for k, v in target.items()}, {k: layout(v) for k, v in gen.items()},
                         i_time_start=start)
    return agg


def _data_keys(case, maps=True):
    per = ("table",) + eu.SLOT_METRICS + ("reliability_curve",) + (("frequency_gen", "frequency_target", "counted") if maps else ())
    return [f"{s}/{name}/{k}" for k in eu.event_names(case) for name, _, _ in case["events"][k] for s in per]


def _counts(agg, case, maps=True):
    """-> (tables {var: (n_slots, E, H, 2, M + 1)}, maps {var: (E, 3, H, W)} rebuilt from the frequencies) as numpy."""
    data = agg.get_data()
    assert all(v.dtype == torch.float64 and v.is_cuda for v in data.values())
    assert list(data) == _data_keys(case, maps)
    tables, freq = {}, {}
    for k in eu.event_names(case):
        names = [name for name, _, _ in case["events"][k]]
        tables[k] = np.stack([data[f"table/{n}/{k}"].cpu().numpy() for n in names], axis=1)
    if maps:
        acc = agg._acc["maps"].cpu().numpy()
        for i, k in enumerate(eu.event_names(case)):
            E, H, W = len(case["events"][k]), case["H"], case["W"]
            at = agg._offsets["maps"][i]
            freq[k] = acc[at:at + E * 3 * H * W].reshape(E, 3, H, W)
    return tables, freq


@pytest.mark.parametrize("pool", [False, True], ids=["slots", "pooled"])
@pytest.mark.parametrize("name", eu.SMALL)
def test_device_equals_host_equals_restatement(cases, wanted, name, pool):
    case = cases[name]
    agg = _run(case, pool=pool)
    got, twin, want = _counts(agg, case), eu.host(case, pool), wanted[name, pool]
    assert eu.same(got[0], twin[0]) and eu.same(got[0], want[0])
    assert eu.same(got[1], twin[1]) and eu.same(got[1], want[1])
    data, w = agg.get_data(), eu.lat_weights(case)
    for k in eu.event_names(case):
        for e, (ev, _, _) in enumerate(case["events"][k]):
            for slot in range(want[0][k].shape[0]):
                s = eu.restate_scores(want[0][k][slot, e], w)
                have = {m: data[f"{m}/{ev}/{k}"][slot].cpu().numpy() for m in eu.SLOT_METRICS + ("reliability_curve",)}
                eu.close_scores(have, {m: s[m] for m in have}, f"{name} {k} {ev} {slot}")
            hits, obs, counted = want[1][k][e]
            with np.errstate(invalid="ignore", divide="ignore"):
                eu.close(data[f"frequency_gen/{ev}/{k}"].cpu().numpy(), hits / (case["M"] * counted), f"{name} frequency_gen")
                eu.close(data[f"frequency_target/{ev}/{k}"].cpu().numpy(), obs / counted, f"{name} frequency_target")
            assert np.array_equal(data[f"counted/{ev}/{k}"].cpu().numpy(), counted)
    logs = agg.get_logs("")
    want_logs = eu.restate_logs(case, want[0])
    assert list(logs) == list(want_logs) and all(isinstance(v, float) for v in logs.values())
    for key, v in want_logs.items():
        unc = want_logs["base_rate/" + key.split("/", 1)[1]]
        scale = 1.0 / (unc * (1 - unc)) if key.startswith("brier_skill_score/") and 0 < unc < 1 else 1.0
        eu.close(logs[key], v, f"{key} {name}", scale)
    assert list(agg.get_logs("ev")) == [f"ev/{k}" for k in want_logs]


def test_known_answer_on_the_device(cases):
    case = cases["known_m5_b2_6x8"]
    tables, maps = _counts(_run(case), case)
    want = np.zeros((6, 2, 6))
    want[:3, 0, 3] = want[3:, 1, 3] = case["B"] * case["W"]
    for k in ("a", "b"):
        for slot in range(1, 5):
            assert np.array_equal(tables[k][slot, 0], want)
        assert (tables[k][0] == 0).all() and (maps[k][0, 0] == 3 * 8).all() and (maps[k][0, 2] == 8).all()


def test_pooled_times_equal_the_slots_summed(cases, wanted):
    case = cases["m5_b2_6x8"]
    tables, maps = _counts(_run(case), case)
    pooled, pooled_maps = _counts(_run(case, pool=True), case)
    assert eu.same(pooled, {k: v.sum(axis=0, keepdims=True) for k, v in tables.items()}) and eu.same(pooled_maps, maps)


@pytest.mark.parametrize("name", ["m5_b2_6x8", "m25_b1_4x360", "nan_m5_b2_6x8"])
def test_layouts_give_the_same_counts(cases, wanted, name):
    """Contiguous, the transposed view of a (samples, members, ...) buffer, and views one element into a larger buffer (scalar
    loads): integers, so identical."""
    case = cases[name]
    for layout, target_layout in ((_transposed, _contiguous), (_offset, _contiguous), (_contiguous, _offset), (_offset, _offset)):
        for pool in (False, True):
            got = _counts(_run(case, layout, pool=pool, target_layout=target_layout), case)
            want = wanted[name, pool]
            assert eu.same(got[0], want[0]) and eu.same(got[1], want[1]), (layout.__name__, target_layout.__name__, pool)


def test_samples_add_up(cases, wanted):
    """Sample 0 alone plus sample 1 alone equals both together."""
    case = cases["clipped_m5_b2_6x8"]
    parts = []
    for b in range(2):
        one = [(s, {k: v[b:b + 1] for k, v in t.items()}, {k: v[:, b:b + 1] for k, v in g.items()}) for s, t, g in case["windows"]]
        parts.append(_counts(_run(case, windows=one), case))
    both = wanted["clipped_m5_b2_6x8", False]
    for j in (0, 1):
        assert eu.same({k: parts[0][j][k] + parts[1][j][k] for k in both[j]}, both[j])


def test_two_runs_give_the_same_bits(cases):
    case = cases["m25_b1_4x360"]
    a, b = _run(case), _run(case)
    assert all(torch.equal(a._acc[s], b._acc[s]) for s in ("table", "maps")) and a.get_logs("x") == b.get_logs("x")


def test_frequency_maps_are_optional(cases, wanted):
    case = cases["m5_b2_6x8"]
    agg = _run(case, maps=False)
    assert list(agg._acc) == ["table"]
    tables, _ = _counts(agg, case, maps=False)
    assert eu.same(tables, wanted["m5_b2_6x8", False][0])


def test_a_later_window_of_another_job_is_refused(cases):
    """Through the class on the device: another variable set, member count or a window past the last slot raises and leaves
    the accumulators alone."""
    case = cases["m5_b2_6x8"]
    agg = _run(case)
    before = {s: v.clone() for s, v in agg._acc.items()}
    start, target, gen = case["windows"][1]
    dev = lambda d: {k: _contiguous(v) for k, v in d.items()}  # noqa: E731
    with pytest.raises(ValueError, match="differ from the first window"):
        agg.record_batch(0.0, dev({"a": target["a"]}), dev({"a": gen["a"]}), i_time_start=3)
    with pytest.raises(ValueError, match="member count, sample count or grids of a window differ from the first window"):
        agg.record_batch(0.0, dev(target), dev({k: v[:2] for k, v in gen.items()}), i_time_start=3)
    with pytest.raises(ValueError, match="outside the aggregator's 5"):
        agg.record_batch(0.0, dev(target), dev(gen), i_time_start=4)
    assert all(torch.equal(agg._acc[s], before[s]) for s in before)


def test_production_grid():
    """One 180 x 360 window of 25 members, 2 variables, 2 times, E = 4 with one map threshold: device against the host twins
    and the restatement, from 16-byte loads and from views one element into a larger buffer (scalar loads)."""
    case = eu.production_case()
    assert sum(isinstance(t, np.ndarray) for _, _, t in case["events"]["a"]) == 1 and len(case["events"]["a"]) == 4
    want = eu.restate(case)
    twin = eu.host(case)
    assert eu.same(twin[0], want[0]) and eu.same(twin[1], want[1])
    assert all(want[0][k].sum() == 4 * 2 * 180 * 360 for k in ("a", "b"))
    want_logs = eu.restate_logs(case, want[0])
    for layout in (_transposed, _offset):
        agg = _run(case, layout, target_layout=_contiguous if layout is _transposed else _offset)
        got = _counts(agg, case)
        assert eu.same(got[0], want[0]) and eu.same(got[1], want[1]), layout.__name__
        logs = agg.get_logs("")
        for key, v in want_logs.items():
            unc = want_logs["base_rate/" + key.split("/", 1)[1]]
            eu.close(logs[key], v, f"production {key}", 1.0 / (unc * (1 - unc)) if key.startswith("brier_skill_score/") else 1.0)


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
    """One pass of run_inference on the tiny loop fixture (2 windows x 6 steps, 2 samples, 3 members) with `events=...` on two
    of its output variables: the tables are the restatement's of the windows the run produced, the logs gain exactly the
    `events/...` keys over an aggregator without events that is fed the same windows, and that one's key list is the default
    one, in its order."""
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
    on = sdy_amd.metrics.InferenceAggregator(w, n_timesteps=n_total + 1, n_ensemble_members=3, events=events)
    rec = _Recorder(on)
    sdy_amd.run_inference(rec, stepper, types.SimpleNamespace(loader=windows), n_total, n_mem, 3)
    off = sdy_amd.metrics.InferenceAggregator(w, n_timesteps=n_total + 1, n_ensemble_members=3)
    plain = sdy_amd.metrics.InferenceAggregator(w, n_timesteps=n_total + 1, n_ensemble_members=3, events=None)
    for start, target, gen, target_norm, gen_norm in rec.windows:
        for agg in (off, plain):
            agg.record_batch(0.0, target, gen, target_norm, gen_norm, i_time_start=start)
    logs_on, logs_off = on.get_logs("inference"), off.get_logs("inference")
    order = [k for k in rec.windows[0][2] if k in spec]                        # the window's order of the variables with events
    new = [f"inference/events/{m}/{name}/{k}" for k in order for name, _, _ in spec[k] for m in eu.LOG_METRICS]
    assert [k for k in logs_on if k not in logs_off] == new and list(logs_on)[:len(logs_off)] == list(logs_off)
    assert list(plain.get_logs("inference")) == list(logs_off)                 # no events: the default key list, in its order
    assert all(isinstance(logs_on[k], float) for k in new)
    seen = dict(M=3, B=2, H=32, W=64, names=list(rec.windows[0][2]), weights=w.cpu().numpy(), n_timesteps=n_total + 1, events=spec,
                windows=[(s, {k: t[k].cpu().numpy() for k in out}, {k: g[k].cpu().numpy() for k in out})
                         for s, t, g, _, _ in rec.windows])
    assert all(g[k].ndim == 5 and g[k].shape[0] == 3 for _, _, g in seen["windows"] for k in out)
    want, _ = eu.restate(seen)
    data = on.get_event_data()
    for k in out:
        for e, (name, _, _) in enumerate(spec[k]):
            assert tuple(data[f"table/{name}/{k}"].shape) == (n_total + 1, 32, 2, 4)
            assert np.array_equal(data[f"table/{name}/{k}"].cpu().numpy(), want[k][:, e])
            assert want[k][0, e].sum() == 0 and (want[k][1:, e].sum(axis=(1, 2, 3)) == 2 * 32 * 64).all()
    for key, v in eu.restate_logs(seen, want, label="inference/events").items():
        unc = logs_on["inference/events/base_rate/" + key.split("/", 3)[3]]
        scale = 1.0 / (unc * (1 - unc)) if "/brier_skill_score/" in key and 0 < unc < 1 else 1.0
        eu.close(logs_on[key], v, key, scale)
