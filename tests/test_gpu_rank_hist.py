"""Ensemble rank histograms on the device (`sdy_amd.RankHistogramAggregator`; kernel of csrc/rank_hist.hip) against the library's
_host twin and the numpy restatement, count for count; layouts, batch independence, determinism, pooled times, the production
grid, the logs, and the way through InferenceAggregator and run_inference.  Cases and comparisons: tests/rank_hist_utils.py.
Every case is a handful of launches."""
import types

import numpy as np
import pytest
import torch

import rank_hist_utils as ru

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return ru.cases()


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


def _run(case, layout=_contiguous, windows=None, pool=False, target_layout=_contiguous):
    import sdy_amd

    agg = sdy_amd.RankHistogramAggregator(torch.from_numpy(case["weights"]).cuda(), n_timesteps=case["n_timesteps"],
                                          pool_times=pool)
    for start, target, gen in (case["windows"] if windows is None else windows):
        agg.record_batch(0.0, {k: target_layout(v) for k, v in target.items()}, {k: layout(v) for k, v in gen.items()},
                         i_time_start=start)
    return agg


def _counts(agg, case):
    """-> (counts (nvars, n_slots, H, M + 1), ties (nvars, n_slots, H)) from get_data(), as numpy."""
    data = agg.get_data()
    assert all(v.dtype == torch.float64 and v.is_cuda for v in data.values())
    assert list(data) == [f"{s}/{k}" for k in case["names"] for s in ("counts", "ties", "frequency")]
    return (np.stack([data[f"counts/{k}"].cpu().numpy() for k in case["names"]]),
            np.stack([data[f"ties/{k}"].cpu().numpy() for k in case["names"]]))


def _same(got, want):
    return got[0].shape == want[0].shape and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("pool", [False, True], ids=["slots", "pooled"])
@pytest.mark.parametrize("name", ru.SMALL)
def test_device_equals_host_equals_restatement(cases, name, pool):
    case = cases[name]
    agg = _run(case, pool=pool)
    got, twin, want = _counts(agg, case), ru.host(case, pool), ru.restate(case, pool)
    assert _same(got, twin) and _same(got, want)
    data = agg.get_data()
    freq = np.stack([data[f"frequency/{k}"].cpu().numpy() for k in case["names"]])
    ru.close(freq, ru.restate_frequency(case, want[0]), f"frequency {name}")
    if not pool:
        assert np.isnan(freq[:, 0]).all() and np.isfinite(freq[:, 1:]).all()       # the initial condition's slot is empty
    logs = agg.get_logs("")
    want_logs = ru.restate_logs(case, *want)
    assert list(logs) == list(want_logs) and all(isinstance(v, float) for v in logs.values())
    for k, v in want_logs.items():
        ru.close(logs[k], v, f"{k} {name}")
    assert list(agg.get_logs("cal")) == [f"cal/{k}" for k in want_logs]


def test_known_answer_on_the_device(cases):
    case = cases["known_m5_b2_6x8"]
    counts, ties = _counts(_run(case), case)
    for slot in range(1, 5):
        assert np.array_equal(counts[:, slot], np.broadcast_to(case["B"] * case["W"] * np.eye(6), (2, 6, 6)))
    assert (counts[:, 0] == 0).all() and (ties == 0).all()


def test_pooled_times_equal_the_slots_summed(cases):
    case = cases["m5_b2_6x8"]
    counts, ties = _counts(_run(case), case)
    pooled = _counts(_run(case, pool=True), case)
    assert np.array_equal(pooled[0][:, 0], counts.sum(axis=1)) and np.array_equal(pooled[1][:, 0], ties.sum(axis=1))


@pytest.mark.parametrize("name", ["m5_b2_6x8", "m25_b1_4x360", "nan_m5_b2_6x8"])
def test_layouts_give_the_same_counts(cases, name):
    """Contiguous, the transposed view of a (samples, members, ...) buffer, and views one element into a larger buffer (scalar
    loads): integers, so identical."""
    case = cases[name]
    ref = _counts(_run(case), case)
    for layout, target_layout in ((_transposed, _contiguous), (_offset, _contiguous), (_contiguous, _offset), (_offset, _offset)):
        for pool in (False, True):
            got = _counts(_run(case, layout, pool=pool, target_layout=target_layout), case)
            want = ref if not pool else (ref[0].sum(axis=1, keepdims=True), ref[1].sum(axis=1, keepdims=True))
            assert _same(got, want), (layout.__name__, target_layout.__name__, pool)


def test_samples_add_up(cases):
    """Sample 0 alone plus sample 1 alone equals both together."""
    case = cases["clipped_m5_b2_6x8"]
    both = _counts(_run(case), case)
    parts = []
    for b in range(2):
        one = [(s, {k: v[b:b + 1] for k, v in t.items()}, {k: v[:, b:b + 1] for k, v in g.items()}) for s, t, g in case["windows"]]
        parts.append(_counts(_run(case, windows=one), case))
    assert _same((parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]), both)


def test_two_runs_give_the_same_counts(cases):
    case = cases["m25_b1_4x360"]
    a, b = _run(case), _run(case)
    assert _same(_counts(a, case), _counts(b, case)) and a.get_logs("x") == b.get_logs("x")


def test_a_later_window_of_another_job_is_refused(cases):
    """Through the class on the device: another variable set, member count or a window past the last slot raises and leaves
    the accumulators alone."""
    case = cases["m5_b2_6x8"]
    agg = _run(case)
    before = _counts(agg, case)
    start, target, gen = case["windows"][1]
    dev = lambda d: {k: _contiguous(v) for k, v in d.items()}  # noqa: E731
    with pytest.raises(ValueError, match="differ from the first window"):
        agg.record_batch(0.0, dev({"a": target["a"], "c": target["b"]}), dev({"a": gen["a"], "c": gen["b"]}), i_time_start=3)
    with pytest.raises(ValueError, match="member count, sample count or grids of a window differ from the first window"):
        agg.record_batch(0.0, dev(target), dev({k: v[:2] for k, v in gen.items()}), i_time_start=3)
    with pytest.raises(ValueError, match="outside the aggregator's 5"):
        agg.record_batch(0.0, dev(target), dev(gen), i_time_start=4)
    assert _same(_counts(agg, case), before)


def test_production_grid():
    """One 180 x 360 window of 25 members, 2 variables, 2 times: device against the host twin and the restatement, from
    16-byte loads and from views one element into a larger buffer (scalar loads)."""
    case = ru.production_case()
    want = ru.restate(case)
    assert _same(ru.host(case), want) and want[0].sum() == 2 * 2 * 180 * 360
    want_logs = ru.restate_logs(case, *want)
    for layout in (_transposed, _offset):
        agg = _run(case, layout, target_layout=_contiguous if layout is _transposed else _offset)
        assert _same(_counts(agg, case), want), layout.__name__
        logs = agg.get_logs("")
        for k, v in want_logs.items():
            ru.close(logs[k], v, f"production {k}")
    pooled = _counts(_run(case, pool=True), case)
    assert _same(pooled, (want[0].sum(axis=1, keepdims=True), want[1].sum(axis=1, keepdims=True)))


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
    """One pass of run_inference on the tiny loop fixture (2 windows x 6 steps, 2 samples, 3 members) with
    `rank_histogram_data=True`: the counts are the restatement's of the windows the run produced (its first time, the initial
    condition, not counted), the logs gain exactly the `rank_histogram/...` keys over an aggregator with the flag off that is
    fed the same windows, and that one's key set is the default one."""
    import sdy_amd
    from test_gpu_derived import _loop_setup

    _, stepper, windows, sigma, n_total, n_mem, names = _loop_setup(3)
    w = sdy_amd.metrics.spherical_area_weights(torch.linspace(-87.0, 87.0, 32), 64).cuda()
    on = sdy_amd.metrics.InferenceAggregator(w, n_timesteps=n_total + 1, n_ensemble_members=3, rank_histogram_data=True)
    rec = _Recorder(on)
    sdy_amd.run_inference(rec, stepper, types.SimpleNamespace(loader=windows), n_total, n_mem, 3)
    off = sdy_amd.metrics.InferenceAggregator(w, n_timesteps=n_total + 1, n_ensemble_members=3)
    plain = sdy_amd.metrics.InferenceAggregator(w, n_timesteps=n_total + 1, n_ensemble_members=3, rank_histogram_data=False)
    for start, target, gen, target_norm, gen_norm in rec.windows:
        for agg in (off, plain):
            agg.record_batch(0.0, target, gen, target_norm, gen_norm, i_time_start=start)
    logs_on, logs_off = on.get_logs("inference"), off.get_logs("inference")
    out = names["out_names"]
    new = {f"inference/rank_histogram/{lab}/{n}" for n in out for lab in ("reliability_index", "outlier_fraction", "tie_fraction")}
    assert set(logs_on) - set(logs_off) == new and set(logs_off) <= set(logs_on)
    assert list(plain.get_logs("inference")) == list(logs_off)                 # flag off: the default key set, in its order
    assert all(isinstance(logs_on[k], float) and np.isfinite(logs_on[k]) for k in new)
    seen = dict(M=3, B=2, H=32, W=64, names=out, weights=w.cpu().numpy(), n_timesteps=n_total + 1,
                windows=[(s, {k: t[k].cpu().numpy() for k in out}, {k: g[k].cpu().numpy() for k in out})
                         for s, t, g, _, _ in rec.windows])
    assert all(g[k].ndim == 5 and g[k].shape[0] == 3 for _, _, g in seen["windows"] for k in out)
    want = ru.restate(seen)
    data = on.get_rank_histogram_data()
    for j, k in enumerate(out):
        assert tuple(data[f"counts/{k}"].shape) == (n_total + 1, 32, 4) and tuple(data[f"ties/{k}"].shape) == (n_total + 1, 32)
        assert np.array_equal(data[f"counts/{k}"].cpu().numpy(), want[0][j]) and np.array_equal(data[f"ties/{k}"].cpu().numpy(), want[1][j])
        assert want[0][j, 0].sum() == 0 and (want[0][j, 1:].sum(axis=(1, 2)) == 2 * 32 * 64).all()
    for k, v in ru.restate_logs(seen, *want, label="inference/rank_histogram").items():
        ru.close(logs_on[k], v, k)
