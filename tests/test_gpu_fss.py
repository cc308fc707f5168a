"""Neighbourhood verification on the device (`sdy_amd.FractionsSkillAggregator`; kernels of csrc/fss.hip) against the library's
_host twin and the numpy restatement, sum for sum: clipped rows and wrap, the whole circle, scalar loads, halos across bands,
the 16- and 32-bit bounds, NaN rules, layouts, windows, slots against pooled, batch independence, workspace chunks, the
production grid, a planted displacement, the keys, and the way through InferenceAggregator and run_inference.  Cases and
comparisons: tests/fss_utils.py.  Every test is a handful of launches."""
import types

import numpy as np
import pytest
import torch

import fss_utils as fu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return fu.cases()


@pytest.fixture(scope="module")
def wanted(cases):
    """The restatement of every small case, computed once: {name: (sums, brute-force fractions)}."""
    return {name: fu.restate(case, brute=True) for name, case in cases.items()}


def _contiguous(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _transposed(x):
    """(members, samples, ...) as the window driver hands it over: a transposed view of a sample-major buffer."""
    if x.ndim != 5:
        return _contiguous(x)
    buf = _contiguous(x).transpose(0, 1).contiguous()
    return buf.transpose(0, 1)


def _offset(x):
    """A view that starts one element into a larger buffer: 4 bytes off a 16-byte boundary, so the scalar path."""
    buf = torch.zeros(x.size + 1, device="cuda")
    buf[1:] = _contiguous(x).reshape(-1)
    out = buf[1:].view(x.shape)
    assert out.data_ptr() % 16 == 4
    return out


def _run(case, layout=_contiguous, windows=None, pool=False, target_layout=_contiguous, **kw):
    import sdy_amd

    agg = sdy_amd.FractionsSkillAggregator(fu.make_events(case), case["radii"], torch.from_numpy(case["weights"]).cuda(),
                                           n_timesteps=case["n_timesteps"], pool_times=pool, **kw)
    for start, target, gen in (case["windows"] if windows is None else windows):
        agg.record_batch(0.0, {k: target_layout(v) for k, v in target.items()}, {k: layout(v) for k, v in gen.items()},
                         i_time_start=start)
    return agg


def _data_keys(case):
    return [f"{s}_r{r}/{name}/{k}" for k in fu.event_names(case) for name, _, _ in case["events"][k] for r in case["radii"]
            for s in ("sums",) + fu.SLOT_METRICS]


def _sums(agg, case):
    """-> {var: (n_slots, E, R, H, 6)} as numpy, from get_data()."""
    data = agg.get_data()
    assert all(v.dtype == torch.float64 and v.is_cuda for v in data.values())
    assert list(data) == _data_keys(case)
    return {k: np.stack([np.stack([data[f"sums_r{r}/{name}/{k}"].cpu().numpy() for r in case["radii"]], axis=1)
                         for name, _, _ in case["events"][k]], axis=1) for k in fu.event_names(case)}


@pytest.mark.parametrize("pool", [False, True], ids=["slots", "pooled"])
@pytest.mark.parametrize("name", fu.SMALL)
def test_device_equals_host_equals_restatement(cases, wanted, name, pool):
    case = cases[name]
    agg = _run(case, pool=pool)
    got, twin = _sums(agg, case), fu.host(case, pool)
    want = {k: (v.sum(axis=0, keepdims=True) if pool else v) for k, v in wanted[name][0].items()}
    assert fu.same(got, twin) and fu.same(got, want)
    frac = {k: (v.sum(axis=0, keepdims=True) if pool else v) for k, v in wanted[name][1].items()}
    data = agg.get_data()
    for k in fu.event_names(case):
        s = fu.brute_scores(frac[k])                                       # (slots, E, R)
        for e, (ev, _, _) in enumerate(case["events"][k]):
            for j, r in enumerate(case["radii"]):
                for metric in fu.SLOT_METRICS:
                    fu.close(data[f"{metric}_r{r}/{ev}/{k}"].cpu().numpy(), s[metric][:, e, j], f"{name} {metric} r{r} {ev} {k}")
    logs, want_logs = agg.get_logs(""), fu.restate_logs(case, wanted[name][1])
    assert list(logs) == list(want_logs) and all(isinstance(v, float) for v in logs.values())
    for key, v in want_logs.items():
        fu.close(logs[key], v, f"{name} {key}")
    assert list(agg.get_logs("fss")) == [f"fss/{k}" for k in want_logs]


def test_known_answer_at_the_bounds_on_the_device(cases):
    """K = M n = 61504 at every full neighbourhood of the M = 64, r = 15 case: the 16-bit box sums and their 32-bit squares."""
    got = _sums(_run(cases["m64_b1_33x32_full"]), cases["m64_b1_33x32_full"])["a"]
    n = fu.sizes(33, 15).astype(np.float64)
    want = np.stack([np.full(33, 32.0), 32 * 64 * n, 32 * n, 32 * (64 * n) ** 2, 32 * 64 * n * n, 32 * n * n], axis=-1)
    assert np.array_equal(got[1, 0, 0], want) and np.array_equal(got[2, 0, 0], want) and (got[0] == 0).all()
    assert want[:, 3].max() == 32 * 61504.0 ** 2


def test_nan_removes_the_centres_within_r_and_no_others():
    """One masked point at (lat 6, lon 3) of a 13 x 12 grid -- a NaN target, or a NaN in the threshold map: at radius r exactly
    the centres within r of it are not counted, those at distance r + 1 are.  A NaN member removes nothing."""
    H, W, M = 13, 12, 3
    for where in ("target", "map", "member"):
        y = np.ones((1, 1, H, W), np.float32)
        g = np.ones((M, 1, 1, H, W), np.float32)
        thr = np.zeros((H, W), np.float32)
        if where == "target":
            y[0, 0, 6, 3] = np.nan
        elif where == "map":
            thr[6, 3] = np.nan
        else:
            g[1, 0, 0, 6, 3] = np.nan
        case = dict(M=M, B=1, H=H, W=W, names=["a"], weights=np.ones((H, W), np.float32), n_timesteps=2, radii=(0, 1, 2, 4),
                    windows=[(1, {"a": y}, {"a": g})], events={"a": [("positive", "above", thr)]})
        got = _sums(_run(case), case)
        assert fu.same(got, fu.restate(case)) and fu.same(got, fu.host(case))
        for j, r in enumerate(case["radii"]):
            lost = np.where(np.abs(np.arange(H) - 6) <= r, 2 * r + 1, 0)
            assert np.array_equal(got["a"][1, 0, j, :, 0], W - (0 * lost if where == "member" else lost)), (where, r)


@pytest.mark.parametrize("name", ["m3_b2_5x8", "m4_b2_5x6", "nan_m5_b2_6x8"])
def test_layouts_give_the_same_sums(cases, wanted, name):
    """Contiguous, the transposed view of a (samples, members, ...) buffer, and views 4 bytes into a larger buffer (scalar
    loads): integers, so identical."""
    case = cases[name]
    for layout, target_layout in ((_transposed, _contiguous), (_offset, _contiguous), (_contiguous, _offset), (_offset, _offset)):
        assert fu.same(_sums(_run(case, layout, target_layout=target_layout), case), wanted[name][0]), layout.__name__


def test_one_run_cut_into_windows_two_ways(cases, wanted):
    """Five times as windows of (3, 2) and of (1, 2, 2): the same slots; and the slots summed are the pooled sums."""
    case = cases["m3_b2_5x8"]
    whole_t = {k: np.concatenate([t[k] for _, t, _ in case["windows"]], axis=1) for k in case["names"]}
    whole_g = {k: np.concatenate([g[k] for _, _, g in case["windows"]], axis=2) for k in case["names"]}
    cut = [(s, {k: v[:, s:s + n] for k, v in whole_t.items()}, {k: v[:, :, s:s + n] for k, v in whole_g.items()})
           for s, n in ((0, 1), (1, 2), (3, 2))]
    got = _sums(_run(case, windows=cut), case)
    assert fu.same(got, wanted["m3_b2_5x8"][0])
    pooled = _sums(_run(case, windows=cut, pool=True), case)
    assert fu.same(pooled, {k: v.sum(axis=0, keepdims=True) for k, v in got.items()})


def test_a_sample_in_a_batch_of_one_and_of_three():
    """Sample 1's sums alone equal its share of a batch of three: the three alone add up to the batch."""
    import rank_hist_utils as ru

    base = ru.make_case(4, 3, 7, 12, seed=41, names=("a",))
    case = fu._with(base, (0, 1, 3), {"a": fu._events(base, "a", 2)})
    both = _sums(_run(case), case)
    parts = []
    for b in range(3):
        one = [(s, {k: v[b:b + 1] for k, v in t.items()}, {k: v[:, b:b + 1] for k, v in g.items()}) for s, t, g in case["windows"]]
        parts.append(_sums(_run(case, windows=one), case))
        assert fu.same(parts[-1], fu.restate(case, windows=one))
    assert fu.same({"a": parts[0]["a"] + parts[1]["a"] + parts[2]["a"]}, both) and fu.same(both, fu.restate(case))


def test_a_small_workspace_forces_several_chunks(cases, wanted):
    """Three variables with equal extents and event count, a workspace that holds the codes of one: three calls, the same bits."""
    import rank_hist_utils as ru

    base = ru.make_case(3, 2, 5, 8, seed=42, names=("a", "b", "c"))
    case = fu._with(base, (0, 2), {k: fu._events(base, k, 2) for k in base["names"]})
    one = 2 * 2 * 3 * 5 * 8 * 2                                            # the first window's codes of one variable
    agg = _run(case, workspace_bytes=one + 7)
    assert agg._ws.numel() == one                                          # the codes of one variable at a time: three calls
    want = fu.restate(case)
    assert fu.same(_sums(agg, case), want) and fu.same(_sums(_run(case), case), want)
    two = _run(case, workspace_bytes=2 * one)
    assert two._ws.numel() == 2 * one and fu.same(_sums(two, case), want)


def test_two_runs_give_the_same_bits(cases):
    case = cases["m25_b1_37x40"]
    a, b = _run(case), _run(case)
    assert torch.equal(a._acc["sums"], b._acc["sums"]) and a.get_logs("x") == b.get_logs("x")


def test_a_later_window_of_another_job_is_refused(cases):
    case = cases["m3_b2_5x8"]
    agg = _run(case)
    before = agg._acc["sums"].clone()
    start, target, gen = case["windows"][1]
    dev = lambda d: {k: _contiguous(v) for k, v in d.items()}  # noqa: E731
    with pytest.raises(ValueError, match="differ from the first window"):
        agg.record_batch(0.0, dev({"a": target["a"]}), dev({"a": gen["a"]}), i_time_start=3)
    with pytest.raises(ValueError, match="member count, sample count or grids of a window differ from the first window"):
        agg.record_batch(0.0, dev(target), dev({k: v[:2] for k, v in gen.items()}), i_time_start=3)
    with pytest.raises(ValueError, match="outside the aggregator's 5"):
        agg.record_batch(0.0, dev(target), dev(gen), i_time_start=4)
    assert torch.equal(agg._acc["sums"], before)


def test_production_grid():
    """One 180 x 360 window of 25 members, one variable, 2 times, radii (1, 3, 7, 15), two events (a scalar and a map): the
    device against the host twin, from the transposed view (16-byte loads) and from 4-byte-offset views (scalar loads)."""
    case = fu.production_case()
    assert case["radii"] == (1, 3, 7, 15) and [isinstance(t, np.ndarray) for _, _, t in case["events"]["a"]] == [False, True]
    twin = fu.host(case)
    assert (twin["a"][4:, :, :, :, 0] == 360).all() and (twin["a"][:4] == 0).all()      # no NaN: every centre is counted
    for layout in (_transposed, _offset):
        got = _sums(_run(case, layout, target_layout=_contiguous if layout is _transposed else _offset), case)
        assert fu.same(got, twin), layout.__name__


def test_a_planted_displacement_is_forgiven_with_the_radius():
    """Every member is the truth moved 2 longitudes east: point by point the forecast is wrong wherever an event's edge is,
    a neighbourhood that spans the displacement sees the same fractions.  FSS is below 1 at r = 0 and rises with r."""
    case = fu.displaced_case(shift=2)
    agg = _run(case, pool=True)
    assert fu.same(_sums(agg, case), fu.restate(case, pool=True))
    logs = agg.get_logs("")
    fss = [logs[f"fss_r{r}/high/a"] for r in case["radii"]]
    assert fss[0] < 1.0 and all(b > a for a, b in zip(fss, fss[1:])), fss
    assert all(abs(logs[f"counted_fraction_r{r}/high/a"] - 1.0) <= fu.TOL for r in case["radii"])
    assert abs(logs["base_rate_r0/high/a"] - 0.2) < 0.02 and logs["fss_useful_r0/high/a"] == 0.5 + logs["base_rate_r0/high/a"] / 2


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
    event_neighbourhoods=(0, 2)` on two of its output variables: the sums are the restatement's of the windows the run
    produced, the logs gain exactly the `fss/...` keys over an aggregator with the events alone, and with
    `event_neighbourhoods=None` the key list is the parent's."""
    import sdy_amd
    from test_gpu_derived import _loop_setup

    _, stepper, windows, sigma, n_total, n_mem, names = _loop_setup(3)
    out = names["out_names"][:2]
    spec = {}
    for k in out:
        y = torch.cat([w.data[k][:, 1:] for w in windows], dim=1).numpy()
        spec[k] = [("above_mean_map", "above", y.mean(axis=(0, 1)).astype(np.float32)), ("below_median", "below", float(np.median(y)))]
    events = sdy_amd.Events()
    for k in out:
        for name, direction, thr in spec[k]:
            events.add(k, name, **{direction: thr})
    w = sdy_amd.metrics.spherical_area_weights(torch.linspace(-87.0, 87.0, 32), 64).cuda()
    kw = dict(n_timesteps=n_total + 1, n_ensemble_members=3)
    on = sdy_amd.metrics.InferenceAggregator(w, events=events, event_neighbourhoods=(0, 2), **kw)
    rec = _Recorder(on)
    sdy_amd.run_inference(rec, stepper, types.SimpleNamespace(loader=windows), n_total, n_mem, 3)
    off = sdy_amd.metrics.InferenceAggregator(w, events=events, **kw)
    none = sdy_amd.metrics.InferenceAggregator(w, events=events, event_neighbourhoods=None, **kw)
    bare = sdy_amd.metrics.InferenceAggregator(w, **kw)
    for start, target, gen, target_norm, gen_norm in rec.windows:
        for agg in (off, none, bare):
            agg.record_batch(0.0, target, gen, target_norm, gen_norm, i_time_start=start)
    logs_on, logs_off = on.get_logs("inference"), off.get_logs("inference")
    order = [k for k in rec.windows[0][2] if k in spec]
    new = [f"inference/fss/{m}_r{r}/{name}/{k}" for k in order for name, _, _ in spec[k] for r in (0, 2) for m in fu.LOG_METRICS]
    assert [k for k in logs_on if k not in logs_off] == new and [k for k in logs_on if k in logs_off] == list(logs_off)
    assert list(none.get_logs("inference")) == list(logs_off)              # None: the parent's key list, in its order
    assert not any("/fss/" in k for k in logs_off) and not any("/fss/" in k or "/events/" in k for k in bare.get_logs("inference"))
    assert all(isinstance(logs_on[k], float) for k in new)
    seen = dict(M=3, B=2, H=32, W=64, names=list(rec.windows[0][2]), weights=w.cpu().numpy(), n_timesteps=n_total + 1, events=spec,
                radii=(0, 2), windows=[(s, {k: t[k].cpu().numpy() for k in out}, {k: g[k].cpu().numpy() for k in out})
                                       for s, t, g, _, _ in rec.windows])
    want, frac = fu.restate(seen, brute=True)
    data = on.get_fss_data()
    for k in out:
        for e, (name, _, _) in enumerate(spec[k]):
            for j, r in enumerate((0, 2)):
                assert tuple(data[f"sums_r{r}/{name}/{k}"].shape) == (n_total + 1, 32, 6)
                assert np.array_equal(data[f"sums_r{r}/{name}/{k}"].cpu().numpy(), want[k][:, e, j])
                assert want[k][0, e, j].sum() == 0 and (want[k][1:, e, j, :, 0] == 2 * 64).all()
    for key, v in fu.restate_logs(seen, frac, label="inference/fss").items():
        fu.close(logs_on[key], v, key)
    # at r = 0 the fractions Brier score is the event table's Brier score
    for k in order:
        for name, _, _ in spec[k]:
            assert abs(logs_on[f"inference/fss/fbs_r0/{name}/{k}"] - logs_on[f"inference/events/brier_score/{name}/{k}"]) <= fu.TOL
