"""Ensemble time-mean statistics on the device (`sdy_amd.EnsembleTimeMeanAggregator`; kernels of csrc/member_mean.hip) against
the reference's own ensemble TimeMeanAggregator (tests/golden/fx_time_mean_ensemble.npz), the library's _host twins and the
float64 restatement; layouts, batch independence, determinism, the production grid, one member, spread, and the way through
run_inference.  Bounds: tests/member_mean_utils.py.  Every case is a handful of launches."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import member_mean_utils as mu

pytestmark = pytest.mark.gpu

CASES = ("m3_b2_6x8", "m2_b3_7x10", "m25_b1_16x32", "m5_b2_18x36")


@pytest.fixture(scope="module")
def cases():
    return mu.cases()


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


def _run(case, layout=_contiguous, windows=None, spread=False, target_layout=_contiguous):
    import sdy_amd

    agg = sdy_amd.EnsembleTimeMeanAggregator(torch.from_numpy(case["weights"]).cuda(), spread=spread)
    for start, target, gen in (case["windows"] if windows is None else windows):
        agg.record_batch(0.0, {k: target_layout(v) for k, v in target.items()}, {k: layout(v) for k, v in gen.items()},
                         i_time_start=start)
    return agg


def _sums(agg, case):
    n, M, B, H, W = len(case["names"]), case["M"], case["B"], case["H"], case["W"]
    return agg._gen_sum.view(n, M, B, H, W).cpu().numpy(), agg._target_sum.view(n, B, H, W).cpu().numpy()


def _raw(agg):
    sums = agg.weighted_sums()
    return np.stack([sums[k].cpu().numpy() for k in agg._names])


def _weight_total(case):
    return case["B"] * float(case["weights"].astype(np.float64).sum())


@pytest.mark.parametrize("name", CASES)
def test_against_reference_and_host(cases, name):
    case = cases[name]
    agg = _run(case)
    logs = agg.get_logs("")
    assert all(isinstance(v, float) for v in logs.values())
    mu.check_against_reference(case, logs, f"device {name}")          # (the reference's key order included)
    assert list(agg.get_logs("full")) == [f"full/{k}" for k in case["keys"]]
    gen_sum, target_sum = _sums(agg, case)
    host_gen, host_target, n_times = mu.host_sums(case)
    assert agg._n_times == n_times == case["S"]
    assert np.array_equal(gen_sum, host_gen) and np.array_equal(target_sum, host_target)
    host_raw = mu.host_stats(host_gen, host_target, case["weights"], n_times)
    _, scales = mu.restate_stats(host_gen, host_target, case["weights"], n_times)
    mu.check_raw(_raw(agg), host_raw, scales, _weight_total(case), f"device vs host {name}")
    maps = agg.time_mean_maps()
    for j, k in enumerate(case["names"]):
        assert maps["gen"][k].dtype == torch.float64 and tuple(maps["gen"][k].shape) == gen_sum.shape[1:]
        assert np.array_equal(maps["gen"][k].cpu().numpy(), host_gen[j] / n_times)
        assert np.array_equal(maps["target"][k].cpu().numpy(), host_target[j] / n_times)


def test_layouts_give_the_same_bits(cases):
    """Contiguous, the transposed view of a (samples, members, ...) buffer, and a view one element into a larger buffer
    (scalar loads): the order of every sum is fixed, so the accumulators are bit-identical."""
    case = cases["m5_b2_18x36"]
    ref = _sums(_run(case), case)
    for layout, target_layout in ((_transposed, _contiguous), (_offset, _contiguous), (_offset, _offset)):
        got = _sums(_run(case, layout, target_layout=target_layout), case)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), layout.__name__


def test_batch_independence(cases):
    """Sample 0's accumulators from the B = 2 run equal those of a run on sample 0 alone, bit for bit."""
    case = cases["m5_b2_18x36"]
    both = _sums(_run(case), case)
    one = dict(case, B=1, windows=[(s, {k: v[:1] for k, v in t.items()}, {k: v[:, :1] for k, v in g.items()})
                                   for s, t, g in case["windows"]])
    alone = _sums(_run(one), one)
    assert np.array_equal(both[0][:, :, :1], alone[0]) and np.array_equal(both[1][:, :1], alone[1])


def test_a_later_window_of_another_job_is_refused(cases):
    """Through the class on the device: another variable set or member count raises and leaves the accumulators alone."""
    case = cases["m3_b2_6x8"]
    agg = _run(case)
    before = _sums(agg, case)
    start, target, gen = case["windows"][1]
    dev = lambda d: {k: _contiguous(v) for k, v in d.items()}  # noqa: E731
    with pytest.raises(ValueError, match="differ from the first window"):
        agg.record_batch(0.0, dev({"a": target["a"], "c": target["b"]}), dev({"a": gen["a"], "c": gen["b"]}), i_time_start=9)
    with pytest.raises(ValueError, match="differ from the first window"):
        agg.record_batch(0.0, dev(target), dev({k: v[:2] for k, v in gen.items()}), i_time_start=9)
    after = _sums(agg, case)
    assert agg._n_times == case["S"] and np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_two_runs_give_the_same_logs(cases):
    case = cases["m25_b1_16x32"]
    a, b = _run(case, spread=True).get_logs("x"), _run(case, spread=True).get_logs("x")
    assert list(a) == list(b) and all(a[k] == b[k] for k in a)


def test_production_grid():
    """180 x 360, 3 members, two variables, windows of 3 and 2 times, from seeded numpy: device against the host twin (sums:
    the same bits) and the restatement.  The aligned run takes 16-byte loads; the run from views one element into a larger
    buffer takes scalar loads, with more items than the capped grid has threads: the stride loop."""
    case = mu.seeded_case(3, 1, 180, 360, (2, 2), ("a", "b"), seed=20260)
    assert [w[1]["a"].shape[1] for w in case["windows"]] == [3, 2]
    host_gen, host_target, n_times = mu.host_sums(case)
    want_gen, want_target, _ = mu.restate_sums(case)
    assert np.array_equal(host_gen, want_gen) and np.array_equal(host_target, want_target)
    host_raw = mu.host_stats(host_gen, host_target, case["weights"], n_times)
    want_raw, scales = mu.restate_stats(host_gen, host_target, case["weights"], n_times)
    want_logs = mu.logs_from_raw(want_raw, case["names"], 1, case["weights"])
    for layout in (_contiguous, _offset):
        agg = _run(case, layout, target_layout=layout)
        gen_sum, target_sum = _sums(agg, case)
        assert np.array_equal(gen_sum, host_gen) and np.array_equal(target_sum, host_target), layout.__name__
        raw = _raw(agg)
        mu.check_raw(raw, host_raw, scales, _weight_total(case), f"production {layout.__name__} vs host")
        mu.check_raw(raw, want_raw, scales, _weight_total(case), f"production {layout.__name__} vs restatement")
        mu.check_logs(case, agg.get_logs(""), want_logs, 1e-12, f"production {layout.__name__}", scales=scales)


def test_one_member_from_flat_rows():
    """A 4-D gen is one member: `rmse` and `bias` only, equal to TimeMeanAggregator's on the same windows (one sample, windows
    of equal length: there the two classes define the same numbers).  TimeMeanAggregator keeps fp32 maps: a map element is an
    fp32 sum of S values scaled and added over windows, (S + 4) u max|x| per map and twice that for gen - target =: delta; the
    bias moves by delta, the mean square by 2 max|g - t| delta + delta^2."""
    import sdy_amd

    case = mu.seeded_case(1, 1, 16, 32, (2, 2), ("a", "b"), seed=7)
    flat = [(s, t, {k: v[0] for k, v in g.items()}) for s, t, g in case["windows"]]
    agg = _run(case, windows=flat)
    logs = agg.get_logs("")
    assert list(logs) == ["rmse/a", "bias/a", "rmse/b", "bias/b"]
    assert tuple(agg.time_mean_maps()["gen"]["a"].shape) == (1, 1, 16, 32)
    old = sdy_amd.metrics.TimeMeanAggregator(torch.from_numpy(case["weights"]).cuda())
    for s, t, g in flat:
        t, g = {k: _contiguous(v) for k, v in t.items()}, {k: _contiguous(v) for k, v in g.items()}
        old.record_batch(0.0, t, g, t, g, i_time_start=s)
    old_logs = old.get_logs("")
    _, scales, xmax = mu.restate(case)
    delta = 2 * (case["S"] + 4) * mu.U * xmax
    for j, k in enumerate(case["names"]):
        mu._within(logs[f"bias/{k}"], old_logs[f"bias/{k}"], delta, f"bias/{k} vs TimeMeanAggregator")
        mu._within(logs[f"rmse/{k}"] ** 2, old_logs[f"rmse/{k}"] ** 2, 2 * scales[j]["abs"] * delta + delta ** 2,
                   f"(rmse/{k})^2 vs TimeMeanAggregator")
    want, _, _ = mu.restate(case)
    mu.check_logs(case, logs, want, 1e-12, "one member vs restatement", scales=scales)


@pytest.mark.parametrize("name", ["m3_b2_6x8", "m25_b1_16x32"])
def test_spread_and_ssr(cases, name):
    case = cases[name]
    logs = _run(case, spread=True).get_logs("")
    want, _, _ = mu.restate(case, spread=True)
    assert list(logs) == list(want)
    mu.check_spread(case, logs, want, f"device {name}")
    mu.check_against_reference(case, logs, f"device {name} with spread")


class _Recorder:
    """Hands every window on and keeps a copy of what it saw."""

    accepts_sample_weights = True

    def __init__(self, inner):
        self.inner, self.windows = inner, []

    def record_batch(self, loss, target_data, gen_data, target_data_norm, gen_data_norm, i_time_start=0, **kw):
        self.windows.append((i_time_start, {k: v.clone() for k, v in target_data.items()},
                             {k: v.clone() for k, v in gen_data.items()}))
        self.inner.record_batch(loss=loss, target_data=target_data, gen_data=gen_data, target_data_norm=target_data_norm,
                                gen_data_norm=gen_data_norm, i_time_start=i_time_start, **kw)


def test_through_run_inference():
    """run_inference on the tiny loop fixture (2 windows x 6 steps, 2 samples, 3 members): the maps are the member-wise time
    means of the windows the run produced (its first time, the initial condition, not counted), the logs carry the new keys
    under time_mean_ensemble, and the default key set is unchanged."""
    import sdy_amd
    from test_gpu_derived import _loop_setup

    _, stepper, windows, sigma, n_total, n_mem, names = _loop_setup(3)
    w = sdy_amd.metrics.spherical_area_weights(torch.linspace(-87.0, 87.0, 32), 64).cuda()
    logs, rec = {}, None
    for on in (False, True):
        agg = sdy_amd.metrics.InferenceAggregator(w, n_timesteps=n_total + 1, n_ensemble_members=3, ensemble_time_mean_data=on,
                                                  ensemble_time_mean_spread=on)
        rec = _Recorder(agg)
        sdy_amd.run_inference(rec, stepper, types.SimpleNamespace(loader=windows), n_total, n_mem, 3)
        logs[on] = agg.get_logs("inference")
    out = names["out_names"]
    new = {f"inference/time_mean_ensemble/{lab}/{n}" for n in out
           for lab in ("rmse_member_avg", "bias_member_avg", "rmse", "bias", "crps", "spread", "ssr")}
    assert set(logs[True]) - set(logs[False]) == new and set(logs[False]) <= set(logs[True])
    assert all(isinstance(logs[True][k], float) and np.isfinite(logs[True][k]) for k in new)
    # the values: the restatement of the (denormalised) windows the run handed over, under the composite's labels
    seen = dict(M=3, B=2, H=32, W=64, names=out, weights=w.cpu().numpy(), S=n_total,
                windows=[(s, {k: t[k].cpu().numpy() for k in out}, {k: g[k].cpu().numpy() for k in out})
                         for s, t, g in rec.windows])
    want, scales, _ = mu.restate(seen, spread=True)
    got = {k: logs[True][f"inference/time_mean_ensemble/{k}"] for k in want}
    mu.check_logs(seen, got, {k: v for k, v in want.items() if mu._kind(k) not in ("spread", "ssr")}, 1e-12,
                  "run_inference vs restatement", scales=scales)
    mu.check_spread(seen, got, want, "run_inference")
    maps = agg.get_ensemble_time_mean_maps()
    assert list(maps["gen"]) == out and list(maps["target"]) == out
    counted = 0
    sums = {}
    for start, target, gen in rec.windows:
        t0 = 1 if start == 0 else 0
        for n in out:
            assert gen[n].dim() == 5 and gen[n].shape[0] == 3
            sg = torch.zeros_like(gen[n][:, :, 0], dtype=torch.float64)
            st = torch.zeros_like(target[n][:, 0], dtype=torch.float64)
            for t in range(t0, gen[n].shape[2]):
                sg += gen[n][:, :, t].double()
                st += target[n][:, t].double()
            sums[n] = (sums[n][0] + sg, sums[n][1] + st) if n in sums else (sg, st)
        counted += gen[out[0]].shape[2] - t0
    assert counted == n_total
    div = torch.full((), float(counted), dtype=torch.float64, device="cuda")      # (a true division: see time_mean_maps)
    for n in out:
        assert tuple(maps["gen"][n].shape) == (3, 2, 32, 64)
        assert torch.equal(maps["gen"][n], sums[n][0] / div) and torch.equal(maps["target"][n], sums[n][1] / div)
