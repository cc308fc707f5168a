"""Host side of the ensemble time-mean statistics (no GPU): sdy_member_time_sum_host / sdy_member_map_stats_host -- the header
the kernels compile (csrc/member_mean.h) -- against the reference's own ensemble TimeMeanAggregator
(tests/golden/fx_time_mean_ensemble.npz), what the entry points refuse, and what `EnsembleTimeMeanAggregator` refuses before it
touches a device.  Bounds: tests/member_mean_utils.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import member_mean_utils as mu

SDY_ERR_ARG, SDY_ERR_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def sdy():
    import sdy_amd

    return sdy_amd


@pytest.fixture(scope="module")
def cases():
    return mu.cases()


CASES = ("m3_b2_6x8", "m2_b3_7x10", "m25_b1_16x32", "m5_b2_18x36")


@pytest.mark.parametrize("name", CASES)
def test_host_twins_against_reference(sdy, cases, name):
    case = cases[name]
    gen_sum, target_sum, n_times = mu.host_sums(case)
    want = mu.restate_sums(case)
    assert n_times == want[2] == case["S"]
    assert np.array_equal(gen_sum, want[0]) and np.array_equal(target_sum, want[1])      # a fixed order: the same bits
    raw = mu.host_stats(gen_sum, target_sum, case["weights"], n_times)
    logs = mu.logs_from_raw(raw, case["names"], case["B"], case["weights"])
    mu.check_against_reference(case, logs, f"host {name}")
    want_raw, scales = mu.restate_stats(gen_sum, target_sum, case["weights"], n_times)
    mu.check_raw(raw, want_raw, scales, case["B"] * float(case["weights"].astype(np.float64).sum()), f"host {name} vs restatement")


def test_fixture_covers_what_it_claims(cases):
    assert list(cases) == list(CASES)
    assert cases["m2_b3_7x10"]["H"] * cases["m2_b3_7x10"]["W"] % 4 != 0                   # the scalar path
    assert cases["m25_b1_16x32"]["M"] == 25
    assert [w[1]["a"].shape[1] for w in cases["m5_b2_18x36"]["windows"]] == [4, 2, 2]     # 3 + 2 + 2 counted
    for case in cases.values():
        assert case["windows"][0][0] == 0 and all(w[0] > 0 for w in case["windows"][1:])


def test_first_time_of_a_run_is_dropped(sdy, cases):
    case = cases["m3_b2_6x8"]
    start, target, gen = case["windows"][0]
    one = dict(case, windows=[(0, target, gen)])
    gen_sum, target_sum, n = mu.host_sums(one)
    T = target["a"].shape[1]
    assert n == T - 1
    assert np.array_equal(target_sum[0], target["a"][:, 1:].astype(np.float64).sum(axis=1))
    assert np.array_equal(gen_sum[0], gen["a"][:, :, 1:].astype(np.float64).sum(axis=2))
    # the same window later in a run counts every time; poisoning time 0 shows in it and not in the first
    bad_t = {k: v.copy() for k, v in target.items()}
    bad_g = {k: v.copy() for k, v in gen.items()}
    for d in (bad_t, bad_g):
        for v in d.values():
            v[..., 0, :, :] = np.nan
    g2, t2, _ = mu.host_sums(dict(case, windows=[(0, bad_t, bad_g)]))
    assert np.array_equal(g2, gen_sum) and np.array_equal(t2, target_sum)
    g3, t3, n3 = mu.host_sums(dict(case, windows=[(5, bad_t, bad_g)]))
    assert n3 == T and np.isnan(g3).all() and np.isnan(t3).all()


def test_struct_sizes(sdy):
    from sdy_amd import _lib

    assert _lib.SdyMemberSumArgs in _lib.ABI_STRUCTS and _lib.SdyMemberStatsArgs in _lib.ABI_STRUCTS   # tests/test_capi_cpu.py
    assert _lib.SDY_MEMBER_STATS_MAX_MEMBERS == 64


def _small_sum_call():
    rng = np.random.default_rng(3)
    target = {"a": rng.standard_normal((2, 3, 4, 6)).astype(np.float32)}
    gen = {"a": rng.standard_normal((3, 2, 3, 4, 6)).astype(np.float32)}
    gen_sum, target_sum = np.full((1, 3, 2, 4, 6), 7.0), np.full((1, 2, 4, 6), 7.0)
    a, keep = mu.sum_args(target, gen, ["a"], 1, gen_sum, target_sum)
    return a, keep, gen_sum, target_sum


@pytest.mark.parametrize("field,value,code", [
    ("nvars", 0, SDY_ERR_ARG), ("nvars", 97, SDY_ERR_ARG), ("n0", 0, SDY_ERR_ARG), ("n1", -1, SDY_ERR_ARG),
    ("T", 0, SDY_ERR_ARG), ("HW", 0, SDY_ERR_ARG), ("gs0", -1, SDY_ERR_ARG), ("gs1", -4, SDY_ERR_ARG), ("ts1", -1, SDY_ERR_ARG),
    ("t0", -1, SDY_ERR_ARG), ("t0", 3, SDY_ERR_ARG), ("gen_sum", None, SDY_ERR_ARG), ("target_sum", None, SDY_ERR_ARG),
    ("gen0", None, SDY_ERR_ARG), ("target0", None, SDY_ERR_ARG),
    ("gen_sum", "+4", SDY_ERR_ARG), ("target_sum", "+4", SDY_ERR_ARG),           # accumulators off an 8-byte boundary
    (("T", "HW"), (2, (1 << 29) + 1), SDY_ERR_UNSUPPORTED),            # T * HW > 2^30
    (("n0", "n1"), (1 << 16, 1 << 15), SDY_ERR_UNSUPPORTED),           # n0 * n1 >= 2^31
    (("n0", "n1", "T", "HW", "t0"), (1 << 20, 1 << 10, 1, 1 << 20, 0), SDY_ERR_UNSUPPORTED),   # accumulator index reaches 2^50
])
def test_sum_entry_point_refuses(sdy, field, value, code):
    a, keep, gen_sum, target_sum = _small_sum_call()
    if field == "gen0":
        a.gen[0] = None
    elif field == "target0":
        a.target[0] = None
    elif isinstance(field, tuple):
        for f, v in zip(field, value):
            setattr(a, f, v)
    elif value == "+4":
        setattr(a, field, getattr(a, field) + 4)
    else:
        setattr(a, field, value)
    # both entry points check before anything else: the device one is refused without a device
    assert sdy.lib.sdy_member_time_sum_host(C.byref(a)) == code
    assert sdy.lib.sdy_member_time_sum(C.byref(a), None) == code
    assert (gen_sum == 7.0).all() and (target_sum == 7.0).all()
    assert sdy.lib.sdy_member_time_sum_host(None) == SDY_ERR_ARG


def _small_stats_call(M=3):
    rng = np.random.default_rng(5)
    gen_sum, target_sum = rng.standard_normal((2, M, 2, 4, 6)), rng.standard_normal((2, 2, 4, 6))
    out = np.full((2, 2 * M + 4), 7.0)
    a, keep = mu.stats_args(gen_sum, target_sum, np.ones((4, 6), np.float32), 3, out)
    return a, keep + [gen_sum, target_sum], out


@pytest.mark.parametrize("field,value,code", [
    ("nvars", 0, SDY_ERR_ARG), ("M", 0, SDY_ERR_ARG), ("n1", 0, SDY_ERR_ARG), ("HW", -2, SDY_ERR_ARG),
    ("gen_sum", None, SDY_ERR_ARG), ("target_sum", None, SDY_ERR_ARG), ("weights", None, SDY_ERR_ARG), ("out", None, SDY_ERR_ARG),
    ("n_times", 0.0, SDY_ERR_ARG), ("n_times", float("nan"), SDY_ERR_ARG),
    ("gen_sum", "+4", SDY_ERR_ARG), ("target_sum", "+4", SDY_ERR_ARG), ("out", "+4", SDY_ERR_ARG),
    ("M", 65, SDY_ERR_UNSUPPORTED), ("nvars", 65536, SDY_ERR_UNSUPPORTED),
    (("n1", "HW"), (1 << 10, (1 << 20) + 1), SDY_ERR_UNSUPPORTED),
    (("nvars", "M", "n1", "HW"), (1 << 14, 64, 1 << 10, 1 << 20), SDY_ERR_UNSUPPORTED),   # nvars M n1 HW reaches 2^50
])
def test_stats_entry_point_refuses(sdy, field, value, code):
    a, keep, out = _small_stats_call()
    for f, v in zip(field, value) if isinstance(field, tuple) else ((field, value),):
        setattr(a, f, getattr(a, f) + 4 if v == "+4" else v)
    assert sdy.lib.sdy_member_map_stats_host(C.byref(a)) == code
    assert (out == 7.0).all()
    assert sdy.lib.sdy_member_map_stats_host(None) == SDY_ERR_ARG


def test_stats_device_entry_point_needs_its_workspace(sdy):
    a, keep, out = _small_stats_call()
    need = sdy.lib.sdy_member_stats_workspace_bytes(2, 3, 2, 24)
    assert need == 2 * 1 * 10 * 8                       # one block of 256 points per variable, 2 M + 4 doubles
    assert sdy.lib.sdy_member_stats_workspace_bytes(2, 65, 2, 24) == 0
    assert sdy.lib.sdy_member_map_stats(C.byref(a), None) == SDY_ERR_ARG             # ws NULL
    ws = np.zeros(need // 8)
    a.ws, a.ws_bytes = ws.ctypes.data_as(C.c_void_p).value, need - 8
    assert sdy.lib.sdy_member_map_stats(C.byref(a), None) == SDY_ERR_ARG             # ws too small
    spare = np.zeros(need // 8 + 1)
    a.ws, a.ws_bytes = spare.ctypes.data_as(C.c_void_p).value + 4, need
    assert sdy.lib.sdy_member_map_stats(C.byref(a), None) == SDY_ERR_ARG             # ws off an 8-byte boundary
    assert (out == 7.0).all()


def test_one_member(sdy):
    """M == 1: CRPS = |g - t|, variance 0, and the ensemble mean is the member."""
    rng = np.random.default_rng(9)
    gen_sum, target_sum = rng.standard_normal((1, 1, 2, 5, 7)), rng.standard_normal((1, 2, 5, 7))
    w = (1.0 + rng.random((5, 7))).astype(np.float32)
    raw = mu.host_stats(gen_sum, target_sum, w, 4)
    d = (gen_sum[0, 0] - target_sum[0]) / 4
    w64 = w.astype(np.float64)
    want = np.array([(w64 * d * d).sum(), (w64 * d).sum(), (w64 * d * d).sum(), (w64 * d).sum(), (w64 * np.abs(d)).sum(), 0.0])
    assert raw[0, 5] == 0.0 and raw[0, 0] == raw[0, 2] and raw[0, 1] == raw[0, 3]
    assert np.allclose(raw[0], want, rtol=1e-13, atol=0.0)


# ---- the Python class, as far as it goes without a device -----------------------------------------------------------------
def _window(M=3, B=2, T=3, H=4, W=6, names=("a", "b")):
    g = torch.Generator().manual_seed(0)
    target = {k: torch.randn(B, T, H, W, generator=g) for k in names}
    gen = {k: torch.randn(M, B, T, H, W, generator=g) for k in names}
    return target, gen


def _record(agg, target, gen, **kw):
    agg.record_batch(loss=0.0, target_data=target, gen_data=gen, target_data_norm=target, gen_data_norm=gen, **kw)


def test_class_refuses_cpu_tensors(sdy):
    agg = sdy.EnsembleTimeMeanAggregator(torch.ones(4, 6))
    with pytest.raises(RuntimeError, match="GPU only"):
        _record(agg, *_window())
    with pytest.raises(ValueError, match="No data recorded"):
        agg.get_logs("x")


def test_class_refuses_another_job(sdy):
    """What record_batch compares a later window with (`EnsembleTimeMeanAggregator._job` of every layout, `check_same_job`),
    on host tensors: the variable set, the member count, the sample count and the grid.  (Through the class on a device:
    tests/test_gpu_member_mean.py.)"""
    from sdy_amd.windows import check_same_job, window_layouts

    def job(**kw):
        target, gen = _window(**kw)
        return list(gen), [sdy.EnsembleTimeMeanAggregator._job(l) for l in window_layouts(target, gen)]

    words = sdy.EnsembleTimeMeanAggregator._job_words
    first = job()
    assert first[1] == [(3, 2, 4, 6)] * 2
    check_same_job(*job(T=2), *first, words)                       # another number of times is the same job
    for other in (dict(names=("a", "c")), dict(names=("b", "a")), dict(names=("a",)), dict(M=4), dict(B=3), dict(H=5)):
        with pytest.raises(ValueError, match="member count, sample count or grids of a window differ from the first window"):
            check_same_job(*job(**other), *first, words)


def test_a_refused_window_changes_nothing(sdy):
    agg = sdy.EnsembleTimeMeanAggregator(torch.ones(4, 6))
    before = dict(vars(agg))
    with pytest.raises(RuntimeError, match="GPU only"):
        _record(agg, *_window())
    assert vars(agg) == before and agg._names is None
    with pytest.raises(RuntimeError, match="GPU only"):            # no job was fixed: other variables get as far again
        _record(agg, *_window(names=("a", "c"), M=4))


def test_class_refuses_accumulators_over_max_bytes(sdy):
    need = 8 * 2 * (2 * 4 * 6) * (3 + 1)
    agg = sdy.EnsembleTimeMeanAggregator(torch.ones(4, 6), max_bytes=need - 1)
    with pytest.raises(ValueError, match=f"need {need} bytes"):
        _record(agg, *_window())
    agg = sdy.EnsembleTimeMeanAggregator(torch.ones(4, 6), max_bytes=need)
    with pytest.raises(RuntimeError, match="GPU only"):
        _record(agg, *_window())


def test_class_refuses_ragged_shares(sdy):
    agg = sdy.EnsembleTimeMeanAggregator(torch.ones(4, 6))
    target, gen = _window()
    flat = {k: v.reshape(-1, *v.shape[2:])[:5] for k, v in gen.items()}       # 5 rows of 3 members x 2 samples
    with pytest.raises(ValueError, match="member-stacked") as e:
        _record(agg, target, flat)
    with pytest.raises(ValueError, match="member-stacked"):
        _record(agg, {k: v[:1] for k, v in target.items()}, {k: v[:1] for k, v in flat.items()}, sample_weights=[1 / 3])
    mean = sdy.metrics.MeanAggregator(torch.ones(4, 6), is_ensemble=True)
    with pytest.raises(ValueError) as e2:
        _record(mean, target, flat)
    assert str(e.value).split(" needs ", 1)[1] == str(e2.value).split(" needs ", 1)[1]          # MeanAggregator's message


def test_inference_aggregator_option_is_off_by_default(sdy):
    w = torch.ones(4, 6)
    assert "time_mean_ensemble" not in sdy.metrics.InferenceAggregator(w, n_timesteps=3, n_ensemble_members=2)._aggregators
    agg = sdy.metrics.InferenceAggregator(w, n_timesteps=3, n_ensemble_members=2, ensemble_time_mean_data=True)
    assert isinstance(agg._aggregators["time_mean_ensemble"], sdy.EnsembleTimeMeanAggregator)
