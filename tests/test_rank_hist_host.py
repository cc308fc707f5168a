"""Host side of the ensemble rank histograms (no GPU): sdy_rank_hist_accumulate_host -- the header the kernel compiles
(csrc/rank_hist.h) -- against the numpy restatement on every case, what the entry points refuse by code, and what
`RankHistogramAggregator` refuses before it touches a device.  Cases and comparisons: tests/rank_hist_utils.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import rank_hist_utils as ru

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SDY_OK, SDY_ERR_ARG, SDY_ERR_UNSUPPORTED = 0, -1, -2


@pytest.fixture(scope="module")
def sdy():
    import sdy_amd

    return sdy_amd


@pytest.fixture(scope="module")
def cases():
    return ru.cases()


@pytest.mark.parametrize("name", ru.SMALL)
@pytest.mark.parametrize("pool", [False, True], ids=["slots", "pooled"])
def test_host_twin_against_restatement(sdy, cases, name, pool):
    case = cases[name]
    counts, ties = ru.host(case, pool)
    want_counts, want_ties = ru.restate(case, pool)
    assert np.array_equal(counts, want_counts) and np.array_equal(ties, want_ties)
    # every counted point is in exactly one bin; the first time of the run is in none
    finite = sum(int(np.isfinite(t[k][:, (1 if s == 0 else 0):]).sum()) for s, t, _ in case["windows"] for k in case["names"])
    assert counts.sum() == finite
    if not pool:
        assert (counts[:, 0] == 0).all() and (ties[:, 0] == 0).all() and (counts[:, 1:].sum(axis=(2, 3)) > 0).all()


def test_production_grid_host(sdy):
    case = ru.production_case()
    assert [(s, t["a"].shape) for s, t, _ in case["windows"]] == [(4, (1, 2, 180, 360))]
    counts, ties = ru.host(case)
    want_counts, want_ties = ru.restate(case)
    assert np.array_equal(counts, want_counts) and np.array_equal(ties, want_ties)
    assert counts.sum() == 2 * 2 * 180 * 360


def test_fixture_covers_what_it_claims(cases):
    assert list(cases) == list(ru.SMALL)
    assert cases["m2_b3_7x10"]["W"] % 4 != 0 and cases["m2_b3_7x10"]["H"] % 2 == 1          # the scalar path, odd H
    assert cases["m9_b1_4x36"]["M"] == 8 + 1 and cases["m9_b1_4x36"]["W"] // 4 == 9
    assert cases["m25_b1_4x360"]["M"] == 25 and cases["m25_b1_4x360"]["W"] // 4 == 90
    assert all(g.ndim == 4 for _, _, gen in cases["m1_b2_6x8"]["windows"] for g in gen.values())
    for case in cases.values():
        assert [(s, t["a"].shape[1]) for s, t, _ in case["windows"]] == [(0, 3), (3, 2)] and case["n_timesteps"] == 5
        assert (case["weights"] == case["weights"][:, :1]).all()


def test_known_answer(sdy, cases):
    """Member m is the constant field m and the target k - 0.5 on latitude k: row k holds all its points in bin k."""
    case = cases["known_m5_b2_6x8"]
    counts, ties = ru.host(case)
    per_row = case["B"] * case["W"]
    for slot in range(1, 5):
        assert np.array_equal(counts[:, slot], np.broadcast_to(per_row * np.eye(6), (2, 6, 6)))
    assert (ties == 0).all()
    logs = ru.restate_logs(case, counts, ties)
    assert logs["tie_fraction/a"] == 0.0 and 0.0 < logs["outlier_fraction/a"] < 1.0


def test_clipped_fields_tie(sdy, cases):
    """max(x, 0) for gen and target: about half the targets are 0 and nearly all of those meet a member at 0; a tie leaves
    the rank at the number of members strictly below (none is below 0)."""
    case = cases["clipped_m5_b2_6x8"]
    counts, ties = ru.host(case)
    total = counts.sum()
    assert 0.35 * total < ties.sum() < 0.65 * total
    assert counts[..., 0].sum() >= ties.sum() > 0


def test_nan_rules(sdy, cases):
    """A NaN target is counted nowhere, a NaN member is not below: poisoning one member of one point can only lower its rank."""
    case = cases["nan_m5_b2_6x8"]
    counts, _ = ru.host(case)
    counted = sum(int(np.isfinite(t[k][:, (1 if s == 0 else 0):]).sum()) for s, t, _ in case["windows"] for k in case["names"])
    points = sum(t[k][:, (1 if s == 0 else 0):].size for s, t, _ in case["windows"] for k in case["names"])
    assert counts.sum() == counted < points
    y = {"a": np.full((1, 1, 1, 4), 10.0, np.float32)}
    g = {"a": np.zeros((3, 1, 1, 1, 4), np.float32)}
    g["a"][1, 0, 0, 0, 2] = np.nan
    y["a"][0, 0, 0, 3] = np.nan
    one = dict(M=3, B=1, H=1, W=4, names=["a"], n_timesteps=6, windows=[(5, y, g)])
    c, t = ru.host(one)
    assert np.array_equal(c[0, 5, 0], [0, 0, 1, 2]) and t.sum() == 0


def test_first_time_of_a_run_is_dropped(sdy, cases):
    case = cases["m5_b2_6x8"]
    start, target, gen = case["windows"][0]
    bad_t, bad_g = {k: v.copy() for k, v in target.items()}, {k: v.copy() for k, v in gen.items()}
    for v in bad_t.values():
        v[:, 0] = np.nan
    for v in bad_g.values():
        v[:, :, 0] = 1e30
    want = ru.host(case, windows=[(0, target, gen)])
    got = ru.host(case, windows=[(0, bad_t, bad_g)])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and (want[0][:, 0] == 0).all()
    later = ru.host(case, windows=[(2, bad_t, bad_g)])                   # the same window later in a run: time 0 counts
    assert later[0][:, 2].sum() == 0 and later[0][:, 3].sum() > 0        # (its targets are NaN: counted nowhere)


def test_pooled_equals_the_slots_summed(sdy, cases):
    for name in ("m5_b2_6x8", "nan_m5_b2_6x8", "clipped_m5_b2_6x8"):
        counts, ties = ru.host(cases[name])
        pooled_counts, pooled_ties = ru.host(cases[name], pool=True)
        assert np.array_equal(pooled_counts[:, 0], counts.sum(axis=1)) and np.array_equal(pooled_ties[:, 0], ties.sum(axis=1))


def test_struct_is_in_the_handshake(sdy):
    from sdy_amd import _lib

    assert _lib.ABI_STRUCTS[-1] is _lib.SdyRankHistArgs and _lib.SDY_RANK_HIST_MAX_MEMBERS >= 64      # tests/test_capi_cpu.py
    hdr = open(os.path.join(ROOT, "include", "sdy_amd.h")).read()
    assert f"#define SDY_RANK_HIST_MAX_MEMBERS {_lib.SDY_RANK_HIST_MAX_MEMBERS}\n" in hdr


def _small_call(M=3, pool=False):
    rng = np.random.default_rng(3)
    target = {"a": rng.standard_normal((2, 3, 4, 6)).astype(np.float32)}
    gen = {"a": rng.standard_normal((M, 2, 3, 4, 6)).astype(np.float32)}
    n_slots = 1 if pool else 5
    counts, ties = np.full((1, n_slots, 4, M + 1), 7.0), np.full((1, n_slots, 4), 7.0)
    a, keep = ru.args(target, gen, ["a"], 1, 0, n_slots, pool, counts, ties)
    return a, keep, counts, ties


@pytest.mark.parametrize("field,value,code", [
    ("counts", None, SDY_ERR_ARG), ("ties", None, SDY_ERR_ARG),                            # NULL accumulators
    ("counts", "+4", SDY_ERR_ARG), ("ties", "+4", SDY_ERR_ARG),                            # off an 8-byte boundary
    ("t0", 4, SDY_ERR_ARG), ("t0", -1, SDY_ERR_ARG),                                       # t0 outside 0..T
    ("t_start", 3, SDY_ERR_ARG), ("t_start", -1, SDY_ERR_ARG), ("n_slots", 2, SDY_ERR_ARG),  # slot overflow
    ("n_slots", 0, SDY_ERR_ARG),
    ("gs0", -1, SDY_ERR_ARG), ("gs1", -4, SDY_ERR_ARG), ("ts1", -1, SDY_ERR_ARG),          # negative strides
    ("nvars", 0, SDY_ERR_ARG), ("nvars", 97, SDY_ERR_ARG),
    ("n0", 0, SDY_ERR_ARG), ("n1", -1, SDY_ERR_ARG), ("T", 0, SDY_ERR_ARG), ("H", 0, SDY_ERR_ARG), ("W", 0, SDY_ERR_ARG),
    ("gen0", None, SDY_ERR_ARG), ("target0", None, SDY_ERR_ARG),
    ("n0", 65, SDY_ERR_UNSUPPORTED),                                                       # M over the maximum
    (("T", "H", "W", "n_slots"), (2, 1 << 15, (1 << 14) + 1, 2), SDY_ERR_UNSUPPORTED),     # T * H * W > 2^30
    (("n0", "n1"), (1 << 16, 1 << 15), SDY_ERR_UNSUPPORTED),                               # n0 * n1 >= 2^31
    (("n1", "H", "W", "T", "n_slots"), (1 << 20, 1, 1 << 12, 1, 1), SDY_ERR_UNSUPPORTED),  # a row's points reach 2^32
    (("t_start", "n_slots", "H", "W"), (0, 1 << 30, 1 << 10, 4), SDY_ERR_UNSUPPORTED),     # n_slots * H reaches 2^40
])
def test_entry_points_refuse(sdy, field, value, code):
    a, keep, counts, ties = _small_call()
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
    assert sdy.lib.sdy_rank_hist_accumulate_host(C.byref(a)) == code
    assert sdy.lib.sdy_rank_hist_accumulate(C.byref(a), None) == code
    assert (counts == 7.0).all() and (ties == 7.0).all()
    assert sdy.lib.sdy_rank_hist_accumulate_host(None) == SDY_ERR_ARG and sdy.lib.sdy_rank_hist_accumulate(None, None) == SDY_ERR_ARG


def test_pooled_entry_point_takes_one_slot_only(sdy):
    a, keep, counts, ties = _small_call(pool=True)
    a.t_start = 1000                                      # not looked at when the times are pooled
    assert sdy.lib.sdy_rank_hist_accumulate_host(C.byref(a)) == SDY_OK and counts.sum() == 7.0 * counts.size + 2 * 2 * 4 * 6
    a.n_slots = 2
    assert sdy.lib.sdy_rank_hist_accumulate_host(C.byref(a)) == SDY_ERR_ARG
    assert sdy.lib.sdy_rank_hist_accumulate(C.byref(a), None) == SDY_ERR_ARG


def test_a_window_without_counted_times_is_ok_and_changes_nothing(sdy):
    """T - t0 == 0 (a window that holds the initial condition only): SDY_OK from both entry points -- the device one launches
    nothing, so it needs no device."""
    a, keep, counts, ties = _small_call()
    a.t0 = a.T
    assert sdy.lib.sdy_rank_hist_accumulate_host(C.byref(a)) == SDY_OK
    assert sdy.lib.sdy_rank_hist_accumulate(C.byref(a), None) == SDY_OK
    assert (counts == 7.0).all() and (ties == 7.0).all()


def test_the_maximum_member_count_is_taken(sdy):
    rng = np.random.default_rng(11)
    y = {"a": rng.standard_normal((1, 1, 2, 5)).astype(np.float32)}
    g = {"a": rng.standard_normal((64, 1, 1, 2, 5)).astype(np.float32)}
    case = dict(M=64, B=1, H=2, W=5, names=["a"], n_timesteps=3, windows=[(2, y, g)])
    got, want = ru.host(case), ru.restate(case)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[0].sum() == 10


# ---- the Python class, as far as it goes without a device -----------------------------------------------------------------
def _window(M=3, B=2, T=3, H=4, W=6, names=("a", "b")):
    g = torch.Generator().manual_seed(0)
    target = {k: torch.randn(B, T, H, W, generator=g) for k in names}
    gen = {k: torch.randn(M, B, T, H, W, generator=g) for k in names}
    return target, gen


def _record(agg, target, gen, **kw):
    agg.record_batch(loss=0.0, target_data=target, gen_data=gen, target_data_norm=target, gen_data_norm=gen, **kw)


def test_class_refuses_weights_that_vary_along_a_row(sdy):
    w = torch.ones(4, 6)
    sdy.RankHistogramAggregator(w * torch.arange(1.0, 5.0)[:, None], n_timesteps=3)         # constant along each row
    w[2, 3] = 1.5
    with pytest.raises(ValueError, match="vary along a latitude row"):
        sdy.RankHistogramAggregator(w, n_timesteps=3)
    with pytest.raises(ValueError, match="n_timesteps must be positive"):
        sdy.RankHistogramAggregator(torch.ones(4, 6), n_timesteps=0)


def test_class_refuses_cpu_tensors(sdy):
    agg = sdy.RankHistogramAggregator(torch.ones(4, 6), n_timesteps=3)
    before = dict(vars(agg))
    with pytest.raises(RuntimeError, match="GPU only"):
        _record(agg, *_window())
    assert vars(agg) == before and agg._names is None              # a refused window changes nothing
    with pytest.raises(ValueError, match="No data recorded"):
        agg.get_logs("x")
    with pytest.raises(ValueError, match="No data recorded"):
        agg.get_data()


def test_class_refuses_ragged_shares(sdy):
    agg = sdy.RankHistogramAggregator(torch.ones(4, 6), n_timesteps=3)
    target, gen = _window()
    flat = {k: v.reshape(-1, *v.shape[2:])[:5] for k, v in gen.items()}       # 5 rows of 3 members x 2 samples
    with pytest.raises(ValueError, match="RankHistogramAggregator needs member-stacked"):
        _record(agg, target, flat)
    with pytest.raises(ValueError, match="member-stacked"):
        _record(agg, {k: v[:1] for k, v in target.items()}, {k: v[:1] for k, v in flat.items()}, sample_weights=[1 / 3])
    assert agg._names is None


def test_class_checks_the_slots_as_the_other_aggregators_do(sdy):
    for pool in (False, True):
        agg = sdy.RankHistogramAggregator(torch.ones(4, 6), n_timesteps=4, pool_times=pool)
        with pytest.raises(ValueError, match="times 2..4 outside the aggregator's 4"):
            _record(agg, *_window(), i_time_start=2)
        with pytest.raises(ValueError, match="outside the aggregator's 4"):
            _record(agg, *_window(), i_time_start=-1)
        with pytest.raises(RuntimeError, match="GPU only"):            # inside: gets as far as the device check
            _record(agg, *_window(), i_time_start=1)
    with pytest.raises(ValueError, match="at most 64 members, got 65"):
        _record(agg, *_window(M=65, B=1, T=1, H=4, W=6, names=("a",)))


def test_class_refuses_another_job(sdy):
    """What record_batch compares a later window with, on host tensors: the variable set, the member count, the sample count
    and the grid -- another member count is another job.  (Through the class on a device, accumulators unchanged:
    tests/test_gpu_rank_hist.py.)"""
    from sdy_amd.windows import check_same_job, window_layouts

    def job(**kw):
        target, gen = _window(**kw)
        return list(gen), [sdy.RankHistogramAggregator._job(l) for l in window_layouts(target, gen)]

    words = sdy.RankHistogramAggregator._job_words
    first = job()
    assert first[1] == [(3, 2, 4, 6)] * 2
    check_same_job(*job(T=2), *first, words)                       # another number of times is the same job
    for other in (dict(names=("a", "c")), dict(names=("a",)), dict(M=4), dict(B=3), dict(H=5)):
        with pytest.raises(ValueError, match="member count, sample count or grids of a window differ from the first window"):
            check_same_job(*job(**other), *first, words)


def test_class_sizes_its_accumulators(sdy):
    need = 8 * 2 * (3 * 4 * (3 + 1) + 3 * 4)                        # counts (slots, lat, M + 1) and ties (slots, lat), 2 variables
    agg = sdy.RankHistogramAggregator(torch.ones(4, 6), n_timesteps=3, max_bytes=need - 1)
    with pytest.raises(ValueError, match=f"need {need} bytes"):
        _record(agg, *_window())
    pooled = sdy.RankHistogramAggregator(torch.ones(4, 6), n_timesteps=3, pool_times=True, max_bytes=need // 3)
    with pytest.raises(RuntimeError, match="GPU only"):            # one slot: a third of the bytes is enough
        _record(pooled, *_window())


def test_inference_aggregator_option_is_off_by_default(sdy):
    w = torch.ones(4, 6)
    assert "rank_histogram" not in sdy.metrics.InferenceAggregator(w, n_timesteps=3, n_ensemble_members=2)._aggregators
    agg = sdy.metrics.InferenceAggregator(w, n_timesteps=3, n_ensemble_members=2, rank_histogram_data=True)
    rank = agg._aggregators["rank_histogram"]
    assert isinstance(rank, sdy.RankHistogramAggregator) and rank._n_slots == 3 and list(agg._aggregators)[-1] == "rank_histogram"
    agg = sdy.metrics.InferenceAggregator(w, n_timesteps=3, n_ensemble_members=2, rank_histogram_data=True,
                                          rank_histogram_pool_times=True)
    assert agg._aggregators["rank_histogram"]._n_slots == 1
