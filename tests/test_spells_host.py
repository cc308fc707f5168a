"""Host side of the spell-duration statistics (no GPU): sdy_event_spell_accumulate_host -- the header the kernel compiles
(csrc/spells.h) -- against the numpy restatement on every case and under every cut of the run into windows, the bin of a
duration, what the entry points refuse, the log arithmetic as a pure function of `rows`, and what `EventSpellAggregator` and
`InferenceAggregator(event_spells=True)` refuse before they touch a device.  Cases and comparisons: tests/spell_utils.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import spell_utils as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SDY_OK, SDY_ERR_ARG, SDY_ERR_UNSUPPORTED = 0, -1, -2


@pytest.fixture(scope="module")
def sdy():
    import sdy_amd

    return sdy_amd


@pytest.fixture(scope="module")
def cases():
    return su.cases()


@pytest.fixture(scope="module")
def wanted(cases):
    return {name: su.restate(case) for name, case in cases.items()}


@pytest.mark.parametrize("name", su.SMALL)
def test_host_twin_against_restatement(sdy, cases, wanted, name):
    case = cases[name]
    states, closed = su.host(case)
    assert su.same(states, wanted[name][0]) and su.same(closed, wanted[name][1])
    n = su.counted_times(case["windows"])
    assert n == 23
    for k in su.event_names(case):
        run, longest, spells, hits = (states[k][:, w].astype(np.int64) for w in range(4))
        # every spell is closed or open; the closed ones and the runs still open add up to the hits
        assert (longest <= hits).all() and (spells <= hits).all() and (run <= longest).all() and (hits <= n).all()
        assert (closed[k].sum(axis=(1, 2, 3)) + (run > 0).sum(axis=(1, 2, 3)) == spells.sum(axis=(1, 2, 3))).all()
        assert hits.sum() > 0


def test_fixture_covers_what_it_claims(cases):
    assert list(cases) == list(su.SMALL)
    base = cases["m5_b2_6x8"]
    assert [len(base["events"].get(k, ())) for k in base["names"]] == [3, 1, 0] and len(list(su._runs(base))) == 2
    assert [(s, t["a"].shape[1]) for s, t, _ in base["windows"]] == [(0, 6), (6, 6), (12, 6), (18, 6)]
    assert cases["m5_b2_6x10"]["W"] % 4 != 0 and cases["m25_b1_4x360"]["M"] == 25
    assert all(g.ndim == 4 for _, _, gen in cases["m1_b2_6x8"]["windows"] for g in gen.values())
    nan = cases["nan_m5_b2_6x8"]
    assert all(np.isnan(g["a"]).any() and np.isnan(t["a"]).any() for _, t, g in nan["windows"])
    assert np.isnan(nan["events"]["a"][0][2]).sum() == 2
    e8 = cases["e8_m5_b1_6x8"]["events"]["a"]
    assert len(e8) == 8 and {(d, isinstance(t, np.ndarray)) for _, d, t in e8} == {("above", False), ("above", True),
                                                                                    ("below", False), ("below", True)}


@pytest.mark.parametrize("name", ["m5_b2_6x8", "nan_m5_b2_6x8", "e8_m5_b1_6x8", "known_m5_b2_6x8"])
def test_window_cuts_give_the_same_bits(sdy, cases, wanted, name):
    """One window, the cuts of the case, and single-time windows: identical state and durations."""
    case = cases[name]
    for cuts in (((0, su.N_TIMES),), su.CUTS, tuple((t, t + 1) for t in range(su.N_TIMES)), ((0, 1), (1, 2), (2, 24))):
        states, closed = su.host(case, su.recut(case, cuts))
        assert su.same(states, wanted[name][0]) and su.same(closed, wanted[name][1]), cuts


def test_a_run_that_starts_later_counts_its_first_time(sdy, cases):
    """The first time of a window is dropped only at i_time_start == 0."""
    case = cases["m5_b2_6x8"]
    late = [(s + 7, t, g) for s, t, g in case["windows"]]
    states, _ = su.host(case, late)
    want, _ = su.restate(case, late)
    assert su.same(states, want) and su.counted_times(late) == 24


def test_duration_bins(sdy):
    """bin(d): the number of edges 1, 2, 4, .., 16384 below d.  Through the host twin: one trajectory that is in the event for d
    times and then leaves it."""
    ds = (1, 2, 3, 4, 5, 8, 9, 16, 17, 16384, 16385, 10 ** 6)
    want = (0, 1, 2, 2, 3, 3, 4, 4, 5, 14, 15, 15)
    assert tuple(int(b) for b in su.duration_bin(ds)) == want
    assert tuple(int(b) for b in sdy.spells.duration_bin(torch.tensor(ds))) == want
    assert sdy.spells.duration_edges().tolist() == su.EDGES.tolist()
    for d, b in zip(ds, want):
        x = np.ones((1, d + 1, 1, 1), np.float32)
        x[0, d] = 0.0
        case = dict(M=1, B=1, H=1, W=1, names=["a"], events={"a": [("on", "above", 0.5)]})
        states, closed = su.host(case, [(5, {"a": x}, {"a": x})])
        hist = np.zeros(16)
        hist[b] = 1
        assert np.array_equal(closed["a"][0, 0], hist[None]) and np.array_equal(closed["a"][0, 1], hist[None]), d
        assert states["a"][0, :, 0, 0, 0].tolist() == [0, d, 1, d]


def test_known_answer(sdy, cases):
    """The hand-made series: every generated trajectory has one spell of 20 times (bin 17..32) and one of 2 that is open at the
    end; every target spells of 1 and 3 times and one of 1 that is open."""
    case = cases["known_m5_b2_6x8"]
    states, closed = su.host(case)
    data = su.readout(case, states, closed)
    gen_rows, target_rows = 5 * 2, 2
    for k in ("a", "b"):
        st = states[k][0]
        assert (st[:, :gen_rows] == np.array([2, 20, 2, 22], np.uint32)[:, None, None, None]).all()
        assert (st[:, gen_rows:] == np.array([1, 3, 3, 5], np.uint32)[:, None, None, None]).all()
        want = np.zeros((2, 6, 16))
        want[0, :, 5] = gen_rows * 8                  # the 20 times: 17..32
        want[1, :, 0] = target_rows * 8               # 1 time
        want[1, :, 2] = target_rows * 8               # 3 times: 3..4
        assert np.array_equal(closed[k][0], want)
        want[0, :, 1] += gen_rows * 8                 # open at the end: 2 times
        want[1, :, 0] += target_rows * 8              # open at the end: 1 time
        assert np.array_equal(data[f"durations_gen/on/{k}"], want[0]) and np.array_equal(data[f"durations_target/on/{k}"], want[1])
        assert (data[f"gen_longest/on/{k}"] == 20).all() and (data[f"gen_spells/on/{k}"] == 2).all()
        assert (data[f"gen_hits/on/{k}"] == 22).all() and data[f"gen_hits/on/{k}"].shape == (5, 2, 6, 8)
        assert (data[f"target_longest/on/{k}"] == 3).all() and (data[f"target_spells/on/{k}"] == 3).all()
        assert (data[f"target_hits/on/{k}"] == 5).all() and data[f"target_hits/on/{k}"].shape == (2, 6, 8)
        assert np.array_equal(data[f"rows/on/{k}"][0], np.tile([22 * 80, 2 * 80, 20 * 80, 80], (6, 1)))
        assert np.array_equal(data[f"rows/on/{k}"][1], np.tile([5 * 16, 3 * 16, 3 * 16, 16], (6, 1)))
    logs, _ = su.restate_logs(case, data, 23)
    assert logs["mean_duration_gen/on/a"] == pytest.approx(11.0) and logs["mean_duration_target/on/a"] == pytest.approx(5 / 3)
    assert logs["longest_bias/on/a"] == pytest.approx(17.0) and logs["time_fraction_gen/on/b"] == pytest.approx(22 / 23)
    assert logs["onset_rate_target/on/b"] == pytest.approx(3 / 23)


def test_nan_rules(sdy, cases):
    """A NaN value is never in an event, so it ends a spell; a point whose threshold is NaN is in no event and its outputs are
    NaN."""
    x = np.ones((1, 6, 1, 4), np.float32)
    x[0, 2, 0, 1] = np.nan                                      # point 1: spells of 2 and 3 times
    thr = np.full((1, 4), 0.5, np.float32)
    thr[0, 3] = np.nan
    case = dict(M=1, B=1, H=1, W=4, names=["a"], events={"a": [("on", "above", thr)]})
    states, closed = su.host(case, [(3, {"a": x}, {"a": x})])
    assert states["a"][0, :, 0, 0].tolist() == [[6, 3, 6, 0], [6, 3, 6, 0], [1, 2, 1, 0], [6, 5, 6, 0]]   # run, longest, spells, hits
    assert closed["a"][0, 0, 0].tolist() == [0, 1] + [0] * 14
    data = su.readout(case, states, closed)
    assert np.isnan(data["gen_longest/on/a"][0, 0, 0, 3]) and np.isnan(data["target_hits/on/a"][0, 0, 3])
    assert data["rows/on/a"][0, 0].tolist() == [17, 4, 15, 3] and data["durations_gen/on/a"][0].tolist() == [0, 1, 1, 2] + [0] * 12
    nan = cases["nan_m5_b2_6x8"]
    states, _ = su.host(nan)
    for k in ("a", "b"):
        assert (states[k][0][:, :, 0, 2] == 0).all() and (states[k][0][:, :, 3, 5] == 0).all()
        assert (states[k][1][3, :, 0, 2] > 0).any()             # the other event of the same point counts


# ---- the entry points ------------------------------------------------------------------------------------------------------
def _small_call(M=3, with_map=True):
    rng = np.random.default_rng(3)
    target = {"a": rng.standard_normal((2, 3, 4, 6)).astype(np.float32)}
    gen = {"a": rng.standard_normal((M, 2, 3, 4, 6)).astype(np.float32)}
    events = {"a": [("hi", "above", 0.5), ("lo", "below", np.zeros((4, 6), np.float32) if with_map else -0.5)]}
    case = dict(M=M, B=2, H=4, W=6, names=["a"], events=events)
    state, durations = np.full((1, 2, 4, (M + 1) * 2, 4, 6), 7, np.uint32), np.full((1, 2, 2, 4, 16), 7.0)
    a, keep = su.args(case, target, gen, ["a"], 1, state, durations)
    return a, keep, state, durations


def _both(sdy, a):
    return [sdy.lib.sdy_event_spell_accumulate_host(C.byref(a)), sdy.lib.sdy_event_spell_accumulate(C.byref(a), None)]


@pytest.mark.parametrize("field,value,code", [
    ("struct_size", 0, SDY_ERR_ARG), ("struct_size", "+8", SDY_ERR_ARG), ("struct_size", "-8", SDY_ERR_ARG),
    ("n_events", 0, SDY_ERR_ARG), ("n_events", 9, SDY_ERR_ARG), ("n_events", -1, SDY_ERR_ARG),
    ("state", None, SDY_ERR_ARG), ("durations", None, SDY_ERR_ARG), ("scalars", None, SDY_ERR_ARG), ("maps", None, SDY_ERR_ARG),
    ("gen0", None, SDY_ERR_ARG), ("target0", None, SDY_ERR_ARG),
    ("state", "+4", SDY_ERR_ARG), ("durations", "+4", SDY_ERR_ARG),                             # off an 8-byte boundary
    ("n_maps", 0, SDY_ERR_ARG), ("map_first0", 1, SDY_ERR_ARG), ("map_first0", -1, SDY_ERR_ARG),  # map planes out of range
    ("t0", 4, SDY_ERR_ARG), ("t0", -1, SDY_ERR_ARG),
    ("gs0", -1, SDY_ERR_ARG), ("gs1", -4, SDY_ERR_ARG), ("ts1", -1, SDY_ERR_ARG),
    ("nvars", 0, SDY_ERR_ARG), ("nvars", 97, SDY_ERR_ARG),
    ("n0", 0, SDY_ERR_ARG), ("n1", -1, SDY_ERR_ARG), ("T", 0, SDY_ERR_ARG), ("H", 0, SDY_ERR_ARG), ("W", 0, SDY_ERR_ARG),
    ("n0", 65, SDY_ERR_UNSUPPORTED),                                                            # M over the maximum
    (("T", "H", "W"), (2, 1 << 15, (1 << 14) + 1), SDY_ERR_UNSUPPORTED),                        # T * H * W > 2^30
    (("n0", "n1"), (1 << 16, 1 << 15), SDY_ERR_UNSUPPORTED),                                    # n0 * n1 >= 2^31
    (("n0", "n1", "H", "W", "T"), (63, 1 << 20, 1, 1 << 6, 1), SDY_ERR_UNSUPPORTED),            # a row's LDS words: 2^32
    (("n0", "n1", "H", "W", "T"), (1, (1 << 30) - 1, 1, 2, 1), SDY_ERR_UNSUPPORTED),            # a row's items: 2^32 - 4
    (("n0", "n1", "H", "W", "T"), (15, 1 << 26, 1, 2, 2), SDY_ERR_UNSUPPORTED),                 # 2^31 items x 2 times
    (("n0", "n1", "H", "W", "T"), (1, 1 << 16, 1 << 30, 1, 1), SDY_ERR_UNSUPPORTED),            # state indices: 2^50
])
def test_entry_points_refuse(sdy, field, value, code):
    a, keep, state, durations = _small_call()
    if field == "gen0":
        a.gen[0] = None
    elif field == "target0":
        a.target[0] = None
    elif field == "map_first0":
        a.map_first[0] = value
    elif isinstance(field, tuple):
        for f, v in zip(field, value):
            setattr(a, f, v)
    elif isinstance(value, str):
        setattr(a, field, getattr(a, field) + int(value))
    else:
        setattr(a, field, value)
    # both entry points check before anything else: the device one is refused without a device
    assert _both(sdy, a) == [code] * 2
    assert (state == 7).all() and (durations == 7.0).all()
    assert [sdy.lib.sdy_event_spell_accumulate_host(None), sdy.lib.sdy_event_spell_accumulate(None, None)] == [SDY_ERR_ARG] * 2


def test_a_good_call_and_a_window_without_counted_times(sdy):
    a, keep, state, durations = _small_call()
    a.t0 = a.T                                                # SDY_OK from both: the device one launches nothing
    assert _both(sdy, a) == [SDY_OK] * 2 and (state == 7).all() and (durations == 7.0).all()
    a.t0 = 1
    assert sdy.lib.sdy_event_spell_accumulate_host(C.byref(a)) == SDY_OK and not (state == 7).all()


def test_struct_carries_its_size_and_is_not_in_the_handshake(sdy):
    from sdy_amd import _lib

    assert _lib.SdyEventSpellArgs not in _lib.ABI_STRUCTS and len(_lib.ABI_STRUCTS) == 25
    assert _lib.ABI_STRUCTS[-1] is _lib.SdyRankHistArgs
    assert _lib.SdyEventSpellArgs().struct_size == C.sizeof(_lib.SdyEventSpellArgs) and _lib.SDY_SPELL_BINS == 16
    assert _lib.SdyEventSpellArgs._fields_[0][0] == "struct_size" and _lib.SdyEventSpellArgs._fields_[1][0] == "win"
    for f in ("H", "W", "t0"):
        assert getattr(_lib.SdyEventSpellArgs, f).size == getattr(_lib.SdyEventArgs, f).size, f
    # the thresholds are the very type that SdyEventArgs embeds, not fields that share its names
    assert dict(_lib.SdyEventSpellArgs._fields_)["thr"] is dict(_lib.SdyEventArgs._fields_)["thr"] is _lib.SdyEventThresholds
    assert {"sdy_event_spell_accumulate", "sdy_event_spell_accumulate_host"} <= set(_lib.SIGNATURES)
    hdr = open(os.path.join(ROOT, "include", "sdy_amd.h")).read()
    assert "#define SDY_SPELL_BINS 16\n" in hdr and re.search(r"typedef struct sdy_event_spell_args sdy_event_spell_args;", hdr)
    assert int(re.search(r"SDY_ABI_STRUCTS (\d+)", hdr)[1]) == 25


# ---- the logs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", su.SMALL)
def test_logs_are_a_pure_function_of_rows(sdy, cases, wanted, name):
    case = cases[name]
    data = su.readout(case, *wanted[name])
    want, bounds = su.restate_logs(case, data, 23)
    got = {}
    w = torch.from_numpy(su.lat_weights(case))
    for k in su.event_names(case):
        for ev, _, _ in case["events"][k]:
            one = sdy.spells.logs_from_rows(data[f"rows/{ev}/{k}"], w, 23)
            assert list(one) == list(su.LOG_METRICS) == list(sdy.spells.LOG_METRICS)
            got.update({f"{m}/{ev}/{k}": v for m, v in one.items()})
    su.close_logs(got, want, bounds, name)
    assert all(np.isfinite(v) for v in want.values())


def test_logs_without_spells_are_nan(sdy):
    rows = np.zeros((2, 3, 4))
    rows[:, :, 3] = 8
    one = sdy.spells.logs_from_rows(rows, np.ones(3), 5)
    assert all(np.isnan(one[m]) for m in ("mean_duration_gen", "mean_duration_target", "mean_duration_ratio"))
    assert one["longest_gen"] == 0.0 and one["onset_rate_target"] == 0.0 and one["time_fraction_gen"] == 0.0
    one = sdy.spells.logs_from_rows(np.zeros((2, 3, 4)), np.ones(3), 5)              # nothing counted at all
    assert all(np.isnan(v) for v in one.values())


# ---- the Python classes, as far as they go without a device -----------------------------------------------------------------
def _window(M=3, B=2, T=3, H=4, W=6, names=("a", "b")):
    g = torch.Generator().manual_seed(0)
    target = {k: torch.randn(B, T, H, W, generator=g) for k in names}
    gen = {k: torch.randn(M, B, T, H, W, generator=g) for k in names}
    return target, gen


def _record(agg, target, gen, **kw):
    agg.record_batch(loss=0.0, target_data=target, gen_data=gen, target_data_norm=target, gen_data_norm=gen, **kw)


def _events(sdy, names=("a",), shape=None):
    ev = sdy.Events()
    for k in names:
        ev.add(k, "hi", above=0.5)
        if shape is not None:
            ev.add(k, "map", below=torch.zeros(shape))
    return ev


def test_class_refuses_before_the_device(sdy):
    assert issubclass(sdy.EventSpellAggregator, sdy.events.EventAccumulator) and sdy.spells.EventSpellAggregator is sdy.EventSpellAggregator
    with pytest.raises(ValueError, match="EventSpellAggregator: the area weights vary along a latitude row"):
        sdy.EventSpellAggregator(_events(sdy), torch.arange(24.0).view(4, 6), n_timesteps=3)
    with pytest.raises(ValueError, match="at least one event"):
        sdy.EventSpellAggregator(sdy.Events(), torch.ones(4, 6), n_timesteps=3)
    agg = sdy.EventSpellAggregator(_events(sdy, shape=(4, 6)), torch.ones(4, 6), n_timesteps=3)
    before = dict(vars(agg))
    with pytest.raises(RuntimeError, match="GPU only"):
        _record(agg, *_window())
    assert vars(agg) == before and agg._names is None and agg.n_times == 0          # a refused window changes nothing
    for read in (agg.get_data, lambda: agg.get_logs("x")):
        with pytest.raises(ValueError, match="No data recorded."):
            read()
    target, gen = _window()
    flat = {k: v.reshape(-1, *v.shape[2:])[:5] for k, v in gen.items()}
    with pytest.raises(ValueError, match="EventSpellAggregator needs member-stacked"):
        _record(agg, target, flat)
    with pytest.raises(ValueError, match="member-stacked"):
        _record(agg, {k: v[:1] for k, v in target.items()}, {k: v[:1] for k, v in flat.items()}, sample_weights=[1 / 3])
    with pytest.raises(ValueError, match="times 2..4 outside the aggregator's 3"):
        _record(agg, *_window(), i_time_start=2)
    with pytest.raises(ValueError, match="at most 64 members, got 65"):
        _record(agg, *_window(M=65, B=1, T=1))
    assert vars(agg) == before


def test_class_sizes_its_state(sdy):
    need = 8 * (2 * 2 * (3 + 1) * 2 * 4 * 6 + 2 * 2 * 4 * 16)          # 16 bytes per (event, trajectory, point) and the histograms
    agg = sdy.EventSpellAggregator(_events(sdy, shape=(4, 6)), torch.ones(4, 6), n_timesteps=3, max_bytes=need - 1)
    with pytest.raises(ValueError, match=f"the spell state .16 bytes per event, trajectory and grid point. of 2 events of 1 "
                                         f"variables, 3 members x 2 samples need {need} bytes"):
        _record(agg, *_window())
    agg = sdy.EventSpellAggregator(_events(sdy, shape=(4, 6)), torch.ones(4, 6), n_timesteps=3, max_bytes=need)
    with pytest.raises(RuntimeError, match="GPU only"):
        _record(agg, *_window())


def test_inference_aggregator_option(sdy):
    w = torch.ones(4, 6)
    with pytest.raises(ValueError, match="event_spells needs events"):
        sdy.metrics.InferenceAggregator(w, n_timesteps=3, n_ensemble_members=2, event_spells=True)
    plain = sdy.metrics.InferenceAggregator(w, n_timesteps=3, n_ensemble_members=2)
    assert list(plain._aggregators) == ["mean", "mean_norm", "time_mean"]               # the default set is unchanged
    with_events = sdy.metrics.InferenceAggregator(w, n_timesteps=3, n_ensemble_members=2, events=_events(sdy))
    assert list(with_events._aggregators) == ["mean", "mean_norm", "time_mean", "events"]
    agg = sdy.metrics.InferenceAggregator(w, n_timesteps=3, n_ensemble_members=2, events=_events(sdy), event_spells=True)
    assert list(agg._aggregators) == ["mean", "mean_norm", "time_mean", "events", "spells"]
    assert isinstance(agg._aggregators["spells"], sdy.EventSpellAggregator) and hasattr(agg, "get_spell_data")


def test_one_field_function_refuses_before_the_device(sdy):
    with pytest.raises(ValueError, match="expected .time, lat, lon."):
        sdy.spells.spell_statistics(torch.zeros(4, 6), 0.5)
    with pytest.raises(RuntimeError, match="GPU only"):
        sdy.spells.spell_statistics(torch.zeros(5, 4, 6), 0.5)
