"""Host side of the threshold-event verification (no GPU): sdy_event_table_accumulate_host and
sdy_event_frequency_accumulate_host -- the header the kernels compile (csrc/events.h) -- against the numpy restatement on
every case, `sdy_amd.events.scores` on CPU tensors against its float64 restatement, what `Events.add` and the entry points
refuse, and what `EventVerificationAggregator` refuses before it touches a device.  Cases and comparisons:
tests/event_verif_utils.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import event_verif_utils as eu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SDY_OK, SDY_ERR_ARG, SDY_ERR_UNSUPPORTED = 0, -1, -2


@pytest.fixture(scope="module")
def sdy():
    import sdy_amd

    return sdy_amd


@pytest.fixture(scope="module")
def cases():
    return eu.cases()


@pytest.mark.parametrize("name", eu.SMALL)
@pytest.mark.parametrize("pool", [False, True], ids=["slots", "pooled"])
def test_host_twins_against_restatement(sdy, cases, name, pool):
    case = cases[name]
    tables, maps = eu.host(case, pool)
    want_tables, want_maps = eu.restate(case, pool)
    assert eu.same(tables, want_tables) and eu.same(maps, want_maps)
    for k in eu.event_names(case):
        # every counted point is in exactly one bin of each of its events; the maps pool the slots
        assert np.array_equal(tables[k].sum(axis=(0, 3, 4)), maps[k][:, 2].sum(axis=2))
        assert np.array_equal((tables[k] * np.arange(case["M"] + 1)).sum(axis=(0, 3, 4)), maps[k][:, 0].sum(axis=2))
        assert np.array_equal(tables[k][:, :, :, 1].sum(axis=(0, 3)), maps[k][:, 1].sum(axis=2))
        if not pool:
            assert (tables[k][0] == 0).all() and (tables[k][1:].sum(axis=(2, 3, 4)) > 0).all()


def test_fixture_covers_what_it_claims(cases):
    assert list(cases) == list(eu.SMALL)
    base = cases["m5_b2_6x8"]
    assert [len(base["events"].get(k, ())) for k in base["names"]] == [3, 1, 0] and len(list(eu._runs(base))) == 2
    kinds = [(d, isinstance(t, np.ndarray)) for _, d, t in base["events"]["a"]]
    assert kinds == [("above", False), ("below", False), ("above", True)]
    assert cases["m2_b3_7x10"]["W"] % 4 != 0 and cases["m2_b3_7x10"]["H"] % 2 == 1
    assert cases["m9_b1_4x36"]["M"] == 8 + 1 and cases["m9_b1_4x36"]["W"] // 4 == 9
    assert cases["m25_b1_4x360"]["M"] == 25 and all(len(v) == 4 for v in cases["m25_b1_4x360"]["events"].values())
    big = cases["m64_b1_4x8_e8"]
    assert big["M"] == 64 and all(len(v) == 8 for v in big["events"].values())
    assert 8 * 2 * 65 * 4 == 4160 and (256 // 4) * 4160 > 64 * 1024        # the narrowest group's 64 rows do not fit: capped
    assert all(g.ndim == 4 for _, _, gen in cases["m1_b2_6x8"]["windows"] for g in gen.values())
    for case in cases.values():
        assert [(s, t["a"].shape[1]) for s, t, _ in case["windows"]] == [(0, 3), (3, 2)] and case["n_timesteps"] == 5


def test_known_answer(sdy, cases):
    """Member m is the constant field m, the target k - 0.5 on latitude k, the event above 1.5: every counted point has k = M -
    2 members in the event and o = 1 exactly on latitudes >= 3."""
    case = cases["known_m5_b2_6x8"]
    tables, maps = eu.host(case)
    per_row = case["B"] * case["W"]
    want = np.zeros((6, 2, 6))
    want[:3, 0, 3] = per_row
    want[3:, 1, 3] = per_row
    for k in ("a", "b"):
        for slot in range(1, 5):
            assert np.array_equal(tables[k][slot, 0], want)
        assert (tables[k][0] == 0).all()
        assert np.array_equal(maps[k][0, 0], np.full((6, 8), 3.0 * 2 * 4)) and (maps[k][0, 2] == 2 * 4).all()
        assert np.array_equal(maps[k][0, 1], np.repeat(np.array([0, 0, 0, 8, 8, 8.0])[:, None], 8, axis=1))


def test_clipped_fields_compare_strictly(sdy, cases):
    """max(x, 0) on both sides: `above 0.0` is false at the zeros that really occur, `below 0.0` is never true."""
    case = cases["clipped_m5_b2_6x8"]
    tables, maps = eu.host(case)
    for k in ("a", "b"):
        wet, negative = tables[k][:, 0], tables[k][:, 1]
        total = negative.sum()
        assert total == 2 * 4 * 6 * 8 and negative[:, :, 0, 0].sum() == total          # o = 0, k = 0 for every point
        y = np.concatenate([t[k] for _, t, _ in case["windows"]], axis=1)[:, 1:]
        assert wet[:, :, 1].sum() == (y > 0).sum() and 0.3 * total < (y == 0).sum() < 0.7 * total
        assert (maps[k][1, :2] == 0).all() and (maps[k][1, 2] == 2 * 4).all()


def test_nan_rules(sdy, cases):
    """A NaN target or a NaN threshold masks the point (for that event only), a NaN member is simply not in the event."""
    case = cases["nan_m5_b2_6x8"]
    tables, maps = eu.host(case)
    for k in ("a", "b"):
        y = np.concatenate([t[k] for _, t, _ in case["windows"]], axis=1)[:, 1:]
        seen = (~np.isnan(y)).sum(axis=(0, 1))
        thr = case["events"][k][0][2]
        assert np.isnan(thr[0, 2]) and np.isnan(thr[3, 5]) and np.isnan(thr).sum() == 2
        assert np.array_equal(maps[k][0, 2], np.where(np.isnan(thr), 0, seen)) and np.array_equal(maps[k][1, 2], seen)
        assert seen.sum() < y[0, 0].size * 2 * 4
    y = {"a": np.full((1, 1, 1, 4), 10.0, np.float32)}
    g = {"a": np.full((3, 1, 1, 1, 4), 20.0, np.float32)}
    g["a"][1, 0, 0, 0, 2] = np.nan
    y["a"][0, 0, 0, 3] = np.nan
    one = dict(M=3, B=1, H=1, W=4, names=["a"], n_timesteps=6, windows=[(5, y, g)], events={"a": [("big", "above", 15.0)]})
    tables, maps = eu.host(one)
    assert np.array_equal(tables["a"][5, 0, 0], [[0, 0, 1, 2], [0, 0, 0, 0]])
    assert np.array_equal(maps["a"][0, :, 0], [[3, 3, 2, 0], [0, 0, 0, 0], [1, 1, 1, 0]])


def test_pooled_equals_the_slots_summed(sdy, cases):
    for name in ("m5_b2_6x8", "nan_m5_b2_6x8", "m64_b1_4x8_e8"):
        tables, maps = eu.host(cases[name])
        pooled, pooled_maps = eu.host(cases[name], pool=True)
        assert eu.same(pooled, {k: v.sum(axis=0, keepdims=True) for k, v in tables.items()}) and eu.same(pooled_maps, maps)


# ---- the scores ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", eu.SMALL)
def test_scores_against_restatement(sdy, cases, name):
    case = cases[name]
    tables, _ = eu.restate(case)
    w = eu.lat_weights(case)
    for k in eu.event_names(case):
        got = sdy.events.scores(torch.from_numpy(tables[k]).transpose(0, 1), torch.from_numpy(w))        # (E, slots, ...)
        assert all(v.dtype == torch.float64 and not v.is_cuda for v in got.values())
        for e in range(tables[k].shape[1]):
            for slot in range(tables[k].shape[0]):
                want = eu.restate_scores(tables[k][slot, e], w)
                eu.close_scores({m: v[e, slot].numpy() for m, v in got.items()}, want, f"{name} {k} {e} {slot}")
                if slot == 0:
                    assert all(bool(torch.isnan(v[e, slot]).all()) for v in got.values())          # a slot without counts
                else:
                    s = {m: float(v[e, slot]) for m, v in got.items() if m != "reliability_curve"}
                    assert abs(s["brier_score"] - (s["brier_reliability"] - s["brier_resolution"] + s["uncertainty"])) <= eu.TOL


def test_scores_known_values(sdy):
    """A perfect forecast and a constant one, by hand."""
    t = torch.zeros(2, 1, 2, 5, dtype=torch.float64)
    t[0, 0, 0, 0], t[0, 0, 1, 4] = 30, 10                    # all members say no / yes, and they are right
    t[1, 0, 0, 2], t[1, 0, 1, 2] = 30, 10                    # always 50 %: no resolution
    s = sdy.events.scores(t, torch.ones(1))
    assert s["brier_score"].tolist() == [0.0, 0.25] and s["base_rate"].tolist() == [0.25, 0.25]
    assert s["brier_reliability"].tolist() == [0.0, 0.0625] and s["brier_resolution"].tolist() == [0.1875, 0.0]
    assert s["roc_area"].tolist() == [1.0, 0.5] and s["forecast_rate"].tolist() == [0.25, 0.5]
    assert s["brier_skill_score"].tolist() == [1.0, 1.0 - 0.25 / 0.1875]
    with pytest.raises(ValueError, match="a table is"):
        sdy.events.scores(torch.zeros(3, 3, 4), torch.ones(3))


def test_logs_restatement_is_the_pooled_table(sdy, cases):
    case = cases["m5_b2_6x8"]
    tables, _ = eu.restate(case)
    logs = eu.restate_logs(case, tables, "x")
    assert list(logs) == [f"x/{m}/{n}/{k}" for k in ("a", "b") for n, _, _ in case["events"][k] for m in eu.LOG_METRICS]
    assert eu.LOG_METRICS == sdy.events.LOG_METRICS and eu.SLOT_METRICS == sdy.events.SLOT_METRICS


# ---- Events ----------------------------------------------------------------------------------------------------------------
def test_events_add_refusals(sdy):
    ev = sdy.Events()
    ev.add("a", "wet", above=1.0).add("a", "dry", below=0.1).add("b", "wet", above=np.zeros((4, 6)))
    assert ev.variables == ["a", "b"] and [e.name for e in ev.of("a")] == ["wet", "dry"] and len(ev) == 3
    assert [e.below for e in ev.of("a")] == [False, True] and ev.of("b")[0].map.dtype == torch.float32 and ev.of("c") == []
    assert ev.of("a")[1].scalar == float(np.float32(0.1))                   # rounded once to fp32
    for kw in ({}, dict(above=1.0, below=2.0)):
        with pytest.raises(ValueError, match="exactly one of above= and below="):
            ev.add("a", "x", **kw)
    for bad in (float("nan"), float("inf"), -float("inf"), 1e39):
        with pytest.raises(ValueError, match="not a finite fp32 number"):
            ev.add("a", "x", above=bad)
    for bad in ("", "a/b"):
        with pytest.raises(ValueError, match="non-empty string without '/'"):
            ev.add("a", bad, above=1.0)
    with pytest.raises(ValueError, match="already has an event 'wet'"):
        ev.add("a", "wet", below=3.0)
    ev.add("c", "wet", above=1.0)                                               # the same name on another variable is fine
    with pytest.raises(ValueError, match="a number or a .lat, lon. map"):
        ev.add("a", "x", above=np.zeros(5))
    for i in range(6):
        ev.add("a", f"e{i}", above=float(i))
    with pytest.raises(ValueError, match="at most 8 events per variable"):
        ev.add("a", "ninth", above=1.0)
    assert len(ev.of("a")) == 8 and len(ev) == 10                               # a refused add changes nothing


# ---- the entry points ------------------------------------------------------------------------------------------------------
def _small_call(M=3, pool=False, with_map=True):
    rng = np.random.default_rng(3)
    target = {"a": rng.standard_normal((2, 3, 4, 6)).astype(np.float32)}
    gen = {"a": rng.standard_normal((M, 2, 3, 4, 6)).astype(np.float32)}
    events = {"a": [("hi", "above", 0.5), ("lo", "below", np.zeros((4, 6), np.float32) if with_map else -0.5)]}
    case = dict(M=M, B=2, H=4, W=6, names=["a"], events=events)
    n_slots = 1 if pool else 5
    table, freq = np.full((1, n_slots, 2, 4, 2, M + 1), 7.0), np.full((1, 2, 3, 4, 6), 7.0)
    a, keep = eu.args(case, target, gen, ["a"], 1, 0, n_slots, pool, table)
    return a, keep, table, freq


def _both(sdy, a, table, freq):
    """-> the codes of the four entry points (table host, table device, frequency host, frequency device); the frequency pair
    gets the maps in the place of the table, at the same offset."""
    from window_utils import vp

    lib = sdy.lib
    codes = [lib.sdy_event_table_accumulate_host(C.byref(a)), lib.sdy_event_table_accumulate(C.byref(a), None)]
    if a.acc:
        a.acc = vp(freq) + (a.acc - vp(table))
    codes += [lib.sdy_event_frequency_accumulate_host(C.byref(a)), lib.sdy_event_frequency_accumulate(C.byref(a), None)]
    return codes


@pytest.mark.parametrize("field,value,code", [
    ("acc", None, SDY_ERR_ARG), ("scalars", None, SDY_ERR_ARG), ("maps", None, SDY_ERR_ARG),    # NULL pointers
    ("acc", "+4", SDY_ERR_ARG),                                                                 # off an 8-byte boundary
    ("n_events", 0, SDY_ERR_ARG), ("n_events", 9, SDY_ERR_ARG), ("n_events", -1, SDY_ERR_ARG),
    ("t0", 4, SDY_ERR_ARG), ("t0", -1, SDY_ERR_ARG),                                            # t0 outside 0..T
    ("t_start", 3, SDY_ERR_ARG), ("t_start", -1, SDY_ERR_ARG), ("n_slots", 2, SDY_ERR_ARG),     # slot overflow
    ("n_slots", 0, SDY_ERR_ARG),
    ("n_maps", 0, SDY_ERR_ARG), ("map_first0", 1, SDY_ERR_ARG), ("map_first0", -1, SDY_ERR_ARG),  # map planes past the buffer
    ("gs0", -1, SDY_ERR_ARG), ("gs1", -4, SDY_ERR_ARG), ("ts1", -1, SDY_ERR_ARG),               # negative strides
    ("nvars", 0, SDY_ERR_ARG), ("nvars", 97, SDY_ERR_ARG),
    ("n0", 0, SDY_ERR_ARG), ("n1", -1, SDY_ERR_ARG), ("T", 0, SDY_ERR_ARG), ("H", 0, SDY_ERR_ARG), ("W", 0, SDY_ERR_ARG),
    ("gen0", None, SDY_ERR_ARG), ("target0", None, SDY_ERR_ARG),
    ("n0", 65, SDY_ERR_UNSUPPORTED),                                                            # M over the maximum
    (("T", "H", "W", "n_slots"), (2, 1 << 15, (1 << 14) + 1, 2), SDY_ERR_UNSUPPORTED),          # T * H * W > 2^30
    (("n0", "n1"), (1 << 16, 1 << 15), SDY_ERR_UNSUPPORTED),                                    # n0 * n1 >= 2^31
])
def test_entry_points_refuse(sdy, field, value, code):
    a, keep, table, freq = _small_call()
    if field == "gen0":
        a.gen[0] = None
    elif field == "target0":
        a.target[0] = None
    elif field == "map_first0":
        a.map_first[0] = value
    elif isinstance(field, tuple):
        for f, v in zip(field, value):
            setattr(a, f, v)
    elif value == "+4":
        setattr(a, field, getattr(a, field) + 4)
    else:
        setattr(a, field, value)
    # all four entry points check before anything else: the device ones are refused without a device
    assert _both(sdy, a, table, freq) == [code] * 4
    assert (table == 7.0).all() and (freq == 7.0).all()
    lib = sdy.lib
    assert [lib.sdy_event_table_accumulate_host(None), lib.sdy_event_table_accumulate(None, None),
            lib.sdy_event_frequency_accumulate_host(None), lib.sdy_event_frequency_accumulate(None, None)] == [SDY_ERR_ARG] * 4


def test_counter_bounds_of_each_entry_point(sdy):
    """What only one of the two kernels cannot take, asked of that one only: a table row's points reach 2^32, n_slots * H
    reaches 2^40; a point's member hits reach 2^31."""
    lib = sdy.lib
    for fields, values in ((("n1", "H", "W", "T", "n_slots"), (1 << 20, 1, 1 << 12, 1, 1)),
                           (("t_start", "n_slots", "H", "W"), (0, 1 << 30, 1 << 10, 4))):
        a, keep, table, freq = _small_call(with_map=False)
        for f, v in zip(fields, values):
            setattr(a, f, v)
        assert lib.sdy_event_table_accumulate_host(C.byref(a)) == SDY_ERR_UNSUPPORTED
        assert lib.sdy_event_table_accumulate(C.byref(a), None) == SDY_ERR_UNSUPPORTED
        assert (table == 7.0).all()
    from window_utils import vp

    a, keep, table, freq = _small_call(with_map=False)
    a.acc = vp(freq)
    for f, v in zip(("n0", "n1", "T", "H", "W", "n_slots"), (64, 1 << 20, 1 << 5, 1, 1, 1 << 5)):
        setattr(a, f, v)
    assert lib.sdy_event_frequency_accumulate_host(C.byref(a)) == SDY_ERR_UNSUPPORTED
    assert lib.sdy_event_frequency_accumulate(C.byref(a), None) == SDY_ERR_UNSUPPORTED
    assert (freq == 7.0).all()


def test_pooled_entry_points_take_one_slot_only(sdy):
    a, keep, table, freq = _small_call(pool=True)
    a.t_start = 1000                                      # not looked at when the times are pooled
    assert sdy.lib.sdy_event_table_accumulate_host(C.byref(a)) == SDY_OK
    assert table.sum() == 7.0 * table.size + 2 * (2 * 2 * 4 * 6)            # two events x the counted points
    a.n_slots = 2
    assert _both(sdy, a, table, freq) == [SDY_ERR_ARG] * 4


def test_a_window_without_counted_times_is_ok_and_changes_nothing(sdy):
    """T - t0 == 0: SDY_OK from all four entry points -- the device ones launch nothing, so they need no device."""
    a, keep, table, freq = _small_call()
    a.t0 = a.T
    assert _both(sdy, a, table, freq) == [SDY_OK] * 4
    assert (table == 7.0).all() and (freq == 7.0).all()


def test_struct_is_in_the_handshake(sdy):
    from sdy_amd import _lib

    assert _lib.SdyEventArgs in _lib.ABI_STRUCTS and (_lib.SDY_EVENT_MAX, _lib.SDY_EVENT_MAX_MEMBERS) == (8, 64)
    hdr = open(os.path.join(ROOT, "include", "sdy_amd.h")).read()
    assert "#define SDY_EVENT_MAX 8\n" in hdr and "#define SDY_EVENT_MAX_MEMBERS 64\n" in hdr


# ---- the Python class, as far as it goes without a device -----------------------------------------------------------------
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


def test_class_refusals_at_construction(sdy):
    w = torch.ones(4, 6)
    sdy.EventVerificationAggregator(_events(sdy), w * torch.arange(1.0, 5.0)[:, None], n_timesteps=3)
    w[2, 3] = 1.5
    with pytest.raises(ValueError, match="EventVerificationAggregator: the area weights vary along a latitude row"):
        sdy.EventVerificationAggregator(_events(sdy), w, n_timesteps=3)
    with pytest.raises(ValueError, match="n_timesteps must be positive"):
        sdy.EventVerificationAggregator(_events(sdy), torch.ones(4, 6), n_timesteps=0)
    with pytest.raises(ValueError, match="at least one event"):
        sdy.EventVerificationAggregator(sdy.Events(), torch.ones(4, 6), n_timesteps=3)


def test_class_refuses_before_the_device(sdy):
    agg = sdy.EventVerificationAggregator(_events(sdy, ("a", "z")), torch.ones(4, 6), n_timesteps=3)
    before = dict(vars(agg))
    with pytest.raises(ValueError, match="no generated variable 'z' in the window"):
        _record(agg, *_window())
    agg = sdy.EventVerificationAggregator(_events(sdy, shape=(4, 5)), torch.ones(4, 6), n_timesteps=3)
    with pytest.raises(ValueError, match=r"a \(4, 5\) threshold map against a \(4, 6\) grid"):
        _record(agg, *_window())
    agg = sdy.EventVerificationAggregator(_events(sdy, shape=(4, 6)), torch.ones(4, 6), n_timesteps=3)
    before = dict(vars(agg))
    with pytest.raises(RuntimeError, match="GPU only"):
        _record(agg, *_window())
    assert vars(agg) == before and agg._names is None and agg._scalars is None      # a refused window changes nothing
    with pytest.raises(ValueError, match="No data recorded"):
        agg.get_logs("x")
    with pytest.raises(ValueError, match="No data recorded"):
        agg.get_data()
    target, gen = _window()
    flat = {k: v.reshape(-1, *v.shape[2:])[:5] for k, v in gen.items()}
    with pytest.raises(ValueError, match="EventVerificationAggregator needs member-stacked"):
        _record(agg, target, flat)
    with pytest.raises(ValueError, match="member-stacked"):
        _record(agg, {k: v[:1] for k, v in target.items()}, {k: v[:1] for k, v in flat.items()}, sample_weights=[1 / 3])
    with pytest.raises(ValueError, match="times 2..4 outside the aggregator's 3"):
        _record(agg, *_window(), i_time_start=2)
    with pytest.raises(ValueError, match="at most 64 members, got 65"):
        _record(agg, *_window(M=65, B=1, T=1))
    assert agg._names is None


def test_class_sizes_its_accumulators(sdy):
    need = 8 * (3 * 2 * 4 * 2 * (3 + 1) + 2 * 3 * 4 * 6)        # table (slots, E, lat, 2, M + 1) and maps (E, 3, lat x lon)
    agg = sdy.EventVerificationAggregator(_events(sdy, shape=(4, 6)), torch.ones(4, 6), n_timesteps=3, frequency_maps=True,
                                          max_bytes=need - 1)
    with pytest.raises(ValueError, match=f"need {need} bytes"):
        _record(agg, *_window())
    agg = sdy.EventVerificationAggregator(_events(sdy, shape=(4, 6)), torch.ones(4, 6), n_timesteps=3, max_bytes=need - 8 * 144)
    with pytest.raises(RuntimeError, match="GPU only"):            # without the maps the table alone fits
        _record(agg, *_window())


def test_inference_aggregator_option_is_off_by_default(sdy):
    w = torch.ones(4, 6)
    assert "events" not in sdy.metrics.InferenceAggregator(w, n_timesteps=3, n_ensemble_members=2)._aggregators
    agg = sdy.metrics.InferenceAggregator(w, n_timesteps=3, n_ensemble_members=2, events=_events(sdy))
    ev = agg._aggregators["events"]
    assert isinstance(ev, sdy.EventVerificationAggregator) and ev._n_slots == 3 and not ev._frequency_maps
    assert list(agg._aggregators)[-1] == "events"
    agg = sdy.metrics.InferenceAggregator(w, n_timesteps=3, n_ensemble_members=2, events=_events(sdy), event_pool_times=True,
                                          event_frequency_maps=True)
    assert agg._aggregators["events"]._n_slots == 1 and agg._aggregators["events"]._frequency_maps
