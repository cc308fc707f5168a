"""Host side of the time bins (no GPU): the calendars of `sdy_amd.TimeBins` against restatements with Python's datetime and
with month-length lists, and sdy_binned_time_accumulate_host -- the chain order, the extremes, the NaN and empty-bin rules, the
independence of the cut into windows and of the order of the groups, and every refusal of the contract."""
import ctypes as C
import datetime
from fractions import Fraction

import numpy as np
import pytest

import time_bins_utils as tu
from time_bins_utils import SDY_ERR_ARG, SDY_ERR_UNSUPPORTED, SDY_OK

SEASONS = ("DJF", "MAM", "JJA", "SON")
MONTHS = ("Jan", "Feb", "Mar", "Apr", "May", "Jun", "Jul", "Aug", "Sep", "Oct", "Nov", "Dec")


@pytest.fixture(scope="module")
def sdy():
    import sdy_amd

    return sdy_amd


def _names_of(kind, dates):
    """Per time the name of its bin, restated; dates: (year, month, hour)."""
    out = []
    for y, m, h in dates:
        s = (m % 12) // 3
        out.append({"month": MONTHS[m - 1], "season": SEASONS[s], "year": f"{y:04d}", "year_month": f"{y:04d}-{m:02d}",
                    "year_season": f"{y + (m == 12):04d}-{SEASONS[s]}", "hour_of_day": f"{h:02d}h"}[kind])
    return out


def _check_labels(bins, kind, dates):
    want = _names_of(kind, dates)
    assert bins.labels.dtype == np.int32 and len(bins.labels) == len(dates) and bins.n_bins == len(bins.names)
    assert [bins.names[b] for b in bins.labels] == want
    # bins in calendar order, none missing between the first and the last
    if kind in ("year", "year_month", "year_season"):
        first_seen = list(dict.fromkeys(want))
        assert bins.names == first_seen
    elif kind == "month":
        assert bins.names == list(MONTHS)
    elif kind == "season":
        assert bins.names == list(SEASONS)


@pytest.mark.parametrize("first_year", [1896, 1996])
@pytest.mark.parametrize("kind", ["month", "season", "year", "year_month", "year_season", "hour_of_day"])
def test_gregorian_labels_equal_datetime(sdy, kind, first_year):
    """Ten years at 6-hour steps: 1896-1905 holds 1900 (no leap day), 1996-2005 holds 2000 (a leap day)."""
    t0 = datetime.datetime(first_year, 1, 1)
    n = (datetime.datetime(first_year + 10, 1, 1) - t0).days * 4
    assert n == (3652 if first_year == 1896 else 3653) * 4
    dates = [(d.year, d.month, d.hour) for d in (t0 + datetime.timedelta(hours=6 * i) for i in range(n))]
    bins = sdy.TimeBins.calendar(kind, (first_year, 1, 1), n, step_hours=6, calendar="proleptic_gregorian")
    _check_labels(bins, kind, dates)
    # whole years: every bin but those of a season-year cut by the run's ends is complete
    counts = bins.label_counts()
    partial = {0, bins.n_bins - 1} if kind == "year_season" else set()
    for b in range(bins.n_bins):
        assert (counts[b] < bins.expected_counts[b]) == (b in partial), (bins.names[b], counts[b], bins.expected_counts[b])


@pytest.mark.parametrize("calendar,lengths", [("noleap", [31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31]), ("360_day", [30] * 12)])
@pytest.mark.parametrize("kind", ["month", "season", "year", "year_month", "year_season", "hour_of_day"])
def test_model_calendars_equal_a_month_length_list(sdy, kind, calendar, lengths):
    """From 11 February 2099, 09:00, at 5-hour steps over more than three years: walked day by day."""
    y, m, d, h = 2099, 2, 11, 9
    n, step = 5400, 5
    dates = []
    for _ in range(n):
        dates.append((y, m, h))
        h += step
        while h >= 24:
            h -= 24
            d += 1
            if d > lengths[m - 1]:
                d, m = 1, m + 1
                if m > 12:
                    m, y = 1, y + 1
    assert y >= 2102
    _check_labels(sdy.TimeBins.calendar(kind, (2099, 2, 11, 9), n, step_hours=step, calendar=calendar), kind, dates)


def test_december_counts_with_the_next_season_year_and_expected_counts(sdy):
    """noleap, daily from 1 November 2001 for 500 days: SON of 2001 from its last third on, all of DJF 2002 (December 2001
    with it) .. SON 2002, DJF 2003 and 15 days of MAM 2003."""
    bins = sdy.TimeBins.calendar("year_season", (2001, 11, 1), 500, step_hours=24)
    assert bins.names == ["2001-SON", "2002-DJF", "2002-MAM", "2002-JJA", "2002-SON", "2003-DJF", "2003-MAM"]
    assert bins.names[bins.labels[30]] == "2002-DJF" and bins.names[bins.labels[29]] == "2001-SON"      # 1 December 2001
    assert list(bins.label_counts()) == [30, 90, 92, 92, 91, 90, 15]
    assert list(bins.expected_counts) == [91, 90, 92, 92, 91, 90, 92]
    # a Gregorian leap February
    leap = sdy.TimeBins.calendar("year_month", (2000, 2, 10), 30, step_hours=24, calendar="proleptic_gregorian")
    assert leap.names == ["2000-02", "2000-03"] and list(leap.label_counts()) == [20, 10] and list(leap.expected_counts) == [29, 31]
    hours = sdy.TimeBins.calendar("hour_of_day", (2000, 1, 1, 6), 7)
    assert hours.names == ["00h", "06h", "12h", "18h"] and list(hours.labels) == [1, 2, 3, 0, 1, 2, 3]
    assert list(hours.expected_counts) == [2, 2, 2, 2]


def test_calendar_refusals(sdy):
    ok = dict(kind="month", start=(2000, 1, 1), n_timesteps=8)
    for wrong in (dict(kind="week"), dict(calendar="julian"), dict(start=(2000, 1)), dict(start=(2000, 13, 1)),
                  dict(start=(2001, 2, 29), calendar="proleptic_gregorian"), dict(start=(2000, 2, 29)),
                  dict(start=(2000, 1, 31), calendar="360_day"), dict(start=(2000, 1, 1, 24)), dict(start=(2000.5, 1, 1)),
                  dict(n_timesteps=0), dict(step_hours=0)):
        with pytest.raises(ValueError):
            sdy.TimeBins.calendar(**{**ok, **wrong})
    assert sdy.TimeBins.calendar("month", (2000, 2, 29), 1, calendar="proleptic_gregorian").labels[0] == 1


def test_from_labels_and_restrict(sdy):
    bins = sdy.TimeBins.from_labels([0, 2, -1, 1, 2])
    assert bins.n_bins == 3 and bins.names == ["0", "1", "2"] and bins.labels.dtype == np.int32 and bins.expected_counts is None
    named = sdy.TimeBins.from_labels(np.array([0, 1, 1, -1]), names=["wet", "dry", "never"])
    assert named.n_bins == 3 and list(named.label_counts()) == [1, 2, 0]
    for wrong, names in (([[0, 1]], None), ([], None), ([0.0, 1.0], None), ([0, -2], None), ([-1, -1], None), ([0, 3], ["a", "b", "c"]),
                         ([0, 1], ["a", "a"]), ([0, 1], ["a", "b/c"]), ([0], [])):
        with pytest.raises(ValueError):
            sdy.TimeBins.from_labels(wrong, names)
    months = sdy.TimeBins.calendar("month", (2000, 1, 1), 4 * 365)
    summer = months.restrict(["Jun", "Jul", 7])
    assert summer.n_bins == 12 and summer.names == months.names
    assert set(summer.labels.tolist()) == {-1, 5, 6, 7} and np.array_equal(summer.labels >= 0, np.isin(months.labels, [5, 6, 7]))
    assert np.array_equal(months.labels, sdy.TimeBins.calendar("month", (2000, 1, 1), 4 * 365).labels)      # a copy was relabelled
    for wrong in ([], ["Juno"], [12], [-1], [1.5]):
        with pytest.raises(ValueError):
            months.restrict(wrong)


# -- the host twin
LABELS = {"rotating": np.array([t % 4 for t in range(13)]),                      # hour_of_day on a 6-hourly run
          "boundary": np.array([0] * 6 + [1] * 7),                               # a bin boundary inside a window
          "holes": np.array([2, 0, -1, 0, 1, -1, -1, 1, 3, 0, 3, -1, 1])}        # times that are not counted; bin 4 stays empty


@pytest.fixture(scope="module")
def integer_case():
    return tu.seeded_case(3, 2, 5, 7, 12, ("a", "b"), seed=11, integer=True)


@pytest.fixture(scope="module")
def real_case():
    return tu.seeded_case(3, 2, 5, 7, 12, ("a", "b"), seed=12, mean=3.0, std=40.0)


@pytest.mark.parametrize("per_member", [True, False])
def test_integer_sums_and_extremes_equal_numpy(sdy, integer_case, per_member):
    """Multiples of 2^-10 below 2^20: every float64 sum is exact, so the sums are numpy's int64 sums bit for bit."""
    case, labels, n_bins = integer_case, LABELS["holes"], 5
    state, counts = tu.host_state(case, tu.cut(case, [5, 8]), labels, n_bins, per_member)
    assert counts == [3, 3, 0, 2, 0]
    for j, name in enumerate(case["names"]):
        g = np.round(case["gen"][name].astype(np.float64) * 1024).astype(np.int64)
        y = np.round(case["target"][name].astype(np.float64) * 1024).astype(np.int64)
        assert np.array_equal(g / 1024.0, case["gen"][name].astype(np.float64))
        for b in range(n_bins):
            ts = [t for t in tu.counted(case, labels) if labels[t] == b]
            gs = g[:, :, ts].sum(axis=2) if per_member else g[:, :, ts].sum(axis=(0, 2))[None]
            assert np.array_equal(state["gen_sum"][b, j].reshape(gs.shape), gs.astype(np.float64) / 1024.0)
            assert np.array_equal(state["target_sum"][b, j], y[:, ts].sum(axis=1).astype(np.float64) / 1024.0)
            if not ts:          # an empty bin keeps what it was filled with
                assert np.all(state["gen_max"][b, j] == -np.inf) and np.all(state["gen_min"][b, j] == np.inf)
                assert np.all(state["target_max"][b, j] == -np.inf) and np.all(state["target_min"][b, j] == np.inf)
                continue
            gv, yv = case["gen"][name][:, :, ts], case["target"][name][:, ts]
            gmax = gv.max(axis=2) if per_member else gv.max(axis=(0, 2))[None]
            gmin = gv.min(axis=2) if per_member else gv.min(axis=(0, 2))[None]
            assert np.array_equal(state["gen_max"][b, j].reshape(gmax.shape), gmax)
            assert np.array_equal(state["gen_min"][b, j].reshape(gmin.shape), gmin)
            assert np.array_equal(state["target_max"][b, j], yv.max(axis=1)) and np.array_equal(state["target_min"][b, j], yv.min(axis=1))


@pytest.mark.parametrize("per_member", [True, False])
def test_real_sums_within_the_bound_of_a_sequential_sum(sdy, real_case, per_member):
    """Seeded fp32 data against exact rational arithmetic: |error| <= n 2^-53 sum |x| per element, n the terms of its chain."""
    case, labels, n_bins = real_case, LABELS["rotating"], 4
    state, _ = tu.host_state(case, tu.cut(case, [13]), labels, n_bins, per_member, extremes=False)
    worst = 0.0
    for j, name in enumerate(case["names"][:1]):
        g = case["gen"][name]
        for b in range(n_bins):
            ts = [t for t in tu.counted(case, labels) if labels[t] == b]
            for s in range(case["B"]):
                for p in range(0, case["H"] * case["W"], 3):
                    lat, lon = divmod(p, case["W"])
                    chains = [[g[m, s, t, lat, lon] for t in ts for m in range(case["M"])]] if not per_member else \
                        [[g[m, s, t, lat, lon] for t in ts] for m in range(case["M"])]
                    for r, xs in enumerate(chains):
                        exact = sum(Fraction(float(x)) for x in xs)
                        bound = len(xs) * Fraction(1, 2 ** 53) * sum(abs(Fraction(float(x))) for x in xs)
                        got = Fraction(float(state["gen_sum"][b, j, r * case["B"] + s if per_member else s, lat, lon]))
                        assert abs(got - exact) <= bound
                        worst = max(worst, float(abs(got - exact) / bound)) if bound else worst
    print(f"worst error / bound: {worst:.3f}")


@pytest.mark.parametrize("which", sorted(LABELS))
@pytest.mark.parametrize("per_member", [True, False])
def test_bits_do_not_depend_on_the_windows_or_the_group_order(sdy, real_case, which, per_member):
    case, labels, n_bins = real_case, LABELS[which], 5
    one, n_one = tu.host_state(case, tu.cut(case, [13]), labels, n_bins, per_member)
    many, n_many = tu.host_state(case, tu.cut(case, tu.SPLIT), labels, n_bins, per_member)
    assert n_one == n_many and sum(n_one) == sum(1 for t in range(1, 13) if labels[t] >= 0)
    assert tu.same_state(one, many)
    back, _ = tu.host_state(case, tu.cut(case, [13]), labels, n_bins, per_member, reorder=lambda g: g[::-1])
    rolled, _ = tu.host_state(case, tu.cut(case, [6, 7]), labels, n_bins, per_member, reorder=lambda g: g[1:] + g[:1])
    assert tu.same_state(one, back) and tu.same_state(one, rolled)
    # ... and is the chain in run order: float64, one addition per time (per member, pooled), into the accumulator itself
    for b in range(n_bins):
        ts = [t for t in tu.counted(case, labels) if labels[t] == b]
        acc = np.zeros((case["M"] if per_member else 1, case["B"], case["H"], case["W"]))
        for t in ts:
            if per_member:
                acc = acc + case["gen"]["a"][:, :, t].astype(np.float64)
            else:
                for m in range(case["M"]):
                    acc = acc + case["gen"]["a"][m, :, t].astype(np.float64)[None]
        assert np.array_equal(one["gen_sum"][b, 0].reshape(acc.shape), acc)


def test_more_counted_times_than_one_call_takes(sdy):
    """70 counted times in one window: the host cuts it into calls of 64 and 6, the bits of 70 windows of one time."""
    from sdy_amd import time_bins

    case = tu.seeded_case(2, 1, 3, 5, 70, ("a",), seed=13)
    labels = np.array([t % 3 for t in range(71)])
    calls = time_bins.group_times(labels[:71], 1)
    assert [sum(len(ts) for _, ts in c) for c in calls] == [64, 6] and [b for b, _ in calls[0]] == [1, 2, 0]
    assert all(list(ts) == sorted(ts) for c in calls for _, ts in c)
    one, n_one = tu.host_state(case, tu.cut(case, [71]), labels, 3)
    many, n_many = tu.host_state(case, tu.cut(case, [1] * 71), labels, 3)
    assert n_one == n_many == [23, 24, 23] and tu.same_state(one, many)


def test_nan_and_empty_bin_rules(sdy, real_case):
    """A NaN makes the sum and both extremes of its bin and element NaN from then on, and touches nothing else."""
    case = dict(real_case, gen={k: v.copy() for k, v in real_case["gen"].items()})
    labels, n_bins = LABELS["boundary"], 3
    case["gen"]["b"][1, 0, 2, 3, 4] = np.nan                      # time 2: bin 0; later times of bin 0 follow it
    clean, _ = tu.host_state(real_case, tu.cut(real_case, [4, 9]), labels, n_bins)
    dirty, counts = tu.host_state(case, tu.cut(case, [4, 9]), labels, n_bins)
    assert counts == [5, 7, 0]
    hit = np.zeros(clean["gen_sum"].shape, bool)
    hit[0, 1, 1 * case["B"] + 0, 3, 4] = True
    for k in ("gen_sum", "gen_max", "gen_min"):
        assert np.isnan(dirty[k][hit]).all() and np.array_equal(dirty[k][~hit], clean[k][~hit]), k
    assert tu.same_state(dirty, clean, keys=("target_sum", "target_max", "target_min"))
    assert np.all(dirty["gen_max"][2] == -np.inf) and np.all(dirty["target_min"][2] == np.inf) and np.all(dirty["gen_sum"][2] == 0.0)
    # pooled: the NaN of one member is the NaN of the sample's element
    pooled, _ = tu.host_state(case, tu.cut(case, [4, 9]), labels, n_bins, per_member=False)
    assert np.isnan(pooled["gen_max"][0, 1, 0, 3, 4]) and np.isnan(pooled["gen_min"][0, 1, 0, 3, 4]) and np.isnan(pooled["gen_sum"][0, 1, 0, 3, 4])
    assert int(np.isnan(pooled["gen_sum"]).sum()) == 1 and int(np.isnan(pooled["gen_max"]).sum()) == 1


def _call(sdy, case, edit, groups=((1, (1, 3)), (0, (2,))), n_bins=3, extremes=True):
    """One call on the first 4 times of the case with `edit(a)` applied -> (status of the twin, of the device entry point,
    whether the state is untouched)."""
    state = tu.empty_state(case, n_bins)
    before = {k: v.copy() for k, v in state.items()}
    target = {k: v[:, :4] for k, v in case["target"].items()}
    gen = {k: v[:, :, :4] for k, v in case["gen"].items()}
    a, keep = tu.host_args(target, gen, state, n_bins, groups, extremes=extremes)
    edit(a)
    host = sdy.lib.sdy_binned_time_accumulate_host(C.byref(a))
    return host, sdy.lib.sdy_binned_time_accumulate(C.byref(a), None), tu.same_state(state, before)


def _set(name, value):
    def edit(a):
        if isinstance(name, tuple):
            getattr(a, name[0])[name[1]] = value
        elif isinstance(value, str):
            setattr(a, name, getattr(a, name) + int(value))
        else:
            setattr(a, name, value)
    return edit


REFUSED = [
    ("struct_size", 0, SDY_ERR_ARG), ("struct_size", "+8", SDY_ERR_ARG), ("struct_size", "-8", SDY_ERR_ARG),
    # what sdy_window_check refuses
    ("nvars", 0, SDY_ERR_ARG), ("nvars", 97, SDY_ERR_ARG), (("gen", 1), None, SDY_ERR_ARG), (("target", 0), None, SDY_ERR_ARG),
    ("gs0", -1, SDY_ERR_ARG), ("gs1", -1, SDY_ERR_ARG), ("ts1", -1, SDY_ERR_ARG), ("n0", 0, SDY_ERR_ARG), ("n1", 0, SDY_ERR_ARG),
    ("T", 0, SDY_ERR_ARG), ("HW", 0, SDY_ERR_ARG), ("T", (1 << 30) // 35 + 1, SDY_ERR_UNSUPPORTED),
    # the bins and the groups
    ("n_bins", 0, SDY_ERR_ARG), ("bin_vars", 1, SDY_ERR_ARG), ("n_groups", -1, SDY_ERR_ARG), ("n_groups", 65, SDY_ERR_ARG),
    (("group_bin", 0), 3, SDY_ERR_ARG), (("group_bin", 1), -1, SDY_ERR_ARG),
    (("group_bin", 1), 1, SDY_ERR_ARG),                                   # a bin listed twice
    (("times", 0), 4, SDY_ERR_ARG), ("T", 3, SDY_ERR_ARG),                # a time outside the window
    (("times", 2), 3, SDY_ERR_ARG),                                       # a time listed twice, in two groups
    (("times", 1), 1, SDY_ERR_ARG),                                       # ... and in one
    (("times", 0), 3, SDY_ERR_ARG),                                       # a group that is not ascending
    (("group_end", 1), 2, SDY_ERR_ARG),                                   # an empty group
    (("group_end", 0), 0, SDY_ERR_ARG), (("group_end", 1), 65, SDY_ERR_ARG),
    # the accumulators
    ("gen_sum", None, SDY_ERR_ARG), ("target_sum", None, SDY_ERR_ARG), ("gen_sum", "+4", SDY_ERR_ARG), ("target_sum", "+2", SDY_ERR_ARG),
    ("gen_max", None, SDY_ERR_ARG), ("gen_min", None, SDY_ERR_ARG), ("target_max", None, SDY_ERR_ARG), ("target_min", None, SDY_ERR_ARG),
    ("gen_max", "+2", SDY_ERR_ARG), ("target_min", "+1", SDY_ERR_ARG),
]


@pytest.mark.parametrize("name,value,code", REFUSED, ids=[f"{n}={v}" for n, v, _ in REFUSED])
def test_refusals_write_nothing(sdy, integer_case, name, value, code):
    """Both entry points refuse before anything is read, written or launched (no GPU here: a launch would not return a code of
    the library's)."""
    host, device, untouched = _call(sdy, integer_case, _set(name, value))
    assert (host, device) == (code, code) and untouched


def test_accumulator_index_bound_and_the_calls_that_pass(sdy, integer_case):
    def huge(a):                       # 2^30 bins x 2^20 variables x 280 elements >= 2^50
        a.n_bins, a.bin_vars = 1 << 30, 1 << 20
    assert _call(sdy, integer_case, huge) == (SDY_ERR_UNSUPPORTED, SDY_ERR_UNSUPPORTED, True)
    assert sdy.lib.sdy_binned_time_accumulate_host(None) == SDY_ERR_ARG and sdy.lib.sdy_binned_time_accumulate(None, None) == SDY_ERR_ARG
    # a window with no counted time: SDY_OK from both, nothing launched (no GPU here), nothing written
    assert _call(sdy, integer_case, lambda a: None, groups=()) == (SDY_OK, SDY_OK, True)
    # without extremes all four pointers are NULL; the untouched call changes the state
    host, _, untouched = _call(sdy, integer_case, lambda a: None, extremes=False)
    assert host == SDY_OK and not untouched


def test_struct_and_bindings(sdy):
    from sdy_amd import _lib

    t = _lib.SdyBinnedSumArgs
    assert t not in _lib.ABI_STRUCTS and t().struct_size == C.sizeof(t) and t._fields_[0][0] == "struct_size"
    assert t._fields_[1][0] == "win" and _lib.SDY_BIN_MAX_TIMES == 64
    assert C.sizeof(t) + 8 <= 4096                     # with the item count inside the kernel-argument limit, 96 variables in it
    assert sdy.BinnedTimeMeanAggregator is sdy.time_bins.BinnedTimeMeanAggregator and sdy.TimeBins is sdy.time_bins.TimeBins
    assert callable(sdy.time_bins.binned_time_mean)
    import torch

    with pytest.raises(RuntimeError, match="GPU only"):
        sdy.time_bins.binned_time_mean(torch.zeros(3, 4, 5), [0, 1, 0])
    agg = sdy.BinnedTimeMeanAggregator(sdy.TimeBins.from_labels([0, 1, 0]), torch.ones(4, 5))
    x = {"a": torch.zeros(1, 3, 4, 5)}
    with pytest.raises(RuntimeError, match="GPU only"):
        agg.record_batch(0.0, x, x, i_time_start=0)
    assert agg._names is None and agg.counts() == [0, 0]
    for wrong in (dict(bins=[0, 1]), dict(target="raw"), dict(variables=[])):
        with pytest.raises(ValueError):
            sdy.BinnedTimeMeanAggregator(**{**dict(bins=sdy.TimeBins.from_labels([0, 1]), area_weights=torch.ones(4, 5)), **wrong})
