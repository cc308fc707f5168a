"""The checks every entry point that embeds an `sdy_event_thresholds` or an `sdy_lead_slots` shares (csrc/event_thresholds.h),
without a GPU: the _host twins refuse a call with one broken field of either descriptor and leave the accumulators alone, the
layout of the embedding structures, and the Python side's `fill_slots` and `EventAccumulator._fill`.

Every case: one variable, 2 members, one sample, T = 2 times on a 2 x 4 grid, two events (a scalar "above" and a (2, 4) map
"below"), accumulators prefilled with 7."""
import ctypes as C

import numpy as np
import pytest
import torch

import event_verif_utils as ev
import fss_utils as fu
import rank_hist_utils as ru
import spell_utils as su

SDY_ERR_ARG = -1
M, T, H, W, E = 2, 2, 2, 4, 2


def _case():
    rng = np.random.default_rng(1)
    target = {"a": rng.standard_normal((1, T, H, W)).astype(np.float32)}
    gen = {"a": rng.standard_normal((M, 1, T, H, W)).astype(np.float32)}
    events = {"a": [("high", "above", 0.25), ("low", "below", rng.standard_normal((H, W)).astype(np.float32))]}
    return dict(events=events, radii=(0, 1)), target, gen


def _call(which):
    """A valid call (both times counted, one slot per time) -> (host entry point, args, accumulators, keep-alive)."""
    import sdy_amd

    case, target, gen = _case()
    if which == "rank_hist":
        acc = [np.full((1, T, H, M + 1), 7.0), np.full((1, T, H), 7.0)]
        a, keep = ru.args(target, gen, ["a"], 0, 0, T, False, *acc)
        return sdy_amd.lib.sdy_rank_hist_accumulate_host, a, acc, keep
    if which == "event_table":
        acc = [np.full((1, T, E, H, 2, M + 1), 7.0)]
        a, keep = ev.args(case, target, gen, ["a"], 0, 0, T, False, acc[0])
        return sdy_amd.lib.sdy_event_table_accumulate_host, a, acc, keep
    if which == "event_frequency":
        acc = [np.full((1, E, 3, H, W), 7.0)]
        a, keep = ev.args(case, target, gen, ["a"], 0, 0, T, False, acc[0])
        return sdy_amd.lib.sdy_event_frequency_accumulate_host, a, acc, keep
    if which == "fss":
        acc = [np.full((1, T, E, len(case["radii"]), H, 6), 7.0)]
        a, keep = fu.args(case, target, gen, ["a"], 0, 0, T, False, acc[0])
        return sdy_amd.lib.sdy_fss_accumulate_host, a, acc, keep
    acc = [np.full((1, E, 4, (M + 1) * 1, H, W), 7, np.uint32), np.full((1, E, 2, H, 16), 7.0)]
    a, keep = su.args(case, target, gen, ["a"], 0, *acc)
    return sdy_amd.lib.sdy_event_spell_accumulate_host, a, acc, keep


def _untouched(acc):
    return all((x == 7).all() for x in acc)


def _break_thresholds(thr, field, value):
    if field == "map_first0":
        thr.map_first[0] = value
    elif value == "odd":                                      # off a 4-byte boundary
        setattr(thr, field, getattr(thr, field) + 2)
    else:
        setattr(thr, field, value)


BROKEN_THRESHOLDS = [("n_events", 0), ("n_events", 9), ("n_events", -1), ("scalars", None), ("scalars", "odd"), ("maps", None),
                     ("maps", "odd"), ("n_maps", 0), ("map_first0", -1), ("map_first0", 1)]


@pytest.mark.parametrize("which", ["event_table", "event_frequency", "fss", "spells"])
def test_host_twins_refuse_broken_thresholds(which):
    host, a, acc, keep = _call(which)
    assert (a.thr.n_events, a.thr.n_maps, a.thr.below[0], a.thr.is_map[0], a.thr.map_first[0]) == (E, 1, 2, 2, 0)
    for field, value in BROKEN_THRESHOLDS:
        host, a, acc, keep = _call(which)
        _break_thresholds(a.thr, field, value)
        assert host(C.byref(a)) == SDY_ERR_ARG, (field, value)
        assert _untouched(acc), (field, value)
    host, a, acc, keep = _call(which)                          # the valid call goes through, and writes
    assert host(C.byref(a)) == 0 and not _untouched(acc)


# (T = 2 window times against the n_slots = 2 of the valid call)
BROKEN_SLOTS = [dict(n_slots=0), dict(t0=-1), dict(t0=T + 1), dict(t_start=-1), dict(t_start=1), dict(pool_times=1, n_slots=2)]


@pytest.mark.parametrize("which", ["rank_hist", "event_table", "event_frequency", "fss"])
def test_host_twins_refuse_broken_slots(which):
    host, a, acc, keep = _call(which)
    assert (a.slots.t0, a.slots.t_start, a.slots.n_slots, a.slots.pool_times, a.win.T) == (0, 0, T, 0, T)
    for fields in BROKEN_SLOTS:
        host, a, acc, keep = _call(which)
        for field, value in fields.items():
            setattr(a.slots, field, value)
        assert host(C.byref(a)) == SDY_ERR_ARG, fields
        assert _untouched(acc), fields
    host, a, acc, keep = _call(which)
    assert host(C.byref(a)) == 0 and not _untouched(acc)


def test_layout():
    from sdy_amd import _lib

    assert [C.sizeof(t) for t in (_lib.SdyEventArgs, _lib.SdyFssArgs, _lib.SdyRankHistArgs)] == [2216, 2256, 1624]
    assert _lib.SdyEventArgs.thr.offset == _lib.SdyFssArgs.thr.offset == 1608
    assert _lib.SdyEventArgs.slots.offset == _lib.SdyFssArgs.slots.offset == _lib.SdyRankHistArgs.slots.offset == 1592
    assert _lib.SdyEventArgs.scalars.offset == _lib.SdyFssArgs.scalars.offset == 2192
    assert (_lib.SdyEventArgs.acc.offset, _lib.SdyFssArgs.acc.offset) == (2208, 2232)
    for t in (_lib.SdyEventArgs, _lib.SdyFssArgs, _lib.SdyEventSpellArgs):
        assert dict(t._fields_)["thr"] is _lib.SdyEventThresholds, t
    for t in (_lib.SdyEventArgs, _lib.SdyFssArgs, _lib.SdyRankHistArgs):
        assert dict(t._fields_)["slots"] is _lib.SdyLeadSlots, t
    assert "slots" not in dict(_lib.SdyEventSpellArgs._fields_) and "thr" not in dict(_lib.SdyRankHistArgs._fields_)
    assert len(_lib.ABI_STRUCTS) == 25                         # like SdyWindow, the descriptors are not argument structures
    assert _lib.SdyEventThresholds not in _lib.ABI_STRUCTS and _lib.SdyLeadSlots not in _lib.ABI_STRUCTS


def test_fill_slots_and_event_fill():
    import sdy_amd
    from sdy_amd._lib import SdyEventArgs, SdyEventSpellArgs, SdyRankHistArgs
    from sdy_amd.windows import fill_slots

    a = SdyRankHistArgs()
    fill_slots(a.slots, 1, 0, 6, False)
    own = lambda a: (a.t0, a.t_start, a.n_slots, a.pool_times)  # noqa: E731  (the slots' fields as the structure's own)
    assert (a.slots.t0, a.slots.t_start, a.slots.n_slots, a.slots.pool_times) == own(a) == (1, 0, 6, 0)
    fill_slots(a.slots, 0, 4, 1, True)                         # pooled: one slot, the start of the window is not looked at
    assert own(a) == (0, 0, 1, 1)

    # two variables of one run; the second one's map follows the first one's: map_first = 1
    maps = {k: torch.full((H, W), float(i)) for i, k in enumerate("ab")}
    events = sdy_amd.Events()
    events.add("a", "high", above=0.25)
    events.add("a", "low", below=maps["a"])
    events.add("b", "high", above=maps["b"])
    events.add("b", "low", below=-0.5)
    agg = sdy_amd.EventVerificationAggregator(events, torch.ones(H, W), n_timesteps=6)
    target = {k: torch.zeros(1, T, H, W) for k in "ab"}
    gen = {k: torch.zeros(M, 1, T, H, W) for k in "ab"}
    names, lay = agg._layouts(target, gen)
    agg._build_thresholds(names, lay, "cpu")
    agg._names = names
    a = SdyEventArgs()
    agg._fill(a, lay, 0, 2, 0, 3)
    assert (a.win.nvars, a.H, a.W) == (2, H, W)
    assert (a.slots.t0, a.slots.t_start, a.slots.n_slots, a.slots.pool_times) == own(a) == (0, 3, 6, 0)
    assert (a.thr.n_events, a.thr.n_maps) == (a.n_events, a.n_maps) == (2, 2)
    assert [a.thr.below[j] for j in range(2)] == [a.below[j] for j in range(2)] == [2, 2]
    assert [a.thr.is_map[j] for j in range(2)] == [a.is_map[j] for j in range(2)] == [2, 1]
    assert [a.thr.map_first[j] for j in range(2)] == [a.map_first[j] for j in range(2)] == [0, 1]
    assert a.thr.scalars == a.scalars == agg._scalars.data_ptr() and a.thr.maps == a.maps == agg._maps.data_ptr()
    assert torch.equal(agg._maps.view(2, H, W), torch.stack([maps["a"], maps["b"]]))
    s = SdyEventSpellArgs()                                    # no slots: the first counted time is the structure's own
    agg._fill(s, lay, 1, 2, 1, 0)
    assert (s.win.nvars, s.t0, s.thr.n_events, s.thr.n_maps, s.thr.is_map[0], s.thr.map_first[0]) == (1, 1, 2, 1, 1, 0)
    assert s.thr.scalars == agg._scalars.data_ptr() + 8 and s.thr.maps == agg._maps.data_ptr() + 4 * H * W
