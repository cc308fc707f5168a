"""Verification of threshold events of an ensemble rollout on the device: Brier score and its Murphy decomposition, the
reliability diagram, the ROC curve and exceedance-frequency maps.  The reference has nothing of the kind; the rank histograms
say whether an ensemble is calibrated as a whole, this says whether its probability of a particular event -- rain above 1
mm/day, surface pressure below 980 hPa -- is reliable, whether it discriminates, and how much better it is than the base rate.

For an M-member ensemble the forecast probability of an event takes the values k / M only, so the whole verification follows
from an integer table of counts per (members in the event, truth in the event or not): the device accumulates the table
exactly, every score is a few float64 operations on it at read-out (`scores`).

Neighbourhood (fractions-skill) scores of the same events: `sdy_amd.fss`; how long an event lasts along a trajectory (spell
durations): `sdy_amd.spells`; threshold maps from the quantiles along time of a run: `sdy_amd.quantiles`.  Out of scope: events
over several variables, plots.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, NamedTuple, Optional, Sequence

import torch

from ._lib import SDY_EVENT_MAX, SDY_EVENT_MAX_MEMBERS, SdyEventArgs, check, current_stream, lib
from .windows import FieldAccumulator, WindowLayout, fill_slots, fill_window, runs, whole_ics_message, window_layouts

#: what `EventVerificationAggregator.get_logs` reports per variable and event, in this order
LOG_METRICS = ("brier_score", "brier_skill_score", "brier_reliability", "brier_resolution", "base_rate", "forecast_rate",
               "roc_area")
#: what `get_data` reports per slot, in this order (after `table`, before `reliability_curve`)
SLOT_METRICS = ("brier_score", "brier_reliability", "brier_resolution", "uncertainty", "base_rate", "forecast_rate", "roc_area")


class Event(NamedTuple):
    """One event of a variable: `x < threshold` when `below`, else `x > threshold`; the threshold is an fp32 scalar, or an
    `(H, W)` fp32 map on the host (`scalar` is None then)."""
    name: str
    below: bool
    scalar: Optional[float]
    map: Optional[torch.Tensor]


class Events:
    """The events to verify, per variable, in insertion order.

    `add(variable, name, above=c)` or `add(variable, name, below=c)`: a value x is in the event when x > c (x < c), strictly;
    a NaN x never is.  c is a finite Python float, or an `(H, W)` array or tensor (rounded once to fp32) whose NaN points are
    masked for this event.  At most 8 events per variable.  A map whose shape does not match the variable's grid is refused at
    the first window.  `sdy_amd.TimeQuantileAggregator.threshold_map` builds such maps from the quantiles of a run; events over
    several variables are out of scope."""

    def __init__(self):
        self._events: Dict[str, List[Event]] = {}

    def add(self, variable: str, name: str, above=None, below=None) -> "Events":
        if (above is None) == (below is None):
            raise ValueError(f"event {name!r} of {variable!r}: give exactly one of above= and below=")
        if not isinstance(name, str) or len(name) == 0 or "/" in name:
            raise ValueError(f"event name {name!r}: a non-empty string without '/'")
        have = self._events.get(variable, [])
        if any(e.name == name for e in have):
            raise ValueError(f"{variable!r} already has an event {name!r}")
        if len(have) >= SDY_EVENT_MAX:
            raise ValueError(f"at most {SDY_EVENT_MAX} events per variable, {variable!r} has {len(have)}")
        c = above if below is None else below
        m = torch.as_tensor(c).detach().to("cpu", torch.float32).contiguous()         # rounded once to fp32
        if m.dim() == 0:
            value = float(m)
            if not math.isfinite(value):
                raise ValueError(f"event {name!r} of {variable!r}: the threshold {c!r} is not a finite fp32 number")
            event = Event(name, below is not None, value, None)
        else:
            if m.dim() != 2:
                raise ValueError(f"event {name!r} of {variable!r}: a threshold is a number or a (lat, lon) map, got shape "
                                 f"{tuple(m.shape)}")
            event = Event(name, below is not None, None, m.clone())
        self._events.setdefault(variable, []).append(event)
        return self

    @property
    def variables(self) -> List[str]:
        return list(self._events)

    def of(self, variable: str) -> List[Event]:
        return list(self._events.get(variable, ()))

    def __len__(self) -> int:
        return sum(len(v) for v in self._events.values())


def scores(table: torch.Tensor, lat_weights: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The scores of a table of counts `(..., lat, 2, M + 1)` -- `table[..., lat, o, k]` counted points with k of M members in
    the event and the truth in it (o = 1) or not -- under `(lat,)` weights; float64 on the table's device, CPU included.

    With N_k = sum over lat and o of w_lat x table, O_k its o = 1 part, N = sum N_k, O = sum O_k and p_k = k / M:
    `base_rate` b = O / N;  `forecast_rate` = sum N_k p_k / N;  `brier_score` = sum [(N_k - O_k) p_k^2 + O_k (1 - p_k)^2] / N;
    `brier_reliability` = sum N_k (p_k - O_k / N_k)^2 / N and `brier_resolution` = sum N_k (O_k / N_k - b)^2 / N over the bins
    with N_k > 0;  `uncertainty` = b (1 - b)  (brier_score = reliability - resolution + uncertainty);  `brier_skill_score` = 1 -
    brier_score / uncertainty, NaN when the uncertainty is 0;  `reliability_curve` `(..., M + 1)` = O_k / N_k, NaN for a bin
    without forecasts;  `roc_area`: the trapezoid area under the points (false-alarm rate, hit rate) of warning when k >= j, j
    = M + 1, M, .., 0 -- hit rate sum_{k>=j} O_k / O, false-alarm rate sum_{k>=j} (N_k - O_k) / (N - O) -- NaN when O = 0 or O =
    N.  Everything else `(...)`.  Without counts everything is NaN."""
    t = table.to(torch.float64)
    w = lat_weights.to(device=t.device, dtype=torch.float64)
    if t.dim() < 3 or t.shape[-2] != 2 or t.shape[-3] != w.numel():
        raise ValueError(f"a table is (..., lat, 2, M + 1) with (lat,) weights, got {tuple(t.shape)} and {tuple(w.shape)}")
    ok = (t * w[:, None, None]).sum(dim=-3)                       # (..., 2, M + 1)
    n_k, o_k = ok.sum(dim=-2), ok[..., 1, :]
    M = n_k.shape[-1] - 1
    p = torch.arange(M + 1, dtype=torch.float64, device=t.device) / max(M, 1)
    nan = torch.full_like(n_k[..., 0], float("nan"))
    n, o = n_k.sum(dim=-1), o_k.sum(dim=-1)
    base = o / n
    some = n_k > 0
    obar = torch.where(some, o_k / torch.where(some, n_k, torch.ones_like(n_k)), torch.full_like(n_k, float("nan")))
    obar0 = torch.where(some, obar, torch.zeros_like(obar))
    brier = ((n_k - o_k) * p * p + o_k * (1.0 - p) * (1.0 - p)).sum(dim=-1) / n
    rel = (n_k * (p - obar0) ** 2).sum(dim=-1) / n                # (a bin with N_k = 0 adds 0)
    base0 = torch.where(n > 0, base, torch.zeros_like(base))
    res = (n_k * (obar0 - base0[..., None]) ** 2).sum(dim=-1) / n
    unc = base * (1.0 - base)
    skill = torch.where(unc > 0, 1.0 - brier / torch.where(unc > 0, unc, torch.ones_like(unc)), nan)
    # ROC: warn when k >= j; from j = M + 1 (never: the origin) down to j = 0 (always: (1, 1))
    zero = torch.zeros_like(n_k[..., :1])
    hits = torch.cat([zero, o_k.flip(-1).cumsum(dim=-1)], dim=-1)
    false = torch.cat([zero, (n_k - o_k).flip(-1).cumsum(dim=-1)], dim=-1)
    both = (o > 0) & (o < n)
    hr = hits / torch.where(both, o, torch.ones_like(o))[..., None]
    far = false / torch.where(both, n - o, torch.ones_like(o))[..., None]
    area = (0.5 * (hr[..., 1:] + hr[..., :-1]) * (far[..., 1:] - far[..., :-1])).sum(dim=-1)
    return {"brier_score": brier, "brier_skill_score": skill, "brier_reliability": rel, "brier_resolution": res,
            "uncertainty": unc, "base_rate": base, "forecast_rate": (n_k * p).sum(dim=-1) / n,
            "roc_area": torch.where(both, area, nan), "reliability_curve": obar}


class _EventLayout(WindowLayout):
    """A `WindowLayout` that knows how many events its variable has (part of what one launch takes, and of the job)."""
    n_events = 0


class EventAccumulator(FieldAccumulator):
    """What `EventVerificationAggregator`, `sdy_amd.FractionsSkillAggregator` and `sdy_amd.EventSpellAggregator` share: the
    events of the variables and their thresholds on the device, the row-constant area weights, the slots, and everything a
    window is checked for before anything changes."""

    accepts_sample_weights = True      # (to see, and refuse, a ragged share)

    _job_words = "member count, sample count"

    def __init__(self, events: Events, area_weights: torch.Tensor, n_timesteps: int, pool_times: bool = False, dist=None,
                 metadata=None, max_bytes: Optional[int] = None):
        super().__init__(n_timesteps, dist=dist, metadata=metadata, max_bytes=max_bytes)
        who = type(self).__name__
        if not isinstance(events, Events) or len(events) == 0:
            raise ValueError(f"{who} needs an sdy_amd.Events with at least one event")
        if area_weights.dim() != 2:
            raise ValueError(f"area weights are (lat, lon), got {tuple(area_weights.shape)}")
        if not bool((area_weights == area_weights[:, :1]).all()):
            raise ValueError(f"{who}: the area weights vary along a latitude row; counts that are pooled "
                             "over longitudes cannot weight them exactly")
        self._events = {v: events.of(v) for v in events.variables}          # a copy: later add()s do not reach a running job
        self._area_weights = area_weights
        self._pool_times = bool(pool_times)
        self._n_slots = 1 if self._pool_times else self._n_timesteps
        self._scalars: Optional[torch.Tensor] = None      # device (sum of E,) fp32, NaN at the map events
        self._maps: Optional[torch.Tensor] = None         # device fp32: every map, variable by variable, event order
        self._scalar_at: List[int] = []                   # per variable: its first scalar / the float offset of its first map
        self._map_at: List[int] = []

    @staticmethod
    def _job(l: WindowLayout) -> tuple:
        return (l.n0, l.n1, l.H, l.W, l.n_events)

    def _layouts(self, target_data, gen_data):
        """-> (names, layouts) of the window's variables that have events, in window order."""
        if self._names is None:
            missing = [v for v in self._events if v not in gen_data]
            if missing:
                raise ValueError(f"no generated variable {missing[0]!r} in the window, but events are defined for it")
        names = [k for k in gen_data if k in self._events]
        if not names:
            raise ValueError("the window holds no variable with events")
        lay = []
        for k, l in zip(names, window_layouts(target_data, {k: gen_data[k] for k in names})):
            l = _EventLayout(*l)
            l.n_events = len(self._events[k])
            lay.append(l)
        return names, lay

    def _build_thresholds(self, names, lay, device) -> None:
        """Once, at the first accepted window: every scalar and every map to the device."""
        scalars, maps, at = [], [], 0
        for k, l in zip(names, lay):
            self._scalar_at.append(len(scalars))
            self._map_at.append(at)
            for e in self._events[k]:
                scalars.append(float("nan") if e.scalar is None else e.scalar)
                if e.map is not None:
                    maps.append(e.map.reshape(-1))
                    at += l.H * l.W
        self._scalars = torch.tensor(scalars, dtype=torch.float32).to(device)
        self._maps = torch.cat(maps).to(device) if maps else None

    def _fill(self, a, lay, first: int, last: int, t0: int, i_time_start: int) -> None:
        """Variables first .. last - 1 of a window (one run: equal extents and event count) into the window, the slots (of a
        structure that has them) and the thresholds of an argument structure; the accumulator is the caller's."""
        fill_window(a.win, lay, first, last)
        l = lay[first]
        a.H, a.W = l.H, l.W
        if hasattr(a, "slots"):
            fill_slots(a.slots, t0, i_time_start, self._n_slots, self._pool_times)
        else:
            a.t0 = t0
        thr = a.thr
        thr.n_events = l.n_events
        thr.scalars = self._scalars.data_ptr() + 4 * self._scalar_at[first]
        n_maps = 0
        for j in range(first, last):
            bits = [(e.below, e.map is not None) for e in self._events[self._names[j]]]
            thr.below[j - first] = sum(1 << i for i, (b, _) in enumerate(bits) if b)
            thr.is_map[j - first] = sum(1 << i for i, (_, m) in enumerate(bits) if m)
            thr.map_first[j - first] = (self._map_at[j] - self._map_at[first]) // (l.H * l.W)      # (a run has one grid)
            n_maps += sum(m for _, m in bits)
        thr.n_maps = n_maps
        thr.maps = self._maps.data_ptr() + 4 * self._map_at[first] if n_maps else None

    def _begin(self, target_data, gen_data, i_time_start: int, sample_weights):
        """Everything a window is checked for, the accumulators and the thresholds at the first accepted one -> (layouts, t0,
        device); t0: the first counted time (the very first time of a run is the initial condition)."""
        ragged = sample_weights is not None or any(
            g.dim() == 4 and k in target_data and target_data[k].dim() == 4 and g.shape[0] != target_data[k].shape[0]
            for k, g in gen_data.items())
        if ragged:
            raise ValueError(whole_ics_message(type(self).__name__))
        names, lay = self._layouts(target_data, gen_data)
        T = lay[0].T
        if i_time_start < 0 or i_time_start + T > self._n_timesteps:
            raise ValueError(f"times {i_time_start}..{i_time_start + T - 1} outside the aggregator's {self._n_timesteps}")
        if any(l.n0 > SDY_EVENT_MAX_MEMBERS for l in lay):
            raise ValueError(f"at most {SDY_EVENT_MAX_MEMBERS} members, got {max(l.n0 for l in lay)}")
        for k, l in zip(names, lay):
            for e in self._events[k]:
                if e.map is not None and tuple(e.map.shape) != (l.H, l.W):
                    raise ValueError(f"event {e.name!r} of {k!r}: a {tuple(e.map.shape)} threshold map against a "
                                     f"{(l.H, l.W)} grid")
        self._check_window(lay)
        device = self._prepare(names, lay)
        if self._scalars is None:
            self._build_thresholds(names, lay, device)
        return lay, (1 if i_time_start == 0 else 0), device

    def _check_window(self, lay) -> None:
        """What a subclass refuses on top, before anything changes."""

    def _reduced(self) -> Dict[str, torch.Tensor]:
        # (raised BEFORE any collective: every rank of a job must have recorded at least one window)
        if self._names is None:
            raise ValueError("No data recorded.")
        return {stat: self._dist.reduce_sum(acc) for stat, acc in self._acc.items()}

    def _lat_weights(self, i: int, device) -> torch.Tensor:
        H, W = self._grids[i][2:4]
        if tuple(self._area_weights.shape) != (H, W):
            raise ValueError(f"area weights {tuple(self._area_weights.shape)} against a {(H, W)} grid")
        return self._area_weights.to(device, torch.float64).mean(dim=1)


class EventVerificationAggregator(EventAccumulator):
    """Per variable, event, lead time and latitude: how many counted points had k of the M members in the event while the truth
    was (o = 1) or was not (o = 0) in it -- and everything that follows from that table.

    Definition (csrc/events.h).  A value x is in an event when x > c (above) or x < c (below), strictly; a NaN x never is.  A
    point (sample, time, lat, lon) is counted for an event when neither its target nor its threshold is NaN: a NaN in a
    threshold map masks the point for that event, a NaN member is simply not in the event.

    `record_batch(loss, target_data, gen_data, target_data_norm, gen_data_norm, i_time_start)` is what `run_inference` calls
    once per window: targets `(samples, time, lat, lon)`, gen `(members, samples, time, lat, lon)` (a 4-D gen is one member:
    a 2 x 2 contingency table).  Only the variables with events are read; one that is missing from the first window raises
    `ValueError`.  One `sdy_event_table_accumulate` launch per run of variables with equal extents and equal event count reads
    the window in place -- the member-stacked transposed view included -- and adds it to a float64 table `(n_slots, events,
    lat, 2, M + 1)` per variable on the device; `frequency_maps=True` adds one `sdy_event_frequency_accumulate` launch per run
    into `(events, 3, lat x lon)` maps of member hits, target hits and counted points, pooled over all lead times.  The
    thresholds go to the device once, at the first accepted window.  The slot of window time t is the lead time `i_time_start
    + t` of `n_timesteps`; `pool_times=True` keeps ONE slot.  The first time of a run (`i_time_start == 0`) is the initial
    condition and is not counted.  Counts are integers held as float64: the same bits in any layout, batch, run and rank
    count.  The first window that is accepted fixes variables, grids, member count and sample count; a later window with
    others raises `ValueError`, and a refused window changes nothing.  The denormalised data are read.

    `area_weights` is `(lat, lon)`, constant along a row (the weight of a latitude is its row's mean); others raise
    `ValueError` at construction.

    `get_data()` returns float64 device tensors, added over ranks (`dist.reduce_sum`: tables add, they are never averaged),
    per variable and event: `table/<event>/<var>` `(n_slots, lat, 2, M + 1)`; per slot `brier_score`, `brier_reliability`,
    `brier_resolution`, `uncertainty`, `base_rate`, `forecast_rate` and `roc_area` `(n_slots,)` and `reliability_curve`
    `(n_slots, M + 1)` (see `scores`); with `frequency_maps=True` also `frequency_gen` = member hits / (M x counted),
    `frequency_target` = target hits / counted (both NaN where nothing was counted) and `counted`, each `(lat, lon)`.
    `get_logs(label)` returns Python floats from the tables pooled over all slots, `<metric>/<event>/<variable>` for the
    metrics of `LOG_METRICS`.  Ranks hold whole initial conditions; ragged shares (flat rows with `sample_weights`) are
    refused.  Events over several variables and plots are out of scope; threshold maps: `sdy_amd.quantiles`; neighbourhood
    (fractions-skill) scores are `sdy_amd.FractionsSkillAggregator`, spell durations `sdy_amd.EventSpellAggregator`."""

    def __init__(self, events: Events, area_weights: torch.Tensor, n_timesteps: int, pool_times: bool = False,
                 frequency_maps: bool = False, dist=None, metadata=None, max_bytes: Optional[int] = None):
        super().__init__(events, area_weights, n_timesteps, pool_times=pool_times, dist=dist, metadata=metadata,
                         max_bytes=max_bytes)
        self._frequency_maps = bool(frequency_maps)

    def _statistics(self) -> Dict[str, float]:
        return {"table": 0.0, "maps": 0.0} if self._frequency_maps else {"table": 0.0}

    def _elements(self, stat: str, job: tuple) -> int:
        M, _, H, W, E = job
        return self._n_slots * E * H * 2 * (M + 1) if stat == "table" else E * 3 * H * W

    def _size_words(self, names, jobs) -> str:
        return f"{sum(j[4] for j in jobs)} events of {len(names)} variables, {jobs[0][0]} members x {self._n_slots} slots"

    def _args(self, lay, first: int, last: int, t0: int, i_time_start: int, stat: str) -> SdyEventArgs:
        a = SdyEventArgs()
        self._fill(a, lay, first, last, t0, i_time_start)
        a.acc = self._at(stat, first)
        return a

    @torch.no_grad()
    def record_batch(self, loss, target_data, gen_data, target_data_norm=None, gen_data_norm=None, i_time_start: int = 0,
                     sample_weights: Optional[Sequence[float]] = None):
        del loss, target_data_norm, gen_data_norm
        i_time_start = int(i_time_start)
        lay, t0, device = self._begin(target_data, gen_data, i_time_start, sample_weights)
        with torch.cuda.device(device):
            for first, last in runs(lay, lambda l: (l.extents, l.n_events)):
                a = self._args(lay, first, last, t0, i_time_start, "table")
                check(lib.sdy_event_table_accumulate(C.byref(a), current_stream()), "sdy_event_table_accumulate")
                if self._frequency_maps:
                    a.acc = self._at("maps", first)
                    check(lib.sdy_event_frequency_accumulate(C.byref(a), current_stream()), "sdy_event_frequency_accumulate")
        for t in range(i_time_start + t0, i_time_start + lay[0].T):
            self._n_batches[t] += 1

    def _table(self, acc: Dict[str, torch.Tensor], i: int) -> torch.Tensor:
        """-> the (n_slots, E, lat, 2, M + 1) table of variable i inside the flat (reduced) buffer."""
        M, _, H, _, E = self._grids[i]
        at = self._offsets["table"][i]
        return acc["table"][at:at + self._n_slots * E * H * 2 * (M + 1)].view(self._n_slots, E, H, 2, M + 1)

    @torch.no_grad()
    def get_data(self) -> Dict[str, torch.Tensor]:
        acc = self._reduced()
        data: Dict[str, torch.Tensor] = {}
        for i, name in enumerate(self._names):
            M, _, H, W, E = self._grids[i]
            table = self._table(acc, i)
            w = self._lat_weights(i, table.device)
            for e, event in enumerate(self._events[name]):
                tail = f"{event.name}/{name}"
                s = scores(table[:, e], w)
                data[f"table/{tail}"] = table[:, e]
                for metric in SLOT_METRICS:
                    data[f"{metric}/{tail}"] = s[metric]
                data[f"reliability_curve/{tail}"] = s["reliability_curve"]
                if self._frequency_maps:
                    at = self._offsets["maps"][i] + e * 3 * H * W
                    hits, obs, counted = acc["maps"][at:at + 3 * H * W].view(3, H, W)
                    data[f"frequency_gen/{tail}"] = hits / (M * counted)
                    data[f"frequency_target/{tail}"] = obs / counted
                    data[f"counted/{tail}"] = counted
        return data

    @torch.no_grad()
    def get_logs(self, label: str) -> Dict[str, float]:
        acc = self._reduced()
        parts = []
        for i in range(len(self._names)):
            table = self._table(acc, i)
            w = self._lat_weights(i, table.device)
            parts.append((w[None, :, None, None] * table.sum(dim=0)).sum(dim=1).reshape(-1))      # (E, 2, M + 1)
        packed = torch.cat(parts).cpu()                # every event's weighted table in one copy
        logs: Dict[str, float] = {}
        at, one = 0, torch.ones(1, dtype=torch.float64)
        for i, name in enumerate(self._names):
            M, E = self._grids[i][0], self._grids[i][4]
            for event in self._events[name]:
                s = scores(packed[at:at + 2 * (M + 1)].view(1, 2, M + 1), one)
                at += 2 * (M + 1)
                for metric in LOG_METRICS:
                    logs[f"{metric}/{event.name}/{name}"] = float(s[metric])
        return {f"{label}/{k}": v for k, v in logs.items()} if len(label) != 0 else logs
