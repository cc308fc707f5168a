"""Spell durations of threshold events along every trajectory of a rollout, on the device: whether an event LASTS as long
as it should -- consecutive dry days (the longest run of pr < 1 mm/day), warm spells above a percentile map, blocking.  The
reference has nothing of the kind.  `EventVerificationAggregator` says whether the ensemble's probability of an event is
reliable and `FractionsSkillAggregator` whether it sits in the right place; `TimeVariabilityAggregator` gives the linear memory
of a value, which the persistence of a threshold event is not a function of.  The definition is `csrc/spells.h`: integers and
comparisons only, so every count has the same bits in any layout, batch, run and cut of the run into windows.

Out of scope: per-point duration histograms, spells of the ensemble mean or of several variables, a minimum-duration rule
(heat waves of at least three days), plots, ragged rank shares.  Threshold maps from the quantiles of a run:
`sdy_amd.quantiles.TimeQuantileAggregator.threshold_map`.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence

import torch

from ._lib import SDY_SPELL_BINS, SdyEventSpellArgs, check, current_stream, lib, ptr
from .events import EventAccumulator, Events
from .windows import runs

#: the 32-bit words of a state element, in this order (csrc/spells.h)
STATE_WORDS = ("run", "longest", "spells", "hits")
#: what `EventSpellAggregator.get_logs` reports per variable and event, in this order
LOG_METRICS = ("mean_duration_gen", "mean_duration_target", "mean_duration_ratio", "longest_gen", "longest_target",
               "longest_bias", "onset_rate_gen", "onset_rate_target", "time_fraction_gen", "time_fraction_target")
#: the columns of `rows` (`get_data`), in this order
ROW_SUMS = ("hits", "spells", "longest", "points")
#: the most counted times a run may have: the state words are 32 bits, and `hits` counts up to all of them
MAX_TIMES = 2 ** 31 - 1


def duration_edges() -> torch.Tensor:
    """The 15 edges 1, 2, 4, .., 16384 of the 16 duration bins (int64): bin(d) = the number of edges < d."""
    return 2 ** torch.arange(SDY_SPELL_BINS - 1, dtype=torch.int64)


def duration_bin(d: torch.Tensor) -> torch.Tensor:
    """The bin of every duration d >= 1 of an integer tensor: 1 -> 0, 2 -> 1, 3..4 -> 2, 5..8 -> 3, .., > 16384 -> 15."""
    return torch.bucketize(d.to(torch.int64), duration_edges().to(d.device))


def logs_from_rows(rows, lat_weights, n_times: int) -> Dict[str, float]:
    """One (variable, event)'s logs from its `rows` `(2, lat, 4)` -- per side and latitude the integer sums over the counted
    points of hits, spells, longest and trajectory-points, already added over ranks -- the `(lat,)` weights and the counted
    times n, in the order of `LOG_METRICS`.  With S_x = sum over lat of w x: mean duration S_hits / S_spells (NaN without
    spells), longest S_longest / S_points, onset rate S_spells / (n S_points), time fraction S_hits / (n S_points)."""
    rows = torch.as_tensor(rows, dtype=torch.float64).cpu()
    w = torch.as_tensor(lat_weights, dtype=torch.float64).cpu()
    s = (w[None, :, None] * rows).sum(dim=1).tolist()              # (2, 4)
    nan = float("nan")
    out: Dict[str, float] = {}
    side = {}
    for i, which in enumerate(("gen", "target")):
        hits, spells, longest, points = s[i]
        side[which] = (hits / spells if spells > 0.0 else nan, longest / points if points > 0.0 else nan,
                       spells / (n_times * points) if points > 0.0 else nan, hits / (n_times * points) if points > 0.0 else nan)
    g, t = side["gen"], side["target"]
    out["mean_duration_gen"], out["mean_duration_target"] = g[0], t[0]
    out["mean_duration_ratio"] = g[0] / t[0] if t[0] == t[0] and t[0] > 0.0 else nan
    out["longest_gen"], out["longest_target"], out["longest_bias"] = g[1], t[1], g[1] - t[1]
    out["onset_rate_gen"], out["onset_rate_target"] = g[2], t[2]
    out["time_fraction_gen"], out["time_fraction_target"] = g[3], t[3]
    return {k: float(out[k]) for k in LOG_METRICS}


class EventSpellAggregator(EventAccumulator):
    """Per variable, event and trajectory -- a member of a sample, or a sample's target -- at every grid point: the longest
    spell, the number of spells and the times in the event; per latitude the histogram of spell durations of gen and of the
    target; and area-weighted summaries of mean duration, longest spell, onset rate and time fraction.

    Definition (csrc/spells.h, csrc/events.h).  A value x is in an event when x > c (above) or x < c (below), strictly; a NaN
    x never is, for the target too, so it ends a spell.  The counted times of a trajectory are those of the run in order; the
    first time of a run (`i_time_start == 0`) is the initial condition and is not counted.  A spell is a maximal run of
    consecutive counted times in the event.  A grid point whose threshold is NaN (a NaN in a threshold map) is NOT COUNTED
    for that event: it adds nothing to the histogram or the summaries and its per-point outputs are NaN -- the way to mask
    land for an ocean-only field; there is no other mask.

    `record_batch(loss, target_data, gen_data, target_data_norm, gen_data_norm, i_time_start)` is what `run_inference` calls
    once per window: targets `(samples, time, lat, lon)`, gen `(members, samples, time, lat, lon)` (a 4-D gen is one member).
    Only the variables with events are read.  One `sdy_event_spell_accumulate` launch per run of variables with equal extents
    and equal event count reads the window in place -- the member-stacked transposed view included -- and advances the state
    of every (event, trajectory, grid point): four 32-bit words `run` (the spell open after the last counted time), `longest`,
    `spells` and `hits`, 16 bytes (one event on 63 variables of 25 members at 180 x 360 needs 1.7 GB).  A spell enters the
    duration histogram at the counted time at which it ends; spells still open are added at read-out from `run`, which
    changes no state: state and histogram have the same bits however a run is cut into windows.  The first window that is
    accepted may start anywhere and fixes variables, grids, member count and sample count; every later one must repeat them
    and start where the one before ended (`ValueError` otherwise).  The state is one more float64-typed statistic (two slots
    per element) allocated on the first window, after comparing its bytes with `max_bytes` (default: a quarter of the
    device's memory).  A refused window changes nothing.  The denormalised data are read.

    `area_weights` is `(lat, lon)`, constant along a row (the weight of a latitude is its row's mean).

    `get_data()` returns float64 device tensors per `<event>/<variable>`: `gen_longest`, `gen_spells`, `gen_hits` `(members,
    samples, lat, lon)` and `target_longest`, `target_spells`, `target_hits` `(samples, lat, lon)`, NaN at the points that are
    not counted (this rank's); `durations_gen` and `durations_target` `(lat, 16)`, closed plus open spells, with
    `duration_edges` (bin(d) = the number of edges 1, 2, 4, .., 16384 below d); and `rows` `(2, lat, 4)`: per side (gen,
    target) and latitude the integer sums over the counted points of hits, spells, longest and trajectory-points.  Read-out is
    torch integer arithmetic on an int32 view of the state, summed in int64: exact in any order.  `rows` and the durations are
    added over ranks (`dist.reduce_sum`) before anything is divided.

    `get_logs(label)` returns Python floats `<metric>/<event>/<variable>` for the metrics of `LOG_METRICS` (`logs_from_rows`).
    `ValueError("No data recorded.")` before any collective when nothing was counted.  Ranks hold whole initial conditions;
    ragged shares (flat rows with `sample_weights`) are refused."""

    def __init__(self, events: Events, area_weights: torch.Tensor, n_timesteps: int, dist=None, metadata=None,
                 max_bytes: Optional[int] = None):
        super().__init__(events, area_weights, n_timesteps, pool_times=True, dist=dist, metadata=metadata, max_bytes=max_bytes)
        self._n_times = 0                          # counted times so far
        self._next_start: Optional[int] = None     # where the next window has to start (None before the first window)

    def _statistics(self) -> Dict[str, float]:
        # "state": the four 32-bit words of an element in two 8-byte slots of a float64-typed buffer (all bits zero: 0.0)
        return {"state": 0.0, "durations": 0.0}

    def _elements(self, stat: str, job: tuple) -> int:
        M, n1, H, W, E = job
        return 2 * E * (M + 1) * n1 * H * W if stat == "state" else E * 2 * H * SDY_SPELL_BINS

    def _size_words(self, names, jobs) -> str:
        return (f"the spell state (16 bytes per event, trajectory and grid point) of {sum(j[4] for j in jobs)} events of "
                f"{len(names)} variables, {jobs[0][0]} members x {jobs[0][1]} samples")

    @property
    def n_times(self) -> int:
        """Counted times so far."""
        return self._n_times

    @torch.no_grad()
    def record_batch(self, loss, target_data, gen_data, target_data_norm=None, gen_data_norm=None, i_time_start: int = 0,
                     sample_weights: Optional[Sequence[float]] = None):
        del loss, target_data_norm, gen_data_norm
        start = int(i_time_start)
        if self._next_start is not None and start != self._next_start:
            raise ValueError(f"EventSpellAggregator: a window that starts at time {start}, where the one before ended at "
                             f"{self._next_start}: a spell needs every window of a run, in order")
        lay, t0, device = self._begin(target_data, gen_data, start, sample_weights)
        T = lay[0].T
        # (after `_begin`, which changes something at the first window only, and that one cannot be too long: T <= 2^30)
        if self._n_times + T - t0 > MAX_TIMES:
            raise ValueError(f"EventSpellAggregator: more than {MAX_TIMES} counted times (the state words are 32 bits)")
        with torch.cuda.device(device):
            for first, last in runs(lay, lambda l: (l.extents, l.n_events)):
                a = SdyEventSpellArgs()
                self._fill(a, lay, first, last, t0, start)
                a.state, a.durations = self._at("state", first), self._at("durations", first)
                check(lib.sdy_event_spell_accumulate(C.byref(a), current_stream()), "sdy_event_spell_accumulate")
        self._n_times += T - t0
        self._next_start = start + T

    def _recorded(self) -> None:
        # (raised BEFORE any collective: every rank of a job must have counted at least one time)
        if self._names is None or self._n_times < 1:
            raise ValueError("No data recorded.")

    def _state(self, i: int) -> torch.Tensor:
        """-> the (E, 4, rows, lat, lon) int32 view of variable i's state; rows: the generated trajectories, then the targets."""
        M, n1, H, W, E = self._grids[i]
        return self._view("state", i, 2 * E * (M + 1) * n1 * H * W).view(torch.int32).view(E, 4, (M + 1) * n1, H, W)

    def _counted(self, name: str, e: int, H: int, W: int, device) -> torch.Tensor:
        """-> (lat, lon) bool: the points that are counted for event e of a variable (its threshold is not NaN)."""
        event = self._events[name][e]
        if event.map is None:
            return torch.ones(H, W, dtype=torch.bool, device=device)
        return ~torch.isnan(event.map).to(device)

    def _per_event(self, i: int, e: int):
        """Variable i, event e -> (state (4, rows, lat, lon) int32, counted (lat, lon) bool, local (2, lat, 4 + 16) float64:
        per side and latitude the four `rows` sums and the durations of the spells that are still open)."""
        M, n1, H, W, E = self._grids[i]
        st = self._state(i)[e]
        counted = self._counted(self._names[i], e, H, W, st.device)
        local = torch.zeros(2, H, 4 + SDY_SPELL_BINS, dtype=torch.float64, device=st.device)
        keep = counted.to(torch.int64)
        for side, rows in enumerate((slice(0, M * n1), slice(M * n1, (M + 1) * n1))):
            run, longest, spells, hits = (st[k, rows].to(torch.int64) * keep for k in range(4))
            for k, x in enumerate((hits, spells, longest)):
                local[side, :, k] = x.sum(dim=(0, 2)).to(torch.float64)
            local[side, :, 3] = (keep.sum(dim=1) * run.shape[0]).to(torch.float64)
            # a spell that is still open: one more of duration `run` at its latitude
            at = torch.arange(H, device=st.device)[None, :, None] * SDY_SPELL_BINS + duration_bin(run.clamp(min=1))
            opened = torch.zeros(H * SDY_SPELL_BINS, dtype=torch.int64, device=st.device)
            opened.scatter_add_(0, at.reshape(-1), (run > 0).to(torch.int64).reshape(-1))
            local[side, :, 4:] = opened.view(H, SDY_SPELL_BINS).to(torch.float64)
        return st, counted, local

    def _durations(self, i: int) -> torch.Tensor:
        H, E = self._grids[i][2], self._grids[i][4]
        return self._view("durations", i, E * 2 * H * SDY_SPELL_BINS).view(E, 2, H, SDY_SPELL_BINS)

    def _sums(self):
        """-> per variable the (E, 2, lat, 4 + 16) float64 sums of `rows` and of closed plus open durations, added over ranks in
        ONE reduce."""
        parts = []
        for i in range(len(self._names)):
            E = self._grids[i][4]
            local = torch.stack([self._per_event(i, e)[2] for e in range(E)])
            local[..., 4:] += self._durations(i)
            parts.append(local.reshape(-1))
        packed = self._dist.reduce_sum(torch.cat(parts))
        out, at = [], 0
        for i in range(len(self._names)):
            H, E = self._grids[i][2], self._grids[i][4]
            n = E * 2 * H * (4 + SDY_SPELL_BINS)
            out.append(packed[at:at + n].view(E, 2, H, 4 + SDY_SPELL_BINS))
            at += n
        return out

    @torch.no_grad()
    def get_data(self) -> Dict[str, torch.Tensor]:
        self._recorded()
        sums = self._sums()
        data: Dict[str, torch.Tensor] = {}
        for i, name in enumerate(self._names):
            M, n1, H, W, E = self._grids[i]
            for e, event in enumerate(self._events[name]):
                tail = f"{event.name}/{name}"
                st, counted, _ = self._per_event(i, e)
                nan = torch.full((), float("nan"), dtype=torch.float64, device=st.device)
                for k, word in ((1, "longest"), (2, "spells"), (3, "hits")):
                    x = torch.where(counted, st[k].to(torch.float64), nan)
                    data[f"gen_{word}/{tail}"] = x[:M * n1].view(M, n1, H, W)
                    data[f"target_{word}/{tail}"] = x[M * n1:]
                data[f"durations_gen/{tail}"] = sums[i][e, 0, :, 4:]
                data[f"durations_target/{tail}"] = sums[i][e, 1, :, 4:]
                data[f"duration_edges/{tail}"] = duration_edges().to(st.device, torch.float64)
                data[f"rows/{tail}"] = sums[i][e, :, :, :4]
        return data

    @torch.no_grad()
    def get_logs(self, label: str) -> Dict[str, float]:
        self._recorded()
        sums = self._sums()
        logs: Dict[str, float] = {}
        for i, name in enumerate(self._names):
            w = self._lat_weights(i, sums[i].device).cpu()
            rows = sums[i][..., :4].cpu()
            for e, event in enumerate(self._events[name]):
                one = logs_from_rows(rows[e], w, self._n_times)
                logs.update({f"{metric}/{event.name}/{name}": one[metric] for metric in LOG_METRICS})
        return {f"{label}/{k}": v for k, v in logs.items()} if len(label) != 0 else logs


@torch.no_grad()
def spell_statistics(x: torch.Tensor, threshold, below: bool = False) -> Dict[str, torch.Tensor]:
    """One `(time, lat, lon)` device tensor against one threshold (a number or a `(lat, lon)` map; x < threshold when `below`,
    else x > threshold; every time is counted) -> {"longest", "spells", "hits": (lat, lon) float64}, NaN where the threshold
    is NaN.  `longest` of pr < 1 mm/day is the consecutive-dry-days index."""
    if x.dim() != 3:
        raise ValueError(f"expected (time, lat, lon), got {tuple(x.shape)}")
    if not x.is_cuda:
        raise RuntimeError("sdy_amd aggregators run on the GPU only (no CPU fallback)")
    T, H, W = x.shape
    if T > MAX_TIMES:
        raise ValueError(f"more than {MAX_TIMES} times")
    x = x.to(torch.float32).contiguous()
    thr = torch.as_tensor(threshold).detach().to(torch.float32)
    if thr.dim() not in (0, 2) or (thr.dim() == 2 and tuple(thr.shape) != (H, W)):
        raise ValueError(f"a threshold is a number or a {(H, W)} map, got shape {tuple(thr.shape)}")
    thr = thr.to(x.device).contiguous()
    state = torch.zeros(4, 2, H, W, dtype=torch.int32, device=x.device)       # (word, trajectory: x and x again, lat, lon)
    durations = torch.zeros(2, H, SDY_SPELL_BINS, dtype=torch.float64, device=x.device)
    scalars = torch.full((1,), float("nan"), dtype=torch.float32, device=x.device)
    a = SdyEventSpellArgs()
    a.nvars, a.gen[0], a.target[0] = 1, ptr(x), ptr(x)
    a.n0, a.n1, a.T, a.gs0, a.gs1, a.ts1 = 1, 1, T, 0, 0, 0
    a.H, a.W, a.t0 = H, W, 0
    a.thr.n_events, a.thr.below[0] = 1, int(bool(below))
    if thr.dim() == 2:
        a.thr.is_map[0], a.thr.map_first[0], a.thr.n_maps, a.thr.maps = 1, 0, 1, ptr(thr)
    else:
        scalars.fill_(float(thr))
    a.thr.scalars, a.state, a.durations = ptr(scalars), ptr(state), ptr(durations)
    with torch.cuda.device(x.device):
        check(lib.sdy_event_spell_accumulate(C.byref(a), current_stream()), "sdy_event_spell_accumulate")
    out = state[:, 0].to(torch.float64)
    if thr.dim() == 2:
        out = torch.where(torch.isnan(thr), torch.full_like(out, math.nan), out)
    return {"longest": out[1], "spells": out[2], "hits": out[3]}
