"""Time means and extremes per calendar bin of an ensemble rollout, on the device (no counterpart in the reference): the
seasonal cycle (monthly or DJF / MAM / JJA / SON climatologies per member), annual and seasonal means per year, block extremes
(the annual maximum of a daily field, the warmest and coldest value of each season) and the diurnal cycle.

`TimeBins` is the host side: one label per global time index of a run, from a calendar in plain integer arithmetic or from
the caller.  `BinnedTimeMeanAggregator` knows that the times of a window belong to different bins: it groups them by bin and
hands the groups to `sdy_binned_time_accumulate` (include/sdy_amd.h), whose float64 sums and fp32 extremes stay on the device.
`binned_time_mean` is the same for one tensor.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import (SDY_BIN_MAX_TIMES, SDY_MEMBER_STATS_MAX_MEMBERS, SdyBinnedSumArgs, SdyMemberStatsArgs, check,
                   current_stream, lib, ptr)
from .windows import FieldAccumulator, WindowLayout, fill_window, runs, strided_layout, whole_ics_message, window_layouts

KINDS = ("month", "season", "year", "year_month", "year_season", "hour_of_day")
CALENDARS = ("noleap", "360_day", "proleptic_gregorian")
MONTH_NAMES = ("Jan", "Feb", "Mar", "Apr", "May", "Jun", "Jul", "Aug", "Sep", "Oct", "Nov", "Dec")
SEASON_NAMES = ("DJF", "MAM", "JJA", "SON")
_CUM_NOLEAP = (0, 31, 59, 90, 120, 151, 181, 212, 243, 273, 304, 334, 365)


# -- calendars: a date <-> the number of its day, in integers (the Gregorian pair is the well-known era arithmetic: 400 years
# are 146097 days; the count starts at 1970-01-01, which no caller relies on)
def _to_days(calendar: str, y: int, m: int, d: int) -> int:
    if calendar == "360_day":
        return y * 360 + (m - 1) * 30 + (d - 1)
    if calendar == "noleap":
        return y * 365 + _CUM_NOLEAP[m - 1] + (d - 1)
    y -= m <= 2
    era = y // 400
    yoe = y - era * 400
    doy = (153 * (m - 3 if m > 2 else m + 9) + 2) // 5 + d - 1
    return era * 146097 + yoe * 365 + yoe // 4 - yoe // 100 + doy - 719468


def _from_days(calendar: str, n: int) -> Tuple[int, int, int]:
    if calendar == "360_day":
        y, r = divmod(n, 360)
        return y, r // 30 + 1, r % 30 + 1
    if calendar == "noleap":
        y, r = divmod(n, 365)
        m = next(i for i in range(1, 13) if r < _CUM_NOLEAP[i])
        return y, m, r - _CUM_NOLEAP[m - 1] + 1
    z = n + 719468
    era = z // 146097
    doe = z - era * 146097
    yoe = (doe - doe // 1460 + doe // 36524 - doe // 146096) // 365
    doy = doe - (365 * yoe + yoe // 4 - yoe // 100)
    mp = (5 * doy + 2) // 153
    m = mp + 3 if mp < 10 else mp - 9
    return yoe + era * 400 + (m <= 2), m, doy - (153 * mp + 2) // 5 + 1


def _days_in_month(calendar: str, y: int, m: int) -> int:
    ny, nm = (y + 1, 1) if m == 12 else (y, m + 1)
    return _to_days(calendar, ny, nm, 1) - _to_days(calendar, y, m, 1)


def _season(m: int) -> int:
    return (m % 12) // 3          # Dec, Jan, Feb -> 0


def _key(kind: str, y: int, m: int, h: int) -> int:
    """The number of the calendar period a time falls in; consecutive periods have consecutive numbers."""
    if kind == "month":
        return m - 1
    if kind == "season":
        return _season(m)
    if kind == "year":
        return y
    if kind == "year_month":
        return y * 12 + (m - 1)
    if kind == "year_season":
        return (y + (m == 12)) * 4 + _season(m)      # December counts with the DJF of the following January
    return h


def _period(kind: str, calendar: str, key: int, day: int) -> Tuple[int, int]:
    """[first day, day after the last) of what a complete bin covers around a time in period `key` on day `day`: the period
    itself for the per-year kinds, the calendar year for "month" and "season", the day for "hour_of_day"."""
    if kind in ("month", "season", "year"):
        y = key if kind == "year" else _from_days(calendar, day)[0]
        return _to_days(calendar, y, 1, 1), _to_days(calendar, y + 1, 1, 1)
    if kind == "year_month":
        y, m0 = divmod(key, 12)
        ny, nm = (y + 1, 1) if m0 == 11 else (y, m0 + 2)
        return _to_days(calendar, y, m0 + 1, 1), _to_days(calendar, ny, nm, 1)
    if kind == "year_season":
        sy, s = divmod(key, 4)
        y, m = (sy - 1, 12) if s == 0 else (sy, 3 * s)
        ey, em = (y + 1, m - 9) if m + 3 > 12 else (y, m + 3)
        return _to_days(calendar, y, m, 1), _to_days(calendar, ey, em, 1)
    return day, day + 1


class TimeBins:
    """The bin of every time of a run.

    `labels`: int32, one per global time index of the run (index 0 is the initial condition), each in `0 .. n_bins - 1` or
    `-1` for "not counted".  `names`: one string per bin.  `expected_counts`: per bin the number of times a run on the same
    time grid would count if it covered every calendar period it touches completely (`None` for labels that come from the
    caller): a first or last season-year that a run covers in part is kept and named like the others, and shows as a count
    below the expected one.
    """

    def __init__(self, labels: np.ndarray, names: Sequence[str], expected_counts: Optional[np.ndarray] = None):
        self.labels = labels
        self.names = list(names)
        self.n_bins = len(self.names)
        self.expected_counts = expected_counts

    @classmethod
    def from_labels(cls, labels, names: Optional[Sequence[str]] = None) -> "TimeBins":
        arr = np.asarray(labels)
        if arr.ndim != 1 or arr.size == 0:
            raise ValueError(f"labels are one integer per time of the run, got an array of shape {arr.shape}")
        if arr.dtype.kind not in "iu":
            raise ValueError(f"labels are integers, got {arr.dtype}")
        if int(arr.min()) < -1:
            raise ValueError(f"a label is a bin 0 .. n_bins - 1 or -1 (not counted), got {int(arr.min())}")
        top = int(arr.max())
        if names is None:
            if top < 0:
                raise ValueError("no time is counted: every label is -1")
            names = [str(b) for b in range(top + 1)]
        names = [str(n) for n in names]
        if len(names) < 1 or top >= len(names):
            raise ValueError(f"label {top} with {len(names)} bin names")
        if len(set(names)) != len(names) or any("/" in n or n == "" for n in names):
            raise ValueError("bin names are distinct, not empty and hold no '/': they are parts of log keys")
        return cls(arr.astype(np.int32), names)

    @classmethod
    def calendar(cls, kind: str, start: Sequence[int], n_timesteps: int, step_hours: int = 6,
                 calendar: str = "noleap") -> "TimeBins":
        """The bins of `n_timesteps` times `step_hours` apart from `start = (year, month, day[, hour])`."""
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
        if calendar not in CALENDARS:
            raise ValueError(f"calendar must be one of {CALENDARS}, got {calendar!r}")
        if len(start) not in (3, 4) or any(int(s) != s for s in start):
            raise ValueError(f"start is (year, month, day[, hour]) in integers, got {start!r}")
        y, m, d = (int(s) for s in start[:3])
        h = int(start[3]) if len(start) == 4 else 0
        if not 1 <= m <= 12 or not 1 <= d <= _days_in_month(calendar, y, m) or not 0 <= h < 24:
            raise ValueError(f"{start!r} is no date of the {calendar} calendar")
        n_timesteps, step_hours = int(n_timesteps), int(step_hours)
        if n_timesteps < 1 or step_hours < 1:
            raise ValueError(f"n_timesteps and step_hours must be positive, got {n_timesteps} and {step_hours}")
        hour0 = _to_days(calendar, y, m, d) * 24 + h

        def keys(first: int, last: int) -> List[Tuple[int, int]]:
            """(period, day) of the time indices first .. last - 1."""
            out = []
            for i in range(first, last):
                day, hh = divmod(hour0 + i * step_hours, 24)
                yy, mm, _ = _from_days(calendar, day)
                out.append((_key(kind, yy, mm, hh), day))
            return out

        run = keys(0, n_timesteps)
        present = sorted({k for k, _ in run})
        if kind in ("year", "year_month", "year_season"):
            present = list(range(present[0], present[-1] + 1))     # (a step of months can pass over a period: an empty bin)
        elif kind in ("month", "season"):
            present = list(range(12 if kind == "month" else 4))    # always the twelve months, the four seasons
        index = {k: b for b, k in enumerate(present)}
        labels = np.array([index[k] for k, _ in run], dtype=np.int32)
        if kind == "month":
            names = [MONTH_NAMES[k] for k in present]
        elif kind == "season":
            names = [SEASON_NAMES[k] for k in present]
        elif kind == "year":
            names = [f"{k:04d}" for k in present]
        elif kind == "year_month":
            names = [f"{k // 12:04d}-{k % 12 + 1:02d}" for k in present]
        elif kind == "year_season":
            names = [f"{k // 4:04d}-{SEASON_NAMES[k % 4]}" for k in present]
        else:
            names = [f"{k:02d}h" for k in present]
        # the same time grid, extended to the beginning of what the first time's complete bin covers and to the end of the last's
        begin = _period(kind, calendar, *run[0])[0] * 24
        end = _period(kind, calendar, *run[-1])[1] * 24
        back = (hour0 - begin) // step_hours
        ahead = (end - 1 - (hour0 + (n_timesteps - 1) * step_hours)) // step_hours
        expected = np.zeros(len(present), dtype=np.int64)
        for k, _ in keys(-back, n_timesteps + ahead):
            if k in index:
                expected[index[k]] += 1
        return cls(labels, names, expected)

    def restrict(self, keep) -> "TimeBins":
        """The same bins with every time outside `keep` (bin names or numbers) relabelled -1."""
        keep = list(keep)
        if len(keep) == 0:
            raise ValueError("keep selects no bin")
        numbers = []
        for k in keep:
            if isinstance(k, str):
                if k not in self.names:
                    raise ValueError(f"no bin {k!r} among {self.names}")
                numbers.append(self.names.index(k))
            else:
                if int(k) != k or not 0 <= int(k) < self.n_bins:
                    raise ValueError(f"bin {k!r} outside 0..{self.n_bins - 1}")
                numbers.append(int(k))
        labels = np.where(np.isin(self.labels, numbers), self.labels, -1).astype(np.int32)
        return TimeBins(labels, self.names, self.expected_counts)

    def label_counts(self) -> np.ndarray:
        """Per bin the number of labelled times, the initial condition (index 0) included."""
        return np.bincount(self.labels[self.labels >= 0], minlength=self.n_bins).astype(np.int64)


def group_times(labels: Sequence[int], t0: int = 0) -> List[List[Tuple[int, List[int]]]]:
    """The counted times (label >= 0) of a window from window time `t0` on, as the calls `sdy_binned_time_accumulate` takes:
    at most SDY_BIN_MAX_TIMES times each, in time order; a call's times grouped by bin, the groups in order of first
    appearance, ascending inside a group.  -> per call [(bin, [window times])]."""
    counted = [(t, int(b)) for t, b in enumerate(labels) if t >= t0 and int(b) >= 0]
    calls = []
    for at in range(0, len(counted), SDY_BIN_MAX_TIMES):
        groups: Dict[int, List[int]] = {}
        for t, b in counted[at:at + SDY_BIN_MAX_TIMES]:
            groups.setdefault(b, []).append(t)
        calls.append(list(groups.items()))
    return calls


def fill_groups(a: SdyBinnedSumArgs, groups: Sequence[Tuple[int, Sequence[int]]]) -> None:
    """One call's groups into the argument structure."""
    a.n_groups = len(groups)
    at = 0
    for g, (b, times) in enumerate(groups):
        for t in times:
            a.times[at] = t
            at += 1
        a.group_bin[g], a.group_end[g] = b, at


class BinnedTimeMeanAggregator(FieldAccumulator):
    """Per time bin one time-mean map per member (and the target's), optionally the bin's extremes, and their scores.

    `bins` is a `TimeBins`: months for the seasonal cycle, years for interannual behaviour, `hour_of_day` for the diurnal cycle.
    `record_batch(loss, target_data, gen_data, target_data_norm, gen_data_norm, i_time_start)` is what `run_inference` calls
    once per window: targets `(samples, time, lat, lon)`, gen `(members, samples, time, lat, lon)` (a 4-D gen is one member).
    The labels of the window's times are `bins.labels[i_time_start : i_time_start + T]`; the first time of a run is the initial
    condition and is never counted, nor is a time labelled -1.  Only `variables` are read (`None`: all generated variables).
    The host groups the window's counted times by bin; one `sdy_binned_time_accumulate` launch per run of same-shaped variables
    reads the window in place -- the member-stacked transposed view included -- and adds it to float64 sums per bin, variable,
    trajectory and grid point that stay on the device; `extremes=True` keeps the fp32 maximum and minimum as well.  The sum of
    one bin and element is one sequential float64 chain over its counted times in run order (`per_member=False`: the members
    of a sample go into one accumulator, in member order inside each time), so every bit is the same however the run is cut
    into windows.  A NaN makes a bin's extreme NaN from then on, for that element only.

    Everything is checked before anything changes, and a refused window changes nothing: the first window that is accepted
    fixes variables, grids, member count and sample count; times outside `len(bins.labels)` are refused; a window that starts
    before the end of the last recorded one is refused, because the chain order is the run order (gaps are allowed).

    Memory.  The accumulators are allocated on the first window, after comparing their bytes with `max_bytes` (default: a
    quarter of the device's memory).  At 25 members, 63 variables and 180 x 360 ONE bin of per-member sums is 0.85 GB, so
    twelve months are 10 GB (extremes: as much again): name the variables with `variables=`, or pool the members with
    `per_member=False` (one 25th).

    `counts()`: per bin the counted times, host integers.  `get_bin_means()`: `{"gen": {name: (n_bins, members, samples, lat,
    lon)}, "target": {name: (n_bins, samples, lat, lon)}}`, float64 on the device, a true division by a device tensor of counts;
    an empty bin is NaN; with `per_member=False` the member axis is 1 and the divisor is count x members.  `get_extremes()`: the
    same shapes in fp32 under `gen_max`, `gen_min`, `target_max`, `target_min`, NaN in an empty bin.

    `get_logs(label)` returns Python floats.  Per non-empty bin `b` and variable `rmse/<names[b]>/<var>` and
    `bias/<names[b]>/<var>` of the ensemble mean of the bin's maps, and with more than one member `rmse_member_avg/...`,
    `bias_member_avg/...` and `crps/...`: the numbers of `EnsembleTimeMeanAggregator.get_logs` for that bin's maps, from the same
    kernel (`sdy_member_map_stats`, one call per non-empty bin and run of same-shaped variables).  Across the non-empty bins,
    when there are at least two, per variable: `bin_range_gen`, `bin_range_target`, `bin_range_ratio` (the area-weighted mean
    over samples and points of max minus min over the bins, of the ensemble-mean maps and of the target's: for months the
    amplitude of the seasonal cycle), `bin_std_gen`, `bin_std_target`, `bin_std_ratio` (the population standard deviation across
    the bins: for years the interannual spread) and `centred_rmse` (the area-weighted RMS over bins, samples and points of
    (gen_b - mean over bins of gen) - (target_b - mean over bins of target): the error of the cycle with the mean bias
    removed), formed in float64 torch on the device.

    Ranks hold whole initial conditions: the raw weighted sums are added over ranks (`dist.reduce_sum`) before any root or
    division, as `EnsembleTimeMeanAggregator` does; a ragged share (flat rows with `sample_weights`) is refused."""

    accepts_sample_weights = True      # (to see, and refuse, a ragged share)

    _job_words = "member count, sample count"

    def __init__(self, bins: TimeBins, area_weights: torch.Tensor, variables: Optional[Sequence[str]] = None,
                 per_member: bool = True, extremes: bool = False, target: str = "denorm", dist=None, metadata=None,
                 max_bytes: Optional[int] = None):
        if not isinstance(bins, TimeBins):
            raise ValueError(f"bins must be a sdy_amd.TimeBins, got {type(bins).__name__}")
        if target not in ("norm", "denorm"):
            raise ValueError(f"target must be 'norm' or 'denorm', got {target!r}")
        super().__init__(dist=dist, metadata=metadata, max_bytes=max_bytes)      # (no lead-time axis)
        self._bins = bins
        self._area_weights = area_weights
        self._variables = None if variables is None else list(variables)
        if self._variables is not None and len(self._variables) == 0:
            raise ValueError("variables=[] selects nothing (None: all generated variables)")
        self._per_member = bool(per_member)
        self._extremes = bool(extremes)
        self._target = target
        self._bin_counts = [0] * bins.n_bins
        self._next_start: Optional[int] = None       # the end of the last recorded window (None before the first)
        self._ext: Dict[str, torch.Tensor] = {}      # fp32 extremes, laid out as the sums
        self._acc_runs: List[Tuple[int, int]] = []   # the runs of same-shaped variables the accumulators are laid out in

    # -- the layout: a run of same-shaped variables is ONE block (n_bins, variables of the run, rows, lat, lon), so that a bin of
    # it is the contiguous (nvars, members, samples, lat, lon) that sdy_member_map_stats takes.  FieldAccumulator's per-variable
    # offsets give a run's block: the offset of its first variable.
    def _statistics(self) -> Dict[str, float]:
        return {"gen_sum": 0.0, "target_sum": 0.0}

    @staticmethod
    def _job(l: WindowLayout) -> tuple:
        return (l.n0, l.n1, l.H, l.W)

    def _rows(self, stat: str, job: tuple) -> int:
        M, n1 = job[:2]
        return (M if self._per_member else 1) * n1 if stat.startswith("gen") else n1

    def _elements(self, stat: str, job: tuple) -> int:
        return self._bins.n_bins * self._rows(stat, job) * job[2] * job[3]

    def _size_words(self, names, jobs) -> str:
        M = jobs[0][0] if self._per_member else 1
        return (f"{self._bins.n_bins} bins x {len(names)} variables x {M} member maps (and the target's)"
                + (", sums and extremes" if self._extremes else ""))

    def _check_memory(self, names: List[str], lay: List[WindowLayout]) -> None:
        """The first window: sums and extremes together against the limit, before anything is allocated."""
        jobs = [self._job(l) for l in lay]
        elements = sum(self._elements(s, j) for s in ("gen_sum", "target_sum") for j in jobs)
        need = elements * (8 + (8 if self._extremes else 0))         # a float64 sum; an fp32 maximum and an fp32 minimum
        limit = self._max_bytes
        if limit is None and all(l.gen.is_cuda for l in lay):
            limit = torch.cuda.get_device_properties(lay[0].gen.device).total_memory // 4
        if limit is not None and need > limit:
            raise ValueError(f"{type(self).__name__}: {self._size_words(names, jobs)} need {need} bytes of accumulators, more "
                             f"than max_bytes = {limit} (variables= names fewer variables, per_member=False pools the members)")

    @torch.no_grad()
    def record_batch(self, loss, target_data, gen_data, target_data_norm=None, gen_data_norm=None, i_time_start: int = 0,
                     sample_weights: Optional[Sequence[float]] = None):
        del loss
        if self._target == "norm":
            target_data, gen_data = target_data_norm, gen_data_norm
        start = int(i_time_start)
        ragged = sample_weights is not None or any(
            g.dim() == 4 and k in target_data and target_data[k].dim() == 4 and g.shape[0] != target_data[k].shape[0]
            for k, g in gen_data.items())
        if ragged:
            raise ValueError(whole_ics_message(type(self).__name__))
        names = list(gen_data) if self._variables is None else self._variables
        missing = [k for k in names if k not in gen_data]
        if missing:
            raise ValueError(f"no generated variable {missing[0]!r} in the window, but its bin means were asked for")
        lay = window_layouts(target_data, {k: gen_data[k] for k in names})
        T = lay[0].T
        if start < 0 or start + T > len(self._bins.labels):
            raise ValueError(f"times {start}..{start + T - 1} outside the {len(self._bins.labels)} times the bins label")
        if self._next_start is not None and start < self._next_start:
            raise ValueError(f"{type(self).__name__}: a window that starts at time {start}, before the end of the last recorded "
                             f"one ({self._next_start}): a bin's sum is one chain in run order")
        if T > 65536:
            raise ValueError(f"a window of {T} times: the kernel takes window times as 16-bit numbers")
        if self._names is None:
            self._check_memory(names, lay)
        device = self._prepare(names, lay)
        if not self._acc_runs:
            self._acc_runs = list(runs(self._grids, lambda g: g))
            if self._extremes:
                for side in ("gen", "target"):
                    n = self._acc[f"{side}_sum"].numel()
                    self._ext[f"{side}_max"] = torch.full((n,), -math.inf, dtype=torch.float32, device=device)
                    self._ext[f"{side}_min"] = torch.full((n,), math.inf, dtype=torch.float32, device=device)
        t0 = 1 if start == 0 else 0                    # the very first time of a run is the initial condition
        calls = group_times(self._bins.labels[start:start + T], t0)
        with torch.cuda.device(device):
            for af, al in self._acc_runs:
                for first, last in runs(lay[af:al], lambda l: l.extents):
                    for groups in calls:
                        self._launch_call(lay, af, al, af + first, af + last, groups)
        for groups in calls:
            for b, times in groups:
                self._bin_counts[b] += len(times)
        self._next_start = start + T

    def _block(self, stat: str, af: int, v: int = 0) -> int:
        """Element offset of variable af + v of bin 0 in the block of the accumulator run that starts at variable af."""
        return self._offsets[stat][af] + v * self._rows(stat, self._grids[af]) * self._grids[af][2] * self._grids[af][3]

    def _launch_call(self, lay, af: int, al: int, first: int, last: int, groups) -> None:
        a = SdyBinnedSumArgs()
        fill_window(a.win, lay, first, last)
        fill_groups(a, groups)
        a.HW = lay[first].H * lay[first].W
        a.n_bins, a.bin_vars, a.pool_members = self._bins.n_bins, al - af, int(not self._per_member)
        for side in ("gen", "target"):
            at = self._block(f"{side}_sum", af, first - af)
            setattr(a, f"{side}_sum", self._acc[f"{side}_sum"].data_ptr() + 8 * at)
            if self._extremes:
                setattr(a, f"{side}_max", self._ext[f"{side}_max"].data_ptr() + 4 * at)
                setattr(a, f"{side}_min", self._ext[f"{side}_min"].data_ptr() + 4 * at)
        check(lib.sdy_binned_time_accumulate(C.byref(a), current_stream()), "sdy_binned_time_accumulate")

    def _check_recorded(self) -> None:
        # (raised BEFORE any collective: every rank of a job must have counted at least one time)
        if self._names is None or not any(self._bin_counts):
            raise ValueError("No data recorded.")

    def counts(self) -> List[int]:
        """Per bin the number of counted times so far (host integers); `bins.expected_counts` has what a complete bin holds."""
        return list(self._bin_counts)

    def _bin_views(self, buf: torch.Tensor, stat: str, i: int) -> torch.Tensor:
        """Variable i of a buffer laid out as `stat`'s: (n_bins, rows, lat, lon), a view."""
        af, al = next(r for r in self._acc_runs if r[0] <= i < r[1])
        rows, (H, W) = self._rows(stat, self._grids[i]), self._grids[i][2:]
        at = self._offsets[stat][af]
        block = buf[at:at + self._bins.n_bins * (al - af) * rows * H * W]
        return block.view(self._bins.n_bins, al - af, rows, H, W)[:, i - af]

    @torch.no_grad()
    def get_bin_means(self) -> Dict[str, Dict[str, torch.Tensor]]:
        self._check_recorded()
        device = self._acc["gen_sum"].device
        n = torch.tensor(self._bin_counts, dtype=torch.float64, device=device)
        out: Dict[str, Dict[str, torch.Tensor]] = {"gen": {}, "target": {}}
        for i, name in enumerate(self._names):
            M, n1, H, W = self._grids[i]
            pooled = 1 if self._per_member else M
            gen = self._bin_views(self._acc["gen_sum"], "gen_sum", i).view(-1, M // pooled, n1, H, W)
            out["gen"][name] = gen / (n * pooled).view(-1, 1, 1, 1, 1)          # 0 / 0: an empty bin is NaN
            out["target"][name] = self._bin_views(self._acc["target_sum"], "target_sum", i) / n.view(-1, 1, 1, 1)
        return out

    @torch.no_grad()
    def get_extremes(self) -> Dict[str, Dict[str, torch.Tensor]]:
        self._check_recorded()
        if not self._extremes:
            raise ValueError("the extremes were not kept (extremes=True)")
        device = self._acc["gen_sum"].device
        empty = torch.tensor([c == 0 for c in self._bin_counts], device=device)
        nan = torch.full((), math.nan, dtype=torch.float32, device=device)
        out: Dict[str, Dict[str, torch.Tensor]] = {}
        for side in ("gen", "target"):
            for which in ("max", "min"):
                out[f"{side}_{which}"] = {}
                for i, name in enumerate(self._names):
                    M, n1, H, W = self._grids[i]
                    x = self._bin_views(self._ext[f"{side}_{which}"], f"{side}_sum", i)
                    if side == "gen":
                        x = x.view(-1, M if self._per_member else 1, n1, H, W)
                    out[f"{side}_{which}"][name] = torch.where(empty.view(-1, *([1] * (x.dim() - 1))), nan, x)
        return out

    @torch.no_grad()
    def weighted_sums(self) -> Dict[int, Dict[str, torch.Tensor]]:
        """Per non-empty bin and variable the 2 M + 4 raw weighted sums of `sdy_member_map_stats` (this rank's) of the bin's
        maps, float64 on the device; M is 1 with `per_member=False`."""
        self._check_recorded()
        device = self._acc["gen_sum"].device
        out: Dict[int, Dict[str, torch.Tensor]] = {}
        with torch.cuda.device(device):
            for af, al in self._acc_runs:
                M, n1, H, W = self._grids[af]
                pooled = 1 if self._per_member else M
                M //= pooled
                if M > SDY_MEMBER_STATS_MAX_MEMBERS:
                    raise ValueError(f"at most {SDY_MEMBER_STATS_MAX_MEMBERS} members, got {M}")
                if tuple(self._area_weights.shape) != (H, W):
                    raise ValueError(f"area weights {tuple(self._area_weights.shape)} against a {(H, W)} grid")
                w = self._area_weights.to(device, torch.float32).contiguous()
                nvars = al - af
                ws_bytes = lib.sdy_member_stats_workspace_bytes(nvars, M, n1, H * W)
                ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=device)
                for b, count in enumerate(self._bin_counts):
                    if count == 0:
                        continue
                    res = torch.empty(nvars, 2 * M + 4, dtype=torch.float64, device=device)
                    a = SdyMemberStatsArgs()
                    a.nvars, a.M, a.n1, a.HW = nvars, M, n1, H * W
                    a.gen_sum = self._acc["gen_sum"].data_ptr() + 8 * (self._offsets["gen_sum"][af] + b * nvars * M * n1 * H * W)
                    a.target_sum = (self._acc["target_sum"].data_ptr()
                                    + 8 * (self._offsets["target_sum"][af] + b * nvars * n1 * H * W))
                    if pooled > 1:
                        # the kernel divides both sums by ONE n_times, and the pooled sum holds count x members values: the
                        # target's sum times the members (a copy of one bin) has the same divisor
                        at = self._offsets["target_sum"][af] + b * nvars * n1 * H * W
                        scaled = self._acc["target_sum"][at:at + nvars * n1 * H * W] * float(pooled)
                        a.target_sum = ptr(scaled)
                    a.weights, a.n_times, a.out = ptr(w), float(count * pooled), ptr(res)
                    a.ws, a.ws_bytes = ptr(ws), ws_bytes
                    check(lib.sdy_member_map_stats(C.byref(a), current_stream()), "sdy_member_map_stats")
                    for j in range(af, al):
                        out.setdefault(b, {})[self._names[j]] = res[j - af]
        return out

    @torch.no_grad()
    def _across_bins(self) -> Dict[str, torch.Tensor]:
        """Per variable the five raw weighted sums across the non-empty bins (this rank's): of the range and of the population
        standard deviation over the bins of the ensemble-mean maps and of the target's, and of the squared centred error."""
        device = self._acc["gen_sum"].device
        full = torch.tensor([b for b, c in enumerate(self._bin_counts) if c > 0], device=device)
        w = self._area_weights.to(device, torch.float32).double()
        means = self.get_bin_means()
        out = {}
        for name in self._names:
            g = means["gen"][name].index_select(0, full).mean(dim=1)       # the ensemble mean: (bins, samples, lat, lon)
            t = means["target"][name].index_select(0, full)
            ga, ta = g - g.mean(dim=0), t - t.mean(dim=0)
            out[name] = torch.stack([
                (w * (g.amax(dim=0) - g.amin(dim=0))).sum(), (w * (t.amax(dim=0) - t.amin(dim=0))).sum(),
                (w * (ga * ga).mean(dim=0).sqrt()).sum(), (w * (ta * ta).mean(dim=0).sqrt()).sum(),
                (w * ((ga - ta) * (ga - ta)).mean(dim=0)).sum()])
        return out

    @torch.no_grad()
    def get_logs(self, label: str) -> Dict[str, float]:
        sums = self.weighted_sums()
        device = self._acc["gen_sum"].device
        wsum = self._area_weights.to(device, torch.float32).double().sum()
        full = sorted(sums)
        across = self._across_bins() if len(full) >= 2 else None
        # ranks hold whole initial conditions: every sum and the sample count x sum(w) of its variable are added over ranks in
        # ONE reduce, before any root or division, and come to the host in one copy
        parts = []
        for i, name in enumerate(self._names):
            parts += [(self._grids[i][1] * wsum).reshape(1)] + [sums[b][name] for b in full]
            if across is not None:
                parts.append(across[name])
        packed = self._dist.reduce_sum(torch.cat(parts)).cpu()
        logs: Dict[str, float] = {}
        at = 0
        for i, name in enumerate(self._names):
            M = self._grids[i][0] if self._per_member else 1
            norm = packed[at]
            at += 1
            for b in full:
                s = packed[at:at + 2 * M + 4] / norm
                at += 2 * M + 4
                key = f"{self._bins.names[b]}/{name}"
                if M > 1:
                    logs[f"rmse_member_avg/{key}"] = float(s[:M].sqrt().mean())
                    logs[f"bias_member_avg/{key}"] = float(s[M:2 * M].mean())
                logs[f"rmse/{key}"] = float(s[2 * M].sqrt())
                logs[f"bias/{key}"] = float(s[2 * M + 1])
                if M > 1:
                    logs[f"crps/{key}"] = float(s[2 * M + 2])
            if across is not None:
                s = packed[at:at + 5] / norm
                at += 5
                for k, what in enumerate(("bin_range", "bin_std")):
                    gen, tgt = float(s[2 * k]), float(s[2 * k + 1])
                    logs[f"{what}_gen/{name}"], logs[f"{what}_target/{name}"] = gen, tgt
                    logs[f"{what}_ratio/{name}"] = gen / tgt if tgt > 0.0 else float("nan")
                logs[f"centred_rmse/{name}"] = float(s[4].sqrt())
        return {f"{label}/{k}": v for k, v in logs.items()} if len(label) != 0 else logs


@torch.no_grad()
def binned_time_mean(x: torch.Tensor, labels, extremes: bool = False) -> Dict[str, torch.Tensor]:
    """The bin means of one `(..., time, lat, lon)` fp32 tensor on the device, every time counted under its label (a `TimeBins`
    or one integer per time, -1: not counted): `{"mean": (n_bins, ..., lat, lon) float64, "count": (n_bins,) int64}`, with
    `extremes=True` also `"max"` and `"min"` in fp32; an empty bin is NaN.  The same kernel and the same chains as the
    aggregator's: one float64 sum per bin and element over its times in ascending order."""
    bins = labels if isinstance(labels, TimeBins) else TimeBins.from_labels(labels)
    if not x.is_cuda:
        raise RuntimeError("sdy_amd aggregators run on the GPU only (no CPU fallback)")
    v, n0, n1, s0, s1, T, HW = strided_layout(x)
    if len(bins.labels) != T:
        raise ValueError(f"{len(bins.labels)} labels for {T} times")
    if min(n0, n1, T, HW) < 1:
        raise ValueError("empty tensor")
    if T > 65536:
        raise ValueError(f"{T} times: the kernel takes window times as 16-bit numbers")
    lead, (H, W) = tuple(x.shape[:-3]), x.shape[-2:]
    dev = x.device
    sums = torch.zeros(bins.n_bins * n0 * n1 * HW, dtype=torch.float64, device=dev)
    side = torch.zeros(bins.n_bins * n1 * HW, dtype=torch.float64, device=dev)      # (the window's target: member 0, unused)
    ext = []
    if extremes:
        ext = [torch.full((sums.numel(),), f, dtype=torch.float32, device=dev) for f in (-math.inf, math.inf)]
        ext += [torch.full((side.numel(),), f, dtype=torch.float32, device=dev) for f in (-math.inf, math.inf)]
    with torch.cuda.device(dev):
        for groups in group_times(bins.labels):
            a = SdyBinnedSumArgs()
            a.nvars, a.gen[0], a.target[0] = 1, ptr(v), ptr(v)
            a.n0, a.n1, a.T, a.gs0, a.gs1, a.ts1 = n0, n1, T, s0, s1, s1
            fill_groups(a, groups)
            a.HW, a.n_bins, a.bin_vars, a.pool_members = HW, bins.n_bins, 1, 0
            a.gen_sum, a.target_sum = ptr(sums), ptr(side)
            if extremes:
                a.gen_max, a.gen_min, a.target_max, a.target_min = (ptr(e) for e in ext)
            check(lib.sdy_binned_time_accumulate(C.byref(a), current_stream()), "sdy_binned_time_accumulate")
    count = torch.from_numpy(bins.label_counts()).to(dev)
    shape = (bins.n_bins, *lead, H, W)
    by_bin = (-1,) + (1,) * (len(shape) - 1)
    out = {"mean": sums.view(shape) / count.double().view(by_bin), "count": count}
    if extremes:
        nan = torch.full((), math.nan, dtype=torch.float32, device=dev)
        out["max"] = torch.where((count == 0).view(by_bin), nan, ext[0].view(shape))
        out["min"] = torch.where((count == 0).view(by_bin), nan, ext[1].view(shape))
    return out
