"""Per-grid-point quantiles along time of gen and target, exactly, on the device: the map of the 99th percentile of daily
precipitation or of the 10 m wind, gen against target -- the classic check of a climate emulator's tails -- and the helper that
turns the target's quantile into the `(lat, lon)` threshold map `sdy_amd.Events` accepts ("2 m temperature above its local 90th
percentile").  The reference has nothing of the kind.  `HistogramDataWriter` pools the whole globe per lead time,
`TimeVariabilityAggregator` stops at second moments and `EnsembleTimeMeanAggregator` at the mean; a quantile along time at a
grid point is a function of none of them.  The definition is `csrc/quantile.h`: the trajectories are kept as sortable 32-bit
keys and the order statistics are selected out of them without sorting, so every output has the same bits in any layout,
batch, run, order and cut of the run into windows.

Out of scope: a bounded-state tail (top-k) for runs too long to store, weighted quantiles, pooling over samples or longitudes,
plots, ragged rank shares.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from ._lib import SDY_MAX_QUANTILES, SdyTimeQuantileAppendArgs, SdyTimeQuantileSelectArgs, check, current_stream, lib, ptr
from .windows import FieldAccumulator, WindowLayout, fill_window, runs, whole_ics_message, window_layouts

#: the methods of `sdy_time_quantile_select`, by their numpy names
METHODS = {"linear": 0, "lower": 1, "higher": 2}
#: what `TimeQuantileAggregator.get_logs` reports per variable and quantile, in this order (without gen: the last two)
LOG_METRICS = ("quantile_gen", "quantile_bias", "quantile_rmse", "quantile_target", "defined_fraction")
#: the key of a NaN and the fill of a series, as the int32 the series is typed with
_NOTHING = -1


def _quantile_list(quantiles) -> List[float]:
    qs = [float(q) for q in ([quantiles] if isinstance(quantiles, (int, float)) else quantiles)]
    if len(qs) == 0:
        raise ValueError("at least one quantile is needed")
    for q in qs:
        if not 0.0 <= q <= 1.0:                      # (a NaN fails both comparisons)
            raise ValueError(f"a quantile lies in [0, 1], got {q!r}")
    return qs


def _method(method: str) -> int:
    if method not in METHODS:
        raise ValueError(f"method is one of {tuple(METHODS)}, got {method!r}")
    return METHODS[method]


def _select(series_ptr: int, device, n_traj: int, capacity: int, n_slots: int, H: int, W: int, first: int, step: int, count: int,
            stride: int, n_groups: int, qs: Sequence[float], method: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (out (n_groups, Q, H, W) float64, valid (n_groups, H, W) int32) of one variable block of a series; more than
    SDY_MAX_QUANTILES quantiles are taken in several calls."""
    outs = []
    valid = torch.empty(n_groups, H, W, dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        for at in range(0, len(qs), SDY_MAX_QUANTILES):
            part = qs[at:at + SDY_MAX_QUANTILES]
            out = torch.empty(n_groups, len(part), H, W, dtype=torch.float64, device=device)
            a = SdyTimeQuantileSelectArgs()
            a.series, a.plane, a.n_traj, a.capacity, a.n_slots = series_ptr, H * W, n_traj, capacity, n_slots
            a.first, a.step, a.count, a.stride, a.n_groups = first, step, count, stride, n_groups
            a.nq, a.method = len(part), method
            for i, q in enumerate(part):
                a.q[i] = q
            a.out, a.valid = ptr(out), ptr(valid)
            check(lib.sdy_time_quantile_select(C.byref(a), current_stream()), "sdy_time_quantile_select")
            outs.append(out)
    return (outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)), valid


class TimeQuantileAggregator(FieldAccumulator):
    """Per variable and grid point the quantiles along time of the generated trajectories -- pooled over the members of a
    sample, and per member when asked -- and of the target, and area-weighted summaries of their difference.

    Definition (csrc/quantile.h).  The values of a group of trajectories at a grid point are its values at all recorded
    counted times that are not NaN (nanquantile semantics); n is their number, and a point with n == 0 gives NaN: the way an
    ocean-only field masks land.  With h = q (n - 1), j = min(floor(h), n - 1) and g = h - j in float64, lo is the j-th
    smallest value (0-based) and hi the min(j + 1, n - 1)-th.  `method="lower"` returns lo, `"higher"` hi when g > 0 and lo
    otherwise, `"linear"` lo when g == 0 or lo == hi and otherwise numpy's `_lerp` of the two in float64 (hi - (hi - lo)(1 - g)
    when g >= 0.5, else lo + (hi - lo) g).  `lower` and `higher` are always exactly an fp32 value of the input; the sign of a
    zero is canonical (+0.0).

    `record_batch(loss, target_data, gen_data, target_data_norm, gen_data_norm, i_time_start)` is what `run_inference` calls
    once per window: targets `(samples, time, lat, lon)`, gen `(members, samples, time, lat, lon)` (a 4-D gen is one member).
    Only `variables` are read (`None`: all generated variables).  One `sdy_time_quantile_append` launch per run of variables
    with equal extents reads the window in place -- the member-stacked transposed view included -- and writes its values as
    sortable 32-bit keys into the series `(trajectories, capacity, lat x lon)` of every variable: `members x samples + samples`
    trajectories (the targets alone with `store_gen=False`: the cheap way to threshold maps from a long target run), capacity
    `n_timesteps - 1` counted times.  Time 0 of a run is the initial condition and is not counted; window time `i_time_start +
    t` goes to slot `i_time_start + t - 1`.  Windows may arrive in any order; a time recorded twice or outside the capacity
    raises `ValueError`.  The series is allocated on the first accepted window, filled with the NaN key, after its bytes --
    4 x trajectories x capacity x lat x lon per variable -- are compared with `max_bytes` (default: a quarter of the device's
    memory): 26 trajectories at 180 x 360 are 6.7 MB per variable and counted time.  The first window that is accepted fixes
    variables, grids, member count and sample count; a refused window changes nothing.  `target="norm"` reads the normalised
    data instead.

    `get_data()` returns float64 device tensors per variable (this rank's samples): `gen/<variable>` `(samples, Q, lat, lon)`,
    members pooled; `target/<variable>` `(samples, Q, lat, lon)`; with `per_member` `gen_members/<variable>` `(members,
    samples, Q, lat, lon)`; the valid counts `gen_count/<variable>` and `target_count/<variable>` `(samples, lat, lon)`; and
    `quantiles` `(Q,)`.  One `sdy_time_quantile_select` call per grouping: selection by digits, no sort and no copy of the
    series.

    `get_logs(label)` returns Python floats `<metric>/q<q:g>/<variable>`.  With w the area weights and D the (sample, grid
    point) pairs at which both quantiles are defined (not NaN): `quantile_gen` = sum_D w gen / sum_D w, `quantile_target`
    likewise, `quantile_bias` their difference, `quantile_rmse` = sqrt(sum_D w (gen - target)^2 / sum_D w), `defined_fraction`
    = sum_D w / sum over all pairs of w.  The raw sums are added over ranks in ONE `dist.reduce_sum` before anything is
    divided.  Without gen (`store_gen=False`) D is where the target is defined and only `quantile_target` and
    `defined_fraction` are reported.  `ValueError("No data recorded.")` before any collective when nothing was counted.  Ranks
    hold whole initial conditions; ragged shares (flat rows with `sample_weights`) are refused.

    `threshold_map(variable, q, side="target", sample=0, method="higher")` returns the fp32 `(lat, lon)` device tensor of one
    sample's quantile -- exact, because `lower` and `higher` are input values; NaN where nothing was valid -- which
    `Events.add(variable, name, above=...)` accepts."""

    accepts_sample_weights = True
    _job_words = "member count, sample count"
    _acc_dtype = torch.int32
    _acc_words = "sortable 32-bit keys"

    def __init__(self, quantiles, area_weights: torch.Tensor, n_timesteps: int, variables: Optional[Sequence[str]] = None,
                 store_gen: bool = True, per_member: bool = False, method: str = "linear", target: str = "denorm", dist=None,
                 metadata=None, max_bytes: Optional[int] = None):
        super().__init__(n_timesteps, dist=dist, metadata=metadata, max_bytes=max_bytes)
        if self._n_timesteps < 2:
            raise ValueError(f"n_timesteps must be at least 2 (time 0 is the initial condition), got {n_timesteps}")
        if target not in ("norm", "denorm"):
            raise ValueError(f"target must be 'norm' or 'denorm', got {target!r}")
        if area_weights.dim() != 2:
            raise ValueError(f"area weights are (lat, lon), got {tuple(area_weights.shape)}")
        self._quantiles = _quantile_list(quantiles)
        self._method = _method(method)
        self._area_weights = area_weights
        self._variables = None if variables is None else list(variables)
        if self._variables is not None and len(self._variables) == 0:
            raise ValueError("variables=[] selects nothing (None: all generated variables)")
        self._store_gen = bool(store_gen)
        self._per_member = bool(per_member)
        if self._per_member and not self._store_gen:
            raise ValueError("per_member needs store_gen=True")
        self._target = target
        self._capacity = self._n_timesteps - 1
        self._slots = [False] * self._capacity           # host-side record of the counted times that were written

    def _statistics(self) -> Dict[str, float]:
        return {"series": _NOTHING}

    def _job(self, l: WindowLayout) -> tuple:
        """(members, samples, lat, lon); without gen the member count is not part of the job (0)."""
        return (l.n0 if self._store_gen else 0, l.n1, l.H, l.W)

    def _n_traj(self, job: tuple) -> int:
        return job[0] * job[1] + job[1]

    def _elements(self, stat: str, job: tuple) -> int:
        return self._n_traj(job) * self._capacity * job[2] * job[3]

    def _size_words(self, names, jobs) -> str:
        M, n1, H, W = jobs[0]
        rows = f"{M} members x {n1} samples + {n1} targets" if self._store_gen else f"{n1} targets"
        return (f"4 bytes x {self._n_traj(jobs[0])} trajectories ({rows}) x {self._capacity} counted times x {H} x {W} grid "
                f"points x {len(names)} variables")

    @property
    def n_times(self) -> int:
        """Counted times recorded so far."""
        return sum(self._slots)

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
            raise ValueError(f"no generated variable {missing[0]!r} in the window, but its quantiles were asked for")
        lay = window_layouts(target_data, {k: gen_data[k] for k in names})
        T = lay[0].T
        if start < 0 or start + T > self._n_timesteps:
            raise ValueError(f"times {start}..{start + T - 1} outside the aggregator's {self._n_timesteps}")
        t0 = 1 if start == 0 else 0                      # the very first time of a run is the initial condition
        slot0 = start + t0 - 1
        twice = [s + 1 for s in range(slot0, slot0 + T - t0) if self._slots[s]]
        if twice:
            raise ValueError(f"{type(self).__name__}: time {twice[0]} is recorded already (a time is recorded once)")
        device = self._prepare(names, lay)
        with torch.cuda.device(device):
            for first, last in runs(lay, lambda l: l.extents):
                a = SdyTimeQuantileAppendArgs()
                fill_window(a.win, lay, first, last)
                l = lay[first]
                if not self._store_gen:                  # the gen rows are not read; a window still needs valid ones
                    for j in range(first, last):
                        a.gen[j - first] = ptr(lay[j].target)
                    a.n0, a.gs0, a.gs1 = 1, 0, l.ts1
                a.H, a.W, a.t0, a.slot0, a.capacity, a.store_gen = l.H, l.W, t0, slot0, self._capacity, int(self._store_gen)
                a.series = self._at("series", first)
                check(lib.sdy_time_quantile_append(C.byref(a), current_stream()), "sdy_time_quantile_append")
        for s in range(slot0, slot0 + T - t0):
            self._slots[s] = True

    def _recorded(self) -> None:
        # (raised BEFORE any collective: every rank of a job must have counted at least one time)
        if self._names is None or not any(self._slots):
            raise ValueError("No data recorded.")

    def _groups(self, i: int, which: str) -> tuple:
        """-> (first, step, count, stride, n_groups) of a grouping of variable i's trajectories."""
        M, n1 = self._grids[i][:2]
        if which == "gen":
            return (0, 1, M, n1, n1)
        if which == "gen_members":
            return (0, 1, 1, 0, M * n1)
        return (M * n1, 1, 1, 0, n1)

    def _quantiles_of(self, i: int, which: str, qs: Sequence[float], method: int):
        M, n1, H, W = self._grids[i]
        n_slots = max(s for s, on in enumerate(self._slots) if on) + 1
        return _select(self._at("series", i), self._acc["series"].device, self._n_traj(self._grids[i]), self._capacity, n_slots,
                       H, W, *self._groups(i, which), qs, method)

    @torch.no_grad()
    def get_data(self) -> Dict[str, torch.Tensor]:
        self._recorded()
        data: Dict[str, torch.Tensor] = {}
        for i, name in enumerate(self._names):
            M, n1, H, W = self._grids[i]
            if self._store_gen:
                data[f"gen/{name}"], count = self._quantiles_of(i, "gen", self._quantiles, self._method)
                data[f"gen_count/{name}"] = count.to(torch.float64)
                if self._per_member:
                    out, _ = self._quantiles_of(i, "gen_members", self._quantiles, self._method)
                    data[f"gen_members/{name}"] = out.view(M, n1, len(self._quantiles), H, W)
            data[f"target/{name}"], count = self._quantiles_of(i, "target", self._quantiles, self._method)
            data[f"target_count/{name}"] = count.to(torch.float64)
        data["quantiles"] = torch.tensor(self._quantiles, dtype=torch.float64, device=self._acc["series"].device)
        return data

    @torch.no_grad()
    def get_logs(self, label: str) -> Dict[str, float]:
        self._recorded()
        parts = []
        for i, name in enumerate(self._names):
            H, W = self._grids[i][2:]
            if tuple(self._area_weights.shape) != (H, W):
                raise ValueError(f"area weights {tuple(self._area_weights.shape)} against a {(H, W)} grid")
            target, _ = self._quantiles_of(i, "target", self._quantiles, self._method)
            gen = self._quantiles_of(i, "gen", self._quantiles, self._method)[0] if self._store_gen else target
            w = self._area_weights.to(target.device, torch.float64)
            both = ~(torch.isnan(gen) | torch.isnan(target))
            zero = torch.zeros((), dtype=torch.float64, device=target.device)
            g, t = torch.where(both, gen, zero), torch.where(both, target, zero)
            wb = w * both.to(torch.float64)                                   # (samples, Q, lat, lon)
            total = (w.sum() * target.shape[0]).expand(len(self._quantiles))
            parts.append(torch.stack([wb.sum(dim=(0, 2, 3)), (wb * g).sum(dim=(0, 2, 3)), (wb * t).sum(dim=(0, 2, 3)),
                                      (wb * (g - t) ** 2).sum(dim=(0, 2, 3)), total]).reshape(-1))
        packed = self._dist.reduce_sum(torch.cat(parts)).cpu().view(len(self._names), 5, len(self._quantiles)).tolist()
        logs: Dict[str, float] = {}
        nan = float("nan")
        for i, name in enumerate(self._names):
            for k, q in enumerate(self._quantiles):
                sw, sg, st, sd, total = (packed[i][j][k] for j in range(5))
                one = {"quantile_gen": sg / sw if sw > 0.0 else nan, "quantile_bias": (sg - st) / sw if sw > 0.0 else nan,
                       "quantile_rmse": math.sqrt(sd / sw) if sw > 0.0 else nan,
                       "quantile_target": st / sw if sw > 0.0 else nan, "defined_fraction": sw / total if total > 0.0 else nan}
                for metric in (LOG_METRICS if self._store_gen else LOG_METRICS[3:]):
                    logs[f"{metric}/q{q:g}/{name}"] = float(one[metric])
        return {f"{label}/{k}": v for k, v in logs.items()} if len(label) != 0 else logs

    @torch.no_grad()
    def threshold_map(self, variable: str, q: float, side: str = "target", sample: int = 0, method: str = "higher") -> torch.Tensor:
        self._recorded()
        if variable not in self._names:
            raise ValueError(f"no quantiles of {variable!r} are kept (kept: {self._names})")
        if side not in ("target", "gen") or (side == "gen" and not self._store_gen):
            raise ValueError(f"side is 'target'{' or gen' if self._store_gen else ''}, got {side!r}")
        if method not in ("lower", "higher"):
            raise ValueError(f"a threshold map is an input value: method 'lower' or 'higher', got {method!r}")
        i = self._names.index(variable)
        n1 = self._grids[i][1]
        if not 0 <= int(sample) < n1:
            raise ValueError(f"sample {sample} outside the window's {n1}")
        out, _ = self._quantiles_of(i, side, _quantile_list(q), _method(method))
        return out[int(sample), 0].to(torch.float32)


@torch.no_grad()
def time_quantiles(x: torch.Tensor, q, method: str = "linear") -> torch.Tensor:
    """The quantiles `q` (a number or a sequence, each in [0, 1]) along time of one `(time, lat, lon)` device tensor ->
    `(Q, lat, lon)` float64; NaNs are left out, NaN where every time is NaN (`TimeQuantileAggregator`'s definition; every time
    is counted).  One append, one select."""
    if x.dim() != 3:
        raise ValueError(f"expected (time, lat, lon), got {tuple(x.shape)}")
    qs, m = _quantile_list(q), _method(method)
    if not x.is_cuda:
        raise RuntimeError("sdy_amd aggregators run on the GPU only (no CPU fallback)")
    T, H, W = x.shape
    if min(T, H, W) < 1:
        raise ValueError("empty tensor")
    x = x.to(torch.float32).contiguous()
    series = torch.full((T, H * W), _NOTHING, dtype=torch.int32, device=x.device)
    a = SdyTimeQuantileAppendArgs()
    a.nvars, a.gen[0], a.target[0] = 1, ptr(x), ptr(x)
    a.n0, a.n1, a.T, a.gs0, a.gs1, a.ts1 = 1, 1, T, 0, 0, 0
    a.H, a.W, a.t0, a.slot0, a.capacity, a.store_gen, a.series = H, W, 0, 0, T, 0, ptr(series)
    with torch.cuda.device(x.device):
        check(lib.sdy_time_quantile_append(C.byref(a), current_stream()), "sdy_time_quantile_append")
    out, _ = _select(ptr(series), x.device, 1, T, T, H, W, 0, 1, 1, 0, 1, qs, m)
    return out[0]
