"""Time variance and lag-1 autocorrelation of every trajectory of a rollout at every grid point, on the device: the second
moments along time, which say whether the emulated weather has the right amplitude and the right memory.  The reference has
nothing of the kind; the definition is `csrc/variability.h`.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence

import torch

from ._lib import (SDY_TV_SLOTS, SdyVariabilityArgs, SdyVariabilityMapsArgs, SdyVariabilityStatsArgs, check, current_stream,
                   lib, ptr)
from .windows import FieldAccumulator, WindowLayout, fill_window, runs, whole_ics_message, window_layouts

_SUMS = ("s1", "s2", "p")


class TimeVariabilityAggregator(FieldAccumulator):
    """Per member and for the target: the standard deviation along time and the lag-1 autocorrelation at every grid point, and
    area-weighted summaries of the two.

    `record_batch(loss, target_data, gen_data, target_data_norm, gen_data_norm, i_time_start)` is what `run_inference` calls
    once per window: targets `(samples, time, lat, lon)`, gen `(members, samples, time, lat, lon)` (a 4-D gen is one
    member).  One `sdy_time_variability_accumulate` launch per run of same-shaped variables reads the window in place -- the
    member-stacked transposed view included -- and advances the state of every trajectory and grid point: with the counted
    times `x_1 .. x_n` and the origin `c = x_1`, the float64 sums of `d_t = x_t - c`, `d_t^2` and `d_{t-1} d_t`, and the
    fp32 pair `(c, x_n)`, 32 bytes in all (25 members x 63 variables x 180 x 360 need 3.4 GB).  The shift by the first value
    keeps the variance of a field with a large mean to float64 rounding of the deviations.  The state carries the run across
    window boundaries -- the lag product of a window's first time takes its predecessor from it -- and its bits do not depend
    on how the run is cut into windows.  The first time of a run (`i_time_start == 0`) is the initial condition and is not
    counted; a window that holds nothing else counts nothing.  The first window that is accepted may start anywhere and fixes
    variables, grids, member count and sample count; every later one must repeat them and start where the one before ended
    (`ValueError` otherwise).  The state is allocated on the first window, after comparing its bytes with `max_bytes`
    (default: a quarter of the device's memory).  A refused window changes nothing.

    `get_data()` returns, per variable, float64 device tensors: `gen_time_std` and `gen_lag1` `(members, samples, lat, lon)`,
    `target_time_std` and `target_lag1` `(samples, lat, lon)`; population variance, and the lag-1 autocorrelation `sum_{t >= 2}
    (x_{t-1} - m)(x_t - m) / sum_t (x_t - m)^2`, NaN where the variance is 0 (`sdy_time_variability_maps`).

    `get_logs(label)` returns Python floats per variable, in this order: `time_std_gen/<var>` and `time_std_target/<var>` (roots
    of the area-weighted means of the member-mean and of the target variance), `time_std_ratio/<var>` (gen / target),
    `time_std_rmse/<var>` (root of the weighted mean of (member-mean std - target std)^2), `lag1_gen/<var>`, `lag1_target/<var>`
    (weighted means over the points where the target and every member have a positive variance), `lag1_bias/<var>` and
    `lag1_defined_fraction/<var>` (those points' share of the weight).  One `sdy_time_variability_stats` call per run of
    same-shaped variables; sums run over samples and grid points in float64.  Fewer than two counted times: `ValueError`.

    Ranks hold whole initial conditions: the raw weighted sums and `samples * sum(weights)` are added over ranks
    (`dist.reduce_sum`) in one reduce before any root or division.  Ragged shares (flat rows with `sample_weights`) are
    refused.  Plots, masks and lags beyond 1 are out of scope."""

    accepts_sample_weights = True      # (to see, and refuse, a ragged share)

    _job_words = "member count, sample count"

    LOG_KEYS = ("time_std_gen", "time_std_target", "time_std_ratio", "time_std_rmse", "lag1_gen", "lag1_target", "lag1_bias",
                "lag1_defined_fraction")

    def __init__(self, area_weights: torch.Tensor, dist=None, target: str = "denorm", metadata=None,
                 max_bytes: Optional[int] = None):
        if target not in ("norm", "denorm"):
            raise ValueError(f"target must be 'norm' or 'denorm', got {target!r}")
        super().__init__(dist=dist, metadata=metadata, max_bytes=max_bytes)      # (no time axis)
        self._area_weights = area_weights
        self._target = target
        self._n_times = 0                          # counted times so far
        self._next_start: Optional[int] = None     # where the next window has to start (None before the first window)

    def _statistics(self) -> Dict[str, float]:
        # "pair": the fp32 pair (origin, last value) of an element in one 8-byte slot of a float64-typed buffer
        return {"s1": 0.0, "s2": 0.0, "p": 0.0, "pair": 0.0}

    @staticmethod
    def _job(l: WindowLayout) -> tuple:
        return (l.n0, l.n1, l.H, l.W)

    def _elements(self, stat: str, job: tuple) -> int:
        M, n1, H, W = job
        return (M + 1) * n1 * H * W

    def _size_words(self, names, jobs) -> str:
        return f"{len(names)} variables of {jobs[0][0]} members"

    @property
    def n_times(self) -> int:
        """Counted times so far."""
        return self._n_times

    @torch.no_grad()
    def record_batch(self, loss, target_data, gen_data, target_data_norm=None, gen_data_norm=None, i_time_start: int = 0,
                     sample_weights: Optional[Sequence[float]] = None):
        del loss
        if self._target == "norm":
            target_data, gen_data = target_data_norm, gen_data_norm
        ragged = sample_weights is not None or any(
            g.dim() == 4 and k in target_data and target_data[k].dim() == 4 and g.shape[0] != target_data[k].shape[0]
            for k, g in gen_data.items())
        if ragged:
            raise ValueError(whole_ics_message("TimeVariabilityAggregator"))
        start = int(i_time_start)
        if start < 0:
            raise ValueError(f"i_time_start must not be negative, got {start}")
        lay = window_layouts(target_data, gen_data)
        if self._next_start is not None and start != self._next_start:
            raise ValueError(f"TimeVariabilityAggregator: a window that starts at time {start}, where the one before ended at "
                             f"{self._next_start}: the lag products need every window of a run, in order")
        device = self._prepare(list(gen_data), lay)
        T = lay[0].T
        t0 = 1 if start == 0 else 0                   # the very first time of a run is the initial condition
        if T - t0 >= 1:
            with torch.cuda.device(device):
                for first, last in runs(lay, lambda l: l.extents):
                    a = SdyVariabilityArgs()
                    fill_window(a.win, lay, first, last)
                    a.HW, a.t0, a.first = lay[first].H * lay[first].W, t0, int(self._n_times == 0)
                    a.s1, a.s2, a.p = (self._at(k, first) for k in _SUMS)
                    a.origin_last = self._at("pair", first)
                    check(lib.sdy_time_variability_accumulate(C.byref(a), current_stream()), "sdy_time_variability_accumulate")
            self._n_times += T - t0
        self._next_start = start + T

    def _check_recorded(self) -> None:
        # (raised BEFORE any collective: every rank of a job must have recorded at least two counted times)
        if not self._acc or self._n_times < 2:
            raise ValueError(f"No data recorded: variance and lag-1 autocorrelation need two counted times, got {self._n_times}.")

    @torch.no_grad()
    def get_data(self) -> Dict[str, Dict[str, torch.Tensor]]:
        """{"gen_time_std", "gen_lag1": {name: (members, samples, lat, lon)}, "target_time_std", "target_lag1": {name: (samples,
        lat, lon)}}: this rank's maps so far, float64 on the device."""
        self._check_recorded()
        s1 = self._acc["s1"]
        variance, lag1 = torch.empty_like(s1), torch.empty_like(s1)
        with torch.cuda.device(s1.device):
            a = SdyVariabilityMapsArgs()
            a.n_elems, a.n_times = s1.numel(), float(self._n_times)
            a.s1, a.s2, a.p, a.origin_last = ptr(s1), ptr(self._acc["s2"]), ptr(self._acc["p"]), ptr(self._acc["pair"])
            a.variance, a.lag1 = ptr(variance), ptr(lag1)
            check(lib.sdy_time_variability_maps(C.byref(a), current_stream()), "sdy_time_variability_maps")
        std = variance.sqrt_()
        out: Dict[str, Dict[str, torch.Tensor]] = {"gen_time_std": {}, "gen_lag1": {}, "target_time_std": {}, "target_lag1": {}}
        for i, name in enumerate(self._names):
            M, n1, H, W = self._grids[i]
            at, n = self._offsets["s1"][i], n1 * H * W
            for kind, buf in (("time_std", std), ("lag1", lag1)):
                out[f"gen_{kind}"][name] = buf[at:at + M * n].view(M, n1, H, W)
                out[f"target_{kind}"][name] = buf[at + M * n:at + (M + 1) * n].view(n1, H, W)
        return out

    @torch.no_grad()
    def weighted_sums(self) -> Dict[str, torch.Tensor]:
        """Per variable the six raw weighted sums of `sdy_time_variability_stats` (this rank's), float64 on the device."""
        self._check_recorded()
        device = self._acc["s1"].device
        out = {}
        with torch.cuda.device(device):
            for first, last in runs(self._grids, lambda g: g):
                M, n1, H, W = self._grids[first]
                if tuple(self._area_weights.shape) != (H, W):
                    raise ValueError(f"area weights {tuple(self._area_weights.shape)} against a {(H, W)} grid")
                w = self._area_weights.to(device, torch.float32).contiguous()
                nvars = last - first
                res = torch.empty(nvars, SDY_TV_SLOTS, dtype=torch.float64, device=device)
                ws_bytes = lib.sdy_time_variability_workspace_bytes(nvars, n1, H * W)
                ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=device)
                a = SdyVariabilityStatsArgs()
                a.nvars, a.M, a.n1, a.HW = nvars, M, n1, H * W
                a.s1, a.s2, a.p = (self._at(k, first) for k in _SUMS)
                a.origin_last = self._at("pair", first)
                a.weights, a.n_times, a.out = ptr(w), float(self._n_times), ptr(res)
                a.ws, a.ws_bytes = ptr(ws), ws_bytes
                check(lib.sdy_time_variability_stats(C.byref(a), current_stream()), "sdy_time_variability_stats")
                for j in range(first, last):
                    out[self._names[j]] = res[j - first]
        return out

    @staticmethod
    def logs_from_sums(s: Sequence[float], den: float) -> Dict[str, float]:
        """One variable's logs from its six raw sums and the total weight `samples * sum(weights)` (both already added over
        ranks), in the order of `LOG_KEYS`."""
        nan = float("nan")
        sd_gen, sd_target = math.sqrt(s[0] / den), math.sqrt(s[1] / den)
        lag_gen, lag_target = (s[3] / s[5], s[4] / s[5]) if s[5] > 0.0 else (nan, nan)
        return {"time_std_gen": sd_gen, "time_std_target": sd_target,
                "time_std_ratio": sd_gen / sd_target if sd_target > 0.0 else nan, "time_std_rmse": math.sqrt(s[2] / den),
                "lag1_gen": lag_gen, "lag1_target": lag_target, "lag1_bias": lag_gen - lag_target,
                "lag1_defined_fraction": s[5] / den}

    @torch.no_grad()
    def get_logs(self, label: str) -> Dict[str, float]:
        sums = self.weighted_sums()
        device = self._acc["s1"].device
        wsum = self._area_weights.to(device, torch.float32).double().sum()
        # ranks hold whole initial conditions: every variable's sums and its sample count x sum(w) are added over ranks in ONE
        # reduce, before any root or division, and come to the host in one copy
        parts = []
        for i, name in enumerate(self._names):
            parts += [sums[name], (self._grids[i][1] * wsum).reshape(1)]
        packed = self._dist.reduce_sum(torch.cat(parts)).cpu().tolist()
        logs: Dict[str, float] = {}
        n = SDY_TV_SLOTS + 1
        for i, name in enumerate(self._names):
            one = self.logs_from_sums(packed[i * n:i * n + SDY_TV_SLOTS], packed[i * n + SDY_TV_SLOTS])
            logs.update({f"{k}/{name}": float(one[k]) for k in self.LOG_KEYS})
        return {f"{label}/{k}": v for k, v in logs.items()} if len(label) != 0 else logs
