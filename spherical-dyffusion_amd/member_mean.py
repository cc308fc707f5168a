"""Statistics of the per-member time-mean state of an ensemble rollout, on the device: mirror of the reference's
`src/evaluation/aggregators/time_mean.py::TimeMeanAggregator(is_ensemble=True)` (its twin:
`src/ace_inference/core/aggregator/inference/time_mean_salva.py`), the class its full-rollout evaluation scores ensembles with.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import torch

from ._lib import SDY_MEMBER_STATS_MAX_MEMBERS, SdyMemberStatsArgs, SdyMemberSumArgs, check, current_stream, lib, ptr
from .windows import FieldAccumulator, WindowLayout, fill_window, runs, whole_ics_message, window_layouts


class EnsembleTimeMeanAggregator(FieldAccumulator):
    """One time-mean map per member, and the reference's numbers on them.

    `record_batch(loss, target_data, gen_data, target_data_norm, gen_data_norm, i_time_start)` is what `run_inference` calls
    once per window: targets `(samples, time, lat, lon)`, gen `(members, samples, time, lat, lon)` (a 4-D gen is one
    member).  One `sdy_member_time_sum` launch per run of same-shaped variables reads the window in place -- the
    member-stacked transposed view included -- and adds it to float64 accumulators on the device: gen `(members, samples,
    lat, lon)` and target `(samples, lat, lon)` per variable.  The first time of a run (`i_time_start == 0`) is the initial
    condition and is not counted.  Every window covers the same samples; the accumulators are per sample, as in
    `ZonalMeanAggregator`.  They are allocated on the first batch, after comparing their bytes with `max_bytes` (default: a
    quarter of the device's memory; 25 members x 63 variables x 180 x 360 need 816 MB).  The first window that is
    accepted fixes variables, grids, member count and sample count; a later window with others raises `ValueError`, and a
    refused window changes nothing.

    `get_logs(label)` returns Python floats under the reference's keys, in its order per variable: `rmse_member_avg/<var>`
    (the mean over members of the square root of each member's pooled MSE) and `bias_member_avg/<var>` when there is more
    than one member, `rmse/<var>` and `bias/<var>` of the ensemble mean of the time means, `crps/<var>` (fair, of the
    members' time means against the target's) when there is more than one member.  `spread=True` adds this library's own
    `spread/<var>` = sqrt(mean member variance (M + 1) / M) and `ssr/<var>` = spread / rmse.  One `sdy_member_map_stats` call
    per run of same-shaped variables; sums run over samples and grid points, float64 throughout (the reference: fp32).
    `time_mean_maps()` returns the maps themselves.  The reference's images and xarray dataset, and masks, are out of scope.

    Ranks.  The reference does not reduce here (its reduce is commented out).  This library's rule: ranks hold whole initial
    conditions, and the raw weighted sums and `samples * sum(weights)` are added over ranks (`dist.reduce_sum`) before any
    square root or division: every sample weighs the same whatever the sharding, and one process gets exactly the
    reference's numbers.  Ragged shares (flat rows with `sample_weights`) are refused."""

    accepts_sample_weights = True      # (to see, and refuse, a ragged share)

    _job_words = "member count, sample count"

    def __init__(self, area_weights: torch.Tensor, dist=None, target: str = "denorm", metadata=None, spread: bool = False,
                 max_bytes: Optional[int] = None):
        if target not in ("norm", "denorm"):
            raise ValueError(f"target must be 'norm' or 'denorm', got {target!r}")
        super().__init__(dist=dist, metadata=metadata, max_bytes=max_bytes)      # (no time axis)
        self._area_weights = area_weights
        self._target = target
        self._spread = bool(spread)
        self._n_times = 0

    def _statistics(self) -> Dict[str, float]:
        return {"gen_sum": 0.0, "target_sum": 0.0}

    @staticmethod
    def _job(l: WindowLayout) -> tuple:
        return (l.n0, l.n1, l.H, l.W)

    def _elements(self, stat: str, job: tuple) -> int:
        M, n1, H, W = job
        return (M if stat == "gen_sum" else 1) * n1 * H * W

    def _size_words(self, names, jobs) -> str:
        return f"{len(names)} variables of {jobs[0][0]} members"

    @property
    def _gen_sum(self) -> Optional[torch.Tensor]:
        """Flat float64: the variables' (members, samples, lat, lon) blocks (None before the first window)."""
        return self._acc.get("gen_sum")

    @property
    def _target_sum(self) -> Optional[torch.Tensor]:
        return self._acc.get("target_sum")

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
            raise ValueError(whole_ics_message("EnsembleTimeMeanAggregator"))
        lay = window_layouts(target_data, gen_data)
        device = self._prepare(list(gen_data), lay)
        T = lay[0].T
        t0 = 1 if int(i_time_start) == 0 else 0       # the very first time of a run is the initial condition
        if T - t0 < 1:
            return                                    # a window that holds the initial condition only
        with torch.cuda.device(device):
            for first, last in runs(lay, lambda l: l.extents):
                a = SdyMemberSumArgs()
                fill_window(a.win, lay, first, last)
                a.HW, a.t0 = lay[first].H * lay[first].W, t0
                a.gen_sum, a.target_sum = self._at("gen_sum", first), self._at("target_sum", first)
                check(lib.sdy_member_time_sum(C.byref(a), current_stream()), "sdy_member_time_sum")
        self._n_times += T - t0

    def _check_recorded(self) -> None:
        # (raised BEFORE any collective: every rank of a job must have recorded at least one window)
        if self._gen_sum is None or self._n_times == 0:
            raise ValueError("No data recorded.")

    @torch.no_grad()
    def time_mean_maps(self) -> Dict[str, Dict[str, torch.Tensor]]:
        """{"gen": {name: (members, samples, lat, lon)}, "target": {name: (samples, lat, lon)}}: this rank's time means so
        far, float64 on the device."""
        self._check_recorded()
        out: Dict[str, Dict[str, torch.Tensor]] = {"gen": {}, "target": {}}
        # a device tensor as the divisor: a true division, as in sdy_member_map_stats (a Python scalar multiplies by 1 / n)
        n = torch.full((), float(self._n_times), dtype=torch.float64, device=self._gen_sum.device)
        for i, name in enumerate(self._names):
            M, n1, H, W = self._grids[i]
            out["gen"][name] = self._view("gen_sum", i, M, n1, H, W) / n
            out["target"][name] = self._view("target_sum", i, n1, H, W) / n
        return out

    @torch.no_grad()
    def weighted_sums(self) -> Dict[str, torch.Tensor]:
        """Per variable the 2 M + 4 raw weighted sums of `sdy_member_map_stats` (this rank's), float64 on the device."""
        self._check_recorded()
        device = self._gen_sum.device
        out = {}
        with torch.cuda.device(device):
            for first, last in runs(self._grids, lambda g: g):
                M, n1, H, W = self._grids[first]
                if M > SDY_MEMBER_STATS_MAX_MEMBERS:
                    raise ValueError(f"at most {SDY_MEMBER_STATS_MAX_MEMBERS} members, got {M}")
                if tuple(self._area_weights.shape) != (H, W):
                    raise ValueError(f"area weights {tuple(self._area_weights.shape)} against a {(H, W)} grid")
                w = self._area_weights.to(device, torch.float32).contiguous()
                nvars = last - first
                res = torch.empty(nvars, 2 * M + 4, dtype=torch.float64, device=device)
                ws_bytes = lib.sdy_member_stats_workspace_bytes(nvars, M, n1, H * W)
                ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=device)
                a = SdyMemberStatsArgs()
                a.nvars, a.M, a.n1, a.HW = nvars, M, n1, H * W
                a.gen_sum, a.target_sum = self._at("gen_sum", first), self._at("target_sum", first)
                a.weights, a.n_times, a.out = ptr(w), float(self._n_times), ptr(res)
                a.ws, a.ws_bytes = ptr(ws), ws_bytes
                check(lib.sdy_member_map_stats(C.byref(a), current_stream()), "sdy_member_map_stats")
                for j in range(first, last):
                    out[self._names[j]] = res[j - first]
        return out

    @torch.no_grad()
    def get_logs(self, label: str) -> Dict[str, float]:
        sums = self.weighted_sums()
        device = self._gen_sum.device
        wsum = self._area_weights.to(device, torch.float32).double().sum()
        # ranks hold whole initial conditions: every variable's sums and its sample count x sum(w) are added over ranks in ONE
        # reduce, before any root or division, and come to the host in one copy
        parts = []
        for i, name in enumerate(self._names):
            parts += [sums[name], (self._grids[i][1] * wsum).reshape(1)]
        packed = self._dist.reduce_sum(torch.cat(parts)).cpu()
        logs: Dict[str, float] = {}
        at = 0
        for i, name in enumerate(self._names):
            M = self._grids[i][0]
            s = packed[at:at + 2 * M + 4] / packed[at + 2 * M + 4]
            at += 2 * M + 5
            rmse = float(s[2 * M].sqrt())
            if M > 1:
                logs[f"rmse_member_avg/{name}"] = float(s[:M].sqrt().mean())
                logs[f"bias_member_avg/{name}"] = float(s[M:2 * M].mean())
            logs[f"rmse/{name}"] = rmse
            logs[f"bias/{name}"] = float(s[2 * M + 1])
            if M > 1:
                logs[f"crps/{name}"] = float(s[2 * M + 2])
            if self._spread:
                spread = float((s[2 * M + 3] * (M + 1) / M).sqrt())
                logs[f"spread/{name}"] = spread
                logs[f"ssr/{name}"] = spread / rmse if rmse > 0.0 else float("nan")
        return {f"{label}/{k}": v for k, v in logs.items()} if len(label) != 0 else logs
