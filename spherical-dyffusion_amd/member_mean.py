"""Statistics of the per-member time-mean state of an ensemble rollout, on the device: mirror of the reference's
`src/evaluation/aggregators/time_mean.py::TimeMeanAggregator(is_ensemble=True)` (its twin:
`src/ace_inference/core/aggregator/inference/time_mean_salva.py`), the class its full-rollout evaluation scores ensembles with.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import torch

from ._lib import (SDY_MAX_VARS, SDY_MEMBER_STATS_MAX_MEMBERS, SdyMemberStatsArgs, SdyMemberSumArgs, check, current_stream,
                   lib, ptr)
from .metrics import TorchDistributed, whole_ics_message, window_layouts


def window_grids(lay) -> List[tuple]:
    """Per variable (members, samples, lat, lon) of `window_layouts`' result."""
    return [(l[2], l[3], l[8], l[9]) for l in lay]


def check_same_job(names: List[str], grids: List[tuple], first_names: List[str], first_grids: List[tuple]) -> None:
    """A later window must hold the first window's variables, in its order, on its grids, with its member and sample count."""
    if list(names) != list(first_names) or list(grids) != list(first_grids):
        raise ValueError("the variables, member count, sample count or grids of a window differ from the first window's")


class EnsembleTimeMeanAggregator:
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

    def __init__(self, area_weights: torch.Tensor, dist=None, target: str = "denorm", metadata=None, spread: bool = False,
                 max_bytes: Optional[int] = None):
        if target not in ("norm", "denorm"):
            raise ValueError(f"target must be 'norm' or 'denorm', got {target!r}")
        self._area_weights = area_weights
        self._dist = TorchDistributed() if dist is None else dist
        self._target = target
        self._metadata = {} if metadata is None else metadata
        self._spread = bool(spread)
        self._max_bytes = max_bytes
        self._names: Optional[List[str]] = None
        self._grids: List[tuple] = []                  # per variable (members, samples, lat, lon)
        self._gen_sum: Optional[torch.Tensor] = None   # flat float64: the variables' (members, samples, lat, lon) blocks
        self._target_sum: Optional[torch.Tensor] = None
        self._gen_at: List[int] = []
        self._target_at: List[int] = []
        self._n_times = 0

    def _prepare(self, names: List[str], lay) -> torch.device:
        """Everything is checked before anything changes: a refused window leaves the aggregator as it was."""
        grids = window_grids(lay)
        on_device = all(l[0].is_cuda and l[1].is_cuda for l in lay)
        if self._names is None:
            need = 8 * sum(n1 * H * W * (M + 1) for M, n1, H, W in grids)
            limit = self._max_bytes
            if limit is None and on_device:
                limit = torch.cuda.get_device_properties(lay[0][0].device).total_memory // 4
            if limit is not None and need > limit:
                raise ValueError(f"EnsembleTimeMeanAggregator: {len(names)} variables of {grids[0][0]} members need {need} "
                                 f"bytes of float64 accumulators, more than max_bytes = {limit}")
        else:
            check_same_job(names, grids, self._names, self._grids)
        if not on_device:
            raise RuntimeError("sdy_amd aggregators run on the GPU only (no CPU fallback)")
        if self._names is None:
            device = lay[0][0].device
            gen_at, target_at, g_at, t_at = [], [], 0, 0
            for M, n1, H, W in grids:
                gen_at.append(g_at)
                target_at.append(t_at)
                g_at += M * n1 * H * W
                t_at += n1 * H * W
            self._gen_sum = torch.zeros(g_at, dtype=torch.float64, device=device)
            self._target_sum = torch.zeros(t_at, dtype=torch.float64, device=device)
            self._gen_at, self._target_at = gen_at, target_at
            self._names, self._grids = list(names), grids
        return self._gen_sum.device

    def _runs(self, key=lambda i: None):
        """Runs of consecutive variables that one launch takes: the same grid and `key`, at most SDY_MAX_VARS."""
        first, n = 0, len(self._grids)
        while first < n:
            last = first + 1
            while (last < n and last - first < SDY_MAX_VARS and self._grids[last] == self._grids[first]
                   and key(last) == key(first)):
                last += 1
            yield first, last
            first = last

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
        for l in lay:
            if l[0].device != device or l[1].device != device:
                raise ValueError(f"tensors on {l[0].device} / {l[1].device}, accumulators on {device}")
        T = lay[0][7]
        t0 = 1 if int(i_time_start) == 0 else 0       # the very first time of a run is the initial condition
        if T - t0 < 1:
            return                                    # a window that holds the initial condition only
        with torch.cuda.device(device):
            for first, last in self._runs(lambda i: lay[i][2:]):
                a = SdyMemberSumArgs()
                a.nvars = last - first
                for j in range(first, last):
                    a.gen[j - first], a.target[j - first] = ptr(lay[j][0]), ptr(lay[j][1])
                _, _, a.n0, a.n1, a.gs0, a.gs1, a.ts1, a.T, H, W = lay[first]
                a.HW, a.t0 = H * W, t0
                a.gen_sum = self._gen_sum.data_ptr() + 8 * self._gen_at[first]
                a.target_sum = self._target_sum.data_ptr() + 8 * self._target_at[first]
                check(lib.sdy_member_time_sum(C.byref(a), current_stream()), "sdy_member_time_sum")
        self._n_times += T - t0

    def _check_recorded(self) -> None:
        # (raised BEFORE any collective: every rank of a job must have recorded at least one window)
        if self._gen_sum is None or self._n_times == 0:
            raise ValueError("No data recorded.")

    def _block(self, i: int):
        M, n1, H, W = self._grids[i]
        g = self._gen_sum[self._gen_at[i]:self._gen_at[i] + M * n1 * H * W]
        t = self._target_sum[self._target_at[i]:self._target_at[i] + n1 * H * W]
        return g, t

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
            g, t = self._block(i)
            out["gen"][name] = g.view(M, n1, H, W) / n
            out["target"][name] = t.view(n1, H, W) / n
        return out

    @torch.no_grad()
    def weighted_sums(self) -> Dict[str, torch.Tensor]:
        """Per variable the 2 M + 4 raw weighted sums of `sdy_member_map_stats` (this rank's), float64 on the device."""
        self._check_recorded()
        device = self._gen_sum.device
        out = {}
        with torch.cuda.device(device):
            for first, last in self._runs():
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
                a.gen_sum = self._gen_sum.data_ptr() + 8 * self._gen_at[first]
                a.target_sum = self._target_sum.data_ptr() + 8 * self._target_at[first]
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
