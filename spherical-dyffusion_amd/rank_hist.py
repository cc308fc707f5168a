"""Rank (Talagrand) histograms of an ensemble rollout per latitude, on the device: is the truth one more member?  The
reference has nothing of the kind; `weighted_ssr` and `EnsembleTimeMeanAggregator(spread=True)` say how wide an ensemble is,
this says whether it is calibrated, and where.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import torch

from ._lib import SDY_RANK_HIST_MAX_MEMBERS, SdyRankHistArgs, check, current_stream, lib
from .windows import FieldAccumulator, WindowLayout, fill_slots, fill_window, runs, whole_ics_message, window_layouts


class RankHistogramAggregator(FieldAccumulator):
    """Per variable, lead time and latitude: how many grid points had `rank` members strictly below the truth.

    Definition.  For the target y and the members g_0 .. g_{M-1} of a grid point, rank = #{m : g_m < y}, 0 .. M.  A point
    whose target is NaN is counted nowhere; a NaN member is not below.  The point is a tie when y is not NaN and some g_m ==
    y: ties do not change the rank and are counted apart, so that a reader sees when the strict inequality matters (clipped
    fields such as precipitation).  Flat frequencies mean calibrated, U-shaped under-dispersive, sloped biased.

    `record_batch(loss, target_data, gen_data, target_data_norm, gen_data_norm, i_time_start)` is what `run_inference` calls
    once per window: targets `(samples, time, lat, lon)`, gen `(members, samples, time, lat, lon)` (a 4-D gen is one member:
    two bins).  One `sdy_rank_hist_accumulate` launch per run of same-shaped variables reads the window in place -- the
    member-stacked transposed view included -- and adds it to float64 accumulators on the device: `counts (n_slots, lat, M +
    1)` and `ties (n_slots, lat)` per variable, pooled over samples and longitudes.  The slot of window time t is the lead
    time `i_time_start + t` of `n_timesteps`; `pool_times=True` keeps ONE slot (long rollouts).  The first time of a run
    (`i_time_start == 0`) is the initial condition and is not counted.  The counts are integers held as float64 (exact below
    2^53, in any order): the same bits in any layout, batch, run and rank count.  The first window that is accepted fixes
    variables, grids, member count and sample count; a later window with others raises `ValueError`, and a refused window
    changes nothing.  Normalisation does not change a rank: the denormalised data are read.

    `area_weights` is `(lat, lon)`; the weight of a latitude is its row's mean.  Keeping the latitude axis makes the area
    weighting exact at read time, for weights that are constant along a row (every grid of this project); others raise
    `ValueError` at construction.

    `get_data()` returns float64 device tensors per variable, added over ranks (`dist.reduce_sum`): `counts/<var>`
    `(n_slots, lat, M + 1)`, `ties/<var>` `(n_slots, lat)` and `frequency/<var>` `(n_slots, M + 1)` = sum_lat w_lat counts /
    sum_lat,k w_lat counts (NaN for a slot without counts).  `get_logs(label)` returns Python floats per variable from the
    counts pooled over all slots, with F the pooled frequency: `reliability_index/<var>` = sum_k |F_k - 1 / (M + 1)|,
    `outlier_fraction/<var>` = F_0 + F_M (expected 2 / (M + 1)) and `tie_fraction/<var>` = sum_lat w_lat ties / sum_lat,k w_lat
    counts.  Ranks hold whole initial conditions; ragged shares (flat rows with `sample_weights`) are refused.  Random or
    fractional tie-breaking, masks and plots are out of scope."""

    accepts_sample_weights = True      # (to see, and refuse, a ragged share)

    _job_words = "member count, sample count"

    def __init__(self, area_weights: torch.Tensor, n_timesteps: int, pool_times: bool = False, dist=None, metadata=None,
                 max_bytes: Optional[int] = None):
        super().__init__(n_timesteps, dist=dist, metadata=metadata, max_bytes=max_bytes)
        if area_weights.dim() != 2:
            raise ValueError(f"area weights are (lat, lon), got {tuple(area_weights.shape)}")
        if not bool((area_weights == area_weights[:, :1]).all()):
            raise ValueError("RankHistogramAggregator: the area weights vary along a latitude row; counts that are pooled "
                             "over longitudes cannot weight them exactly")
        self._area_weights = area_weights
        self._pool_times = bool(pool_times)
        self._n_slots = 1 if self._pool_times else self._n_timesteps

    def _statistics(self) -> Dict[str, float]:
        return {"counts": 0.0, "ties": 0.0}

    @staticmethod
    def _job(l: WindowLayout) -> tuple:
        return (l.n0, l.n1, l.H, l.W)

    def _elements(self, stat: str, job: tuple) -> int:
        M, _, H, _ = job
        return self._n_slots * H * (M + 1 if stat == "counts" else 1)

    def _size_words(self, names, jobs) -> str:
        return f"{len(names)} variables of {jobs[0][0]} members x {self._n_slots} slots"

    @torch.no_grad()
    def record_batch(self, loss, target_data, gen_data, target_data_norm=None, gen_data_norm=None, i_time_start: int = 0,
                     sample_weights: Optional[Sequence[float]] = None):
        del loss, target_data_norm, gen_data_norm
        ragged = sample_weights is not None or any(
            g.dim() == 4 and k in target_data and target_data[k].dim() == 4 and g.shape[0] != target_data[k].shape[0]
            for k, g in gen_data.items())
        if ragged:
            raise ValueError(whole_ics_message("RankHistogramAggregator"))
        i_time_start = int(i_time_start)
        lay = window_layouts(target_data, gen_data)
        T = lay[0].T
        if i_time_start < 0 or i_time_start + T > self._n_timesteps:
            raise ValueError(f"times {i_time_start}..{i_time_start + T - 1} outside the aggregator's {self._n_timesteps}")
        if any(l.n0 > SDY_RANK_HIST_MAX_MEMBERS for l in lay):
            raise ValueError(f"at most {SDY_RANK_HIST_MAX_MEMBERS} members, got {max(l.n0 for l in lay)}")
        device = self._prepare(list(gen_data), lay)
        t0 = 1 if i_time_start == 0 else 0            # the very first time of a run is the initial condition
        with torch.cuda.device(device):
            for first, last in runs(lay, lambda l: l.extents):
                a = SdyRankHistArgs()
                fill_window(a.win, lay, first, last)
                a.H, a.W = lay[first].H, lay[first].W
                fill_slots(a.slots, t0, i_time_start, self._n_slots, self._pool_times)
                a.counts, a.ties = self._at("counts", first), self._at("ties", first)
                check(lib.sdy_rank_hist_accumulate(C.byref(a), current_stream()), "sdy_rank_hist_accumulate")
        for t in range(i_time_start + t0, i_time_start + T):
            self._n_batches[t] += 1

    def _reduced(self) -> Dict[str, torch.Tensor]:
        # (raised BEFORE any collective: every rank of a job must have recorded at least one window)
        if self._names is None:
            raise ValueError("No data recorded.")
        return {stat: self._dist.reduce_sum(acc) for stat, acc in self._acc.items()}

    def _lat_weights(self, i: int, device) -> torch.Tensor:
        H, W = self._grids[i][2:]
        if tuple(self._area_weights.shape) != (H, W):
            raise ValueError(f"area weights {tuple(self._area_weights.shape)} against a {(H, W)} grid")
        return self._area_weights.to(device, torch.float64).mean(dim=1)

    def _per_variable(self, acc: Dict[str, torch.Tensor], i: int):
        """-> (counts (n_slots, lat, M + 1), ties (n_slots, lat)) of variable i inside the flat (reduced) buffers."""
        M, _, H, _ = self._grids[i]
        c0, t0 = self._offsets["counts"][i], self._offsets["ties"][i]
        counts = acc["counts"][c0:c0 + self._n_slots * H * (M + 1)].view(self._n_slots, H, M + 1)
        ties = acc["ties"][t0:t0 + self._n_slots * H].view(self._n_slots, H)
        return counts, ties

    @torch.no_grad()
    def get_data(self) -> Dict[str, torch.Tensor]:
        acc = self._reduced()
        data: Dict[str, torch.Tensor] = {}
        for i, name in enumerate(self._names):
            counts, ties = self._per_variable(acc, i)
            weighted = (self._lat_weights(i, counts.device)[None, :, None] * counts).sum(dim=1)      # (n_slots, M + 1)
            data[f"counts/{name}"] = counts
            data[f"ties/{name}"] = ties
            data[f"frequency/{name}"] = weighted / weighted.sum(dim=1, keepdim=True)
        return data

    @torch.no_grad()
    def get_logs(self, label: str) -> Dict[str, float]:
        acc = self._reduced()
        parts = []
        for i in range(len(self._names)):
            counts, ties = self._per_variable(acc, i)
            w = self._lat_weights(i, counts.device)
            parts += [(w[:, None] * counts.sum(dim=0)).sum(dim=0), (w * ties.sum(dim=0)).sum().reshape(1)]
        packed = torch.cat(parts).cpu()                # every variable's weighted bins and ties in one copy
        logs: Dict[str, float] = {}
        at = 0
        for i, name in enumerate(self._names):
            M = self._grids[i][0]
            bins, tied = packed[at:at + M + 1], packed[at + M + 1]
            at += M + 2
            total = bins.sum()
            freq = bins / total
            logs[f"reliability_index/{name}"] = float((freq - 1.0 / (M + 1)).abs().sum())
            logs[f"outlier_fraction/{name}"] = float(freq[0] + freq[M])
            logs[f"tie_fraction/{name}"] = float(tied / total)
        return {f"{label}/{k}": v for k, v in logs.items()} if len(label) != 0 else logs
