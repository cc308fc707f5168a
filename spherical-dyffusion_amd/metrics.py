"""On-device ensemble diagnostics: host mirror of the reductions in `src/ace_inference/core/metrics.py`.

`ensemble_metrics(truth, predicted, weights)` returns, per (sample, time) plane, what the reference computes with
`root_mean_squared_error(truth, predicted.mean(0), weights, dim=(-2, -1))` (`metrics.py:107-132`),
`ensemble_spread(predicted, weights, dim=(-2, -1))` (`:135-144`), `spread_skill_ratio` (`:146-155`),
`weighted_crps(truth, predicted, weights, dim=(-2, -1))` (`:158-208`, fair form) and `weighted_mean_bias` (`:84-104`) of
the ensemble mean -- in ONE pass over the ensemble on the device (`sdy_ensemble_metrics`): the reference materialises the
(E, E, ...) pairwise-difference tensor for the CRPS.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Mapping, Optional, Sequence

import numpy as np
import torch

from ._lib import SdyVideoArgs, SdyZonalArgs, aligned, check, current_stream, lib, ptr
from .member_mean import EnsembleTimeMeanAggregator
from .rank_hist import RankHistogramAggregator
from .events import Events, EventVerificationAggregator
from .fss import FractionsSkillAggregator
from .spells import EventSpellAggregator
from .quantiles import TimeQuantileAggregator
from .spacetime import SpaceTimeSpectra, SpaceTimeSpectrumAggregator
from .field_scores import FieldScoreAggregator
from .regions import RegionalMeanAggregator, Regions
from .spectrum import KineticEnergySpectrumAggregator, PowerSpectrumAggregator
from .variability import TimeVariabilityAggregator
from .eddies import CovarianceGroups, EddyCovarianceAggregator
from .time_bins import BinnedTimeMeanAggregator, TimeBins
from .windows import FieldAccumulator, TorchDistributed, fill_window, whole_ics_message, window_layouts  # noqa: F401


def spherical_area_weights(lats, num_lon: int) -> torch.Tensor:
    """`metrics.py:14-29`: cos(latitude) weights of a regular lat-lon grid, normalised to sum 1; shape (num_lat, num_lon)."""
    lats = torch.as_tensor(lats)
    w = torch.cos(torch.deg2rad(lats)).repeat(num_lon, 1).t()
    return w / w.sum()


def ensemble_metrics(truth: torch.Tensor, predicted: torch.Tensor, weights: torch.Tensor) -> Dict[str, torch.Tensor]:
    """truth (..., H, W), predicted (E, ..., H, W), weights (H, W) -> dict of (...) fp64 tensors:
    rmse (of the ensemble mean), spread (with the (E+1)/E correction), spread_skill_ratio, crps (fair), bias."""
    if not predicted.is_cuda:
        raise RuntimeError("sdy_amd metrics run on the GPU only (no CPU fallback)")
    assert predicted.shape[1:] == truth.shape, f"truth {tuple(truth.shape)} vs predicted {tuple(predicted.shape)}"
    dev = predicted.device
    p = predicted.to(torch.float32).contiguous()
    t = truth.to(dev, torch.float32).contiguous()
    w = weights.to(dev, torch.float32).contiguous()
    E = p.shape[0]
    H, W = p.shape[-2:]
    assert tuple(w.shape) == (H, W)
    lead = tuple(t.shape[:-2])
    n = 1
    for s in lead:
        n *= s
    out = torch.zeros(max(n, 1), 4, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib.sdy_ensemble_metrics(ptr(p), ptr(t), ptr(w), E, max(n, 1) * H * W, max(n, 1), H * W, ptr(out),
                                       current_stream()), "sdy_ensemble_metrics")
    out = out / w.double().sum()
    rmse = out[:, 0].sqrt().reshape(lead)
    spread = out[:, 1].sqrt().reshape(lead) * ((E + 1) / E) ** 0.5
    return {"rmse": rmse, "spread": spread, "spread_skill_ratio": spread / rmse, "crps": out[:, 2].reshape(lead),
            "bias": out[:, 3].reshape(lead)}


class TimeMeanAggregator:
    """Statistics on the time-mean state: host mirror of `TimeMeanAggregator`
    (`src/ace_inference/core/aggregator/inference/time_mean.py:45-173`) minus its plots.

    Same constructor keywords that matter (`area_weights`, `dist`, `target`, `is_ensemble`), same `record_batch(loss,
    target_data, gen_data, target_data_norm, gen_data_norm, i_time_start)` (what `run_inference` calls once per window) and
    the same numbers from `get_logs(label)`: `rmse/<name>`, `bias/<name>`, `rmse/channel_mean` of the time-mean maps.  The
    maps stay on the device (`time_mean_maps()`), one HIP launch per variable and window adds a window's time means
    (`sdy_time_mean_accumulate`, strided views welcome); `get_logs` combines ranks and takes RMSE / bias with
    `sdy_ensemble_metrics`.  The matplotlib / wandb images of the reference are out of scope.

    Ranks.  The reference shards whole initial conditions over ranks and averages the ranks' maps with equal weight
    (`time_mean.py:147-148`, `Distributed.reduce_mean`).  Here a rank's share is any contiguous range of trajectories
    (`ensemble.shard`: 25 members over 8 GPUs are 4, 3, 3, ... rows), so the maps are kept as SUMS over rows of per-row time
    means next to the row count, both are summed over ranks (`dist.reduce_sum`) and divided at the end: every trajectory
    weighs the same whatever the sharding, and one process gets exactly the reference's numbers.  Generated data may be the
    member-stacked `(members, samples, time, lat, lon)` or, for a ragged share, flat `(rows, time, lat, lon)`; for a ragged
    share `run_inference` also passes `sample_weights` (the fraction of each touched initial condition's members that ran on
    this rank), which weigh the target maps the same way."""

    accepts_sample_weights = True

    def __init__(self, area_weights: torch.Tensor, dist=None, target: str = "denorm", metadata=None,
                 log_individual_channels: bool = True, is_ensemble: bool = False):
        if target not in ("norm", "denorm"):
            raise ValueError(f"target must be 'norm' or 'denorm', got {target!r}")
        self._area_weights = area_weights
        self._is_ensemble = is_ensemble
        self._target = target
        self._log_individual_channels = log_individual_channels
        self._dist = TorchDistributed() if dist is None else dist
        self._target_data: Dict[str, torch.Tensor] = {}
        self._gen_data: Dict[str, torch.Tensor] = {}
        self._target_rows = 0.0       # sum over windows of the (weighted) sample count behind the target maps
        self._gen_rows = 0.0          # ... of the trajectory count behind the generated maps
        self._n_batches = 0

    @staticmethod
    def _accumulate(maps: Dict[str, torch.Tensor], data, t0: int, ensemble: bool,
                    sample_weights: Optional[Sequence[float]] = None) -> float:
        """maps[name] += sum over rows of the row's mean over times t0..T-1 (row weights optional); returns the row count."""
        rows = 0.0
        for name, v in data.items():
            if not v.is_cuda:
                raise RuntimeError("sdy_amd aggregators run on the GPU only (no CPU fallback)")
            v = v.to(torch.float32)
            if ensemble and v.dim() == 5:
                n0, n1, T, H, W = v.shape
            else:
                assert v.dim() == 4, "data are (samples, time, lat, lon) [or (members, samples, time, lat, lon)]"
                (n1, T, H, W), n0 = v.shape, 1
            if v.stride(-1) != 1 or v.stride(-2) != W or v.stride(-3) != H * W:
                v = v.contiguous()
            v = aligned(v)                                  # float4 loads (sdy_time_mean_accumulate)
            s0, s1 = (v.stride(0), v.stride(1)) if v.dim() == 5 else (0, v.stride(0))
            if name not in maps:
                maps[name] = torch.zeros(H, W, dtype=torch.float32, device=v.device)
            with torch.cuda.device(v.device):
                if sample_weights is None:
                    check(lib.sdy_time_mean_accumulate(ptr(v), n0, s0, n1, s1, t0, T, H * W, 1.0 / (T - t0), ptr(maps[name]),
                                                       current_stream()), "sdy_time_mean_accumulate")
                    rows = float(n0 * n1)
                else:
                    assert n0 == 1 and len(sample_weights) == n1, "one weight per sample"
                    for j, wj in enumerate(sample_weights):
                        check(lib.sdy_time_mean_accumulate(ptr(v[j]), 1, 0, 1, 0, t0, T, H * W, float(wj) / (T - t0),
                                                           ptr(maps[name]), current_stream()), "sdy_time_mean_accumulate")
                    rows = float(sum(sample_weights))
        return rows

    @torch.no_grad()
    def record_batch(self, loss, target_data, gen_data, target_data_norm, gen_data_norm, i_time_start: int = 0,
                     sample_weights: Optional[Sequence[float]] = None):
        if self._target == "norm":
            target_data, gen_data = target_data_norm, gen_data_norm
        t0 = 1 if i_time_start == 0 else 0          # the very first time of a run is the initial condition
        self._target_rows += self._accumulate(self._target_data, target_data, t0, ensemble=False,
                                              sample_weights=sample_weights)
        self._gen_rows += self._accumulate(self._gen_data, gen_data, t0, ensemble=self._is_ensemble)
        self._n_batches += 1

    def time_mean_maps(self) -> Dict[str, Dict[str, torch.Tensor]]:
        """{"gen": {name: (H, W)}, "target": {...}}: time means so far over every rank's trajectories, on the device."""
        if self._n_batches == 0:
            # (raised BEFORE any collective: every rank of a job must have recorded at least one window -- a rank without a
            # share would leave the others waiting in reduce_sum; shard with ensemble.partition, which gives every rank of
            # world <= trajectories a non-empty share)
            raise ValueError("No data recorded.")

        def red(d, rows):
            if not d:
                return {}
            dev = next(iter(d.values())).device
            n = float(self._dist.reduce_sum(torch.tensor([rows], dtype=torch.float64, device=dev))[0])
            return {k: self._dist.reduce_sum(v) / n for k, v in d.items()}

        return {"gen": red(self._gen_data, self._gen_rows), "target": red(self._target_data, self._target_rows)}

    @torch.no_grad()
    def get_logs(self, label: str) -> Dict[str, float]:
        maps = self.time_mean_maps()
        logs, rmse_all = {}, {}
        for name, gen in maps["gen"].items():
            m = ensemble_metrics(maps["target"][name], gen[None], self._area_weights)     # one "member": RMSE and bias of a map
            rmse_all[name] = float(m["rmse"])
            if self._log_individual_channels:
                logs[f"rmse/{name}"] = rmse_all[name]
                logs[f"bias/{name}"] = float(m["bias"])
        logs["rmse/channel_mean"] = sum(rmse_all.values()) / len(rmse_all)
        return {f"{label}/{k}": v for k, v in logs.items()} if len(label) != 0 else logs


SERIES_METRICS = ("weighted_rmse", "weighted_bias", "weighted_mean_gen", "weighted_mean_target", "weighted_std_gen",
                  "weighted_std_target")
SERIES_METRICS_ENSEMBLE = ("weighted_crps", "weighted_ssr")
GRAD_MAG_METRIC = "weighted_grad_mag_percent_diff"


def ensemble_series(truth: torch.Tensor, predicted: torch.Tensor, weights: torch.Tensor,
                    grad_mag: bool = False) -> torch.Tensor:
    """truth (n_sample, T, H, W), predicted (members, n_sample, T, H, W) -- any strides on the two leading axes, so the window
    driver's member-stacked VIEW is read in place -- weights (H, W)  ->  (n_sample, T, 8) fp64: the area-weighted means of
    (ens. mean - truth)^2 | member variance (unbiased) | fair CRPS | ens. mean - truth | ens. mean | (ens. mean)^2 | truth |
    truth^2 per (sample, time) plane (`sdy_ensemble_series`: one pass, members in registers).

    `grad_mag=True` -> (n_sample, T, 10): the same eight, then the area-weighted mean gradient magnitude of the truth and the
    mean over members of each member's (`weighted_mean_gradient_magnitude`, `metrics.py:210-220`: torch.gradient over
    (H, W) with unit spacing, edge_order 1, longitude not periodic) -- the T and P of `gradient_magnitude_percent_diff`
    (`:223-241`), from the same pass (`sdy_ensemble_series_grad`).  H, W >= 2."""
    if not predicted.is_cuda:
        raise RuntimeError("sdy_amd metrics run on the GPU only (no CPU fallback)")
    assert predicted.dim() == 5 and predicted.shape[1:] == truth.shape, \
        f"truth {tuple(truth.shape)} vs predicted {tuple(predicted.shape)}"
    dev = predicted.device
    M, n_sample, T, H, W = predicted.shape
    p = predicted.to(torch.float32)
    if p.stride(-1) != 1 or p.stride(-2) != W or p.stride(-3) != H * W:
        p = p.contiguous()
    t = truth.to(dev, torch.float32)
    if t.stride(-1) != 1 or t.stride(-2) != W or t.stride(-3) != H * W:
        t = t.contiguous()
    w = weights.to(dev, torch.float32).contiguous()
    out = torch.zeros(n_sample, T, 10 if grad_mag else 8, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        if grad_mag:
            check(lib.sdy_ensemble_series_grad(ptr(p), M, p.stride(0), p.stride(1), ptr(t), t.stride(0), ptr(w), n_sample, T,
                                               H, W, ptr(out), current_stream()), "sdy_ensemble_series_grad")
            out[..., 9] /= M                      # sum over members -> mean over members
        else:
            check(lib.sdy_ensemble_series(ptr(p), M, p.stride(0), p.stride(1), ptr(t), t.stride(0), ptr(w), n_sample, T,
                                          H * W, ptr(out), current_stream()), "sdy_ensemble_series")
    return out / w.double().sum()


def grad_mag_percent_diff(s: torch.Tensor) -> torch.Tensor:
    """`gradient_magnitude_percent_diff` (`metrics.py:223-241`) from `ensemble_series(..., grad_mag=True)` rows:
    100 (P - T) / T per plane; a truth plane without gradient gives inf / nan, as in the reference."""
    return 100.0 * (s[..., 9] - s[..., 8]) / s[..., 8]


class MeanAggregator:
    """Per-timestep series of area-weighted metrics: host mirror of `MeanAggregator` / `AreaWeightedReducedMetric`
    (`src/ace_inference/core/aggregator/inference/reduced.py:105-266`) minus the wandb table / xarray packaging.

    Same constructor keywords that matter (`area_weights`, `target`, `n_timesteps`, `is_ensemble`, `dist`), same
    `record_batch(loss, target_data, gen_data, target_data_norm, gen_data_norm, i_time_start)`; `get_series()` returns
    `{"<metric>/<variable>": (n_timesteps,) fp64 tensor}` -- the arrays the reference puts into its table: mean over the
    windows' samples, accumulated at `i_time_start ...` and divided by the number of windows that touched a time index, then
    averaged over ranks (`dist.reduce_mean`, `reduced.py:247`).  Metrics: `weighted_rmse`, `weighted_bias` (of the ensemble
    mean), `weighted_mean_gen / _target`, `weighted_std_gen / _target`, for ensembles `weighted_crps` (fair) and
    `weighted_ssr`, and with `grad_mag_percent_diff=True` the reference's `weighted_grad_mag_percent_diff` (per plane
    100 (P - T) / T of the area-weighted mean gradient magnitudes, P the mean over members: `reduced.py:178,225-227`).
    One `sdy_ensemble_series` (`sdy_ensemble_series_grad`) launch per variable and window reads the member-stacked view in
    place; the accumulators are (n_timesteps,) fp64 tensors on the device.

    `grad_mag_percent_diff` is off by default so that the key set of the series stays what existing callers rely on; a
    drop-in caller passes `grad_mag_percent_diff=True` to get the reference's full key set.

    Ensemble metrics need every member of an initial condition on one rank (the reference's IC sharding): a ragged share
    (`run_inference(unit_range=...)` cutting through an IC's members) hands over flat rows and is refused."""

    def __init__(self, area_weights: torch.Tensor, target: str = "denorm", n_timesteps: int = 1, is_ensemble: bool = False,
                 dist=None, device=None, metadata=None, grad_mag_percent_diff: bool = False):
        if target not in ("norm", "denorm"):
            raise ValueError(f"target must be 'norm' or 'denorm', got {target!r}")
        self._area_weights = area_weights
        self._target = target
        self._n_timesteps = int(n_timesteps)
        self.is_ensemble = is_ensemble
        self._grad_mag = bool(grad_mag_percent_diff)
        self._dist = TorchDistributed() if dist is None else dist
        self._total: Dict[str, Dict[str, torch.Tensor]] = {}      # metric -> variable -> (n_timesteps,) fp64
        self._n_batches: Optional[torch.Tensor] = None            # (n_timesteps,) int32, as AreaWeightedReducedMetric

    @property
    def metric_names(self) -> List[str]:
        return list(SERIES_METRICS + (SERIES_METRICS_ENSEMBLE if self.is_ensemble else ()) +
                    ((GRAD_MAG_METRIC,) if self._grad_mag else ()))

    @torch.no_grad()
    def record_batch(self, loss, target_data, gen_data, target_data_norm, gen_data_norm, i_time_start: int = 0):
        if self._target == "norm":
            target_data, gen_data = target_data_norm, gen_data_norm
        n_time = None
        for name, gen in gen_data.items():
            if self.is_ensemble:
                if gen.dim() != 5:
                    raise ValueError(whole_ics_message("MeanAggregator(is_ensemble=True)"))
                pred = gen
            else:
                pred = gen[None]
            s = ensemble_series(target_data[name], pred, self._area_weights, grad_mag=self._grad_mag)  # (n_sample, T, 8|10)
            E = pred.shape[0]
            mse, var, crps, bias, mg, mg2, mt, mt2 = s[..., :8].unbind(dim=-1)
            rmse = mse.sqrt()
            vals = {"weighted_rmse": rmse, "weighted_bias": bias, "weighted_mean_gen": mg, "weighted_mean_target": mt,
                    "weighted_std_gen": (mg2 - mg * mg).clamp_min(0.0).sqrt(),
                    "weighted_std_target": (mt2 - mt * mt).clamp_min(0.0).sqrt()}
            if self.is_ensemble:
                vals["weighted_crps"] = crps
                vals["weighted_ssr"] = var.sqrt() * ((E + 1) / E) ** 0.5 / rmse
            if self._grad_mag:
                vals[GRAD_MAG_METRIC] = grad_mag_percent_diff(s)
            n_time = s.shape[1]
            sl = slice(i_time_start, i_time_start + n_time)
            for metric, v in vals.items():
                tot = self._total.setdefault(metric, {})
                if name not in tot:
                    tot[name] = torch.zeros(self._n_timesteps, dtype=torch.float64, device=s.device)
                tot[name][sl] += v.mean(dim=0)                                        # mean over the window's samples
            if self._n_batches is None:
                self._n_batches = torch.zeros(self._n_timesteps, dtype=torch.int32, device=s.device)
        if n_time is not None:
            self._n_batches[i_time_start:i_time_start + n_time] += 1

    @torch.no_grad()
    def get_series(self) -> Dict[str, torch.Tensor]:
        if not self._total:
            raise ValueError("No batches have been recorded.")
        return {f"{metric}/{name}": self._dist.reduce_mean(tot / self._n_batches)
                for metric, per_var in self._total.items() for name, tot in per_var.items()}

    @torch.no_grad()
    def get_logs(self, label: str):
        """`reduced.py:252-266` puts the series into one wandb table under `<label>/series`; here: the arrays themselves."""
        return {f"{label}/series": {k: v.cpu().numpy() for k, v in self.get_series().items()}}


# ---- the reference's composite (`src/ace_inference/core/aggregator/inference/main.py`) ----------------------------------
class Table:
    """The two members of `wandb.Table` the reference's log plumbing uses (`columns`, `data`, `add_data`): wandb itself is not
    a dependency of this package."""

    def __init__(self, columns: Sequence[str]):
        self.columns = list(columns)
        self.data: List[list] = []

    def add_data(self, *row):
        if len(row) != len(self.columns):
            raise ValueError(f"expected {len(self.columns)} values, got {len(row)}")
        self.data.append(list(row))


def data_to_table(data: Mapping[str, Sequence[float]]) -> Table:
    """`reduced.py:282-293`: 1-D series -> one table with a `forecast_step` column and the keys in sorted order."""
    keys = sorted(data.keys())
    table = Table(["forecast_step"] + keys)
    for i in range(len(data[keys[0]])):
        table.add_data(i, *[data[k][i] for k in keys])
    return table


def to_inference_logs(log: Mapping[str, object]) -> List[Dict[str, float]]:
    """`main.py:189-211`: a dict holding tables and scalars -> one dict per table row (the wandb step is the forecast step),
    columns renamed `<key without its last component>/<column>`; scalars go into the last row's dict."""
    n_rows = max([len(v.data) for v in log.values() if isinstance(v, Table)], default=0)
    logs: List[Dict[str, float]] = [{} for _ in range(n_rows)]
    for key, val in log.items():
        if isinstance(val, Table):
            stem = key[: key.rfind("/")]
            for i, row in enumerate(val.data):
                for j, col in enumerate(val.columns):
                    logs[i][f"{stem}/{col}"] = row[j]
        else:
            logs[-1][key] = val
    return logs


class OneStepMeanAggregator:
    """Metrics of ONE forecast step averaged over the windows that contain it (`one_step/reduced.py:35-147`, the reference's
    `mean_step_20`): `weighted_rmse`, `weighted_bias` (of the ensemble mean), `weighted_mean_gen`, for ensembles
    `weighted_crps` and `weighted_ssr`, with `grad_mag_percent_diff=True` the reference's `weighted_grad_mag_percent_diff`
    (`one_step/reduced.py:75,121-123`; off by default, as in `MeanAggregator`), and the mean of the `loss` values handed to
    `record_batch`."""

    def __init__(self, area_weights: torch.Tensor, target_time: int = 1, is_ensemble: bool = False, dist=None, device=None,
                 grad_mag_percent_diff: bool = False):
        self._area_weights = area_weights
        self._target_time = int(target_time)
        self.is_ensemble = is_ensemble
        self._grad_mag = bool(grad_mag_percent_diff)
        self._dist = TorchDistributed() if dist is None else dist
        self._loss = 0.0
        self._n_batches = 0
        self._total: Dict[str, Dict[str, torch.Tensor]] = {}

    @property
    def metric_names(self) -> List[str]:
        return list(("weighted_rmse", "weighted_bias", "weighted_mean_gen") +
                    (SERIES_METRICS_ENSEMBLE if self.is_ensemble else ()) + ((GRAD_MAG_METRIC,) if self._grad_mag else ()))

    @torch.no_grad()
    def record_batch(self, loss, target_data, gen_data, target_data_norm, gen_data_norm, i_time_start: int = 0):
        self._loss = self._loss + loss        # (added for every window, as the reference does: reduced.py:103)
        t = self._target_time - i_time_start
        any_gen = next(iter(gen_data.values()))
        if t < 0 or t >= any_gen.shape[2 if self.is_ensemble else 1]:
            return
        for name, gen in gen_data.items():
            pred = gen if self.is_ensemble else gen[None]
            s = ensemble_series(target_data[name][:, t:t + 1], pred[:, :, t:t + 1], self._area_weights,
                                grad_mag=self._grad_mag)[:, 0]                                         # (n_sample, 8|10)
            E = pred.shape[0]
            mse, var, crps, bias, mg = s[:, 0], s[:, 1], s[:, 2], s[:, 3], s[:, 4]
            vals = {"weighted_rmse": mse.sqrt(), "weighted_bias": bias, "weighted_mean_gen": mg}
            if self.is_ensemble:
                vals["weighted_crps"] = crps
                vals["weighted_ssr"] = var.sqrt() * ((E + 1) / E) ** 0.5 / mse.sqrt()
            if self._grad_mag:
                vals[GRAD_MAG_METRIC] = grad_mag_percent_diff(s)
            for metric, v in vals.items():
                per_var = self._total.setdefault(metric, {})
                per_var[name] = per_var.get(name, 0.0) + v.mean()
        self._n_batches += 1

    @torch.no_grad()
    def get_logs(self, label: str) -> Dict[str, float]:
        if self._n_batches == 0:
            raise ValueError("No batches have been recorded.")
        dev = self._area_weights.device
        logs = {f"{label}/loss": torch.as_tensor(self._loss, dtype=torch.float64, device=dev) / self._n_batches}
        for metric, per_var in self._total.items():
            for name, tot in per_var.items():
                logs[f"{label}/{metric}/{name}"] = tot.double() / self._n_batches
        return {k: float(self._dist.reduce_mean(logs[k].reshape(1))[0]) for k in sorted(logs)}


class VideoAggregator(FieldAccumulator):
    """Videos of state evolution: device mirror of `VideoAggregator`
    (`src/ace_inference/core/aggregator/inference/video.py`) minus the wandb rendering.

    Same constructor keywords (`n_timesteps`, `enable_extended_videos`, `dist`, `metadata`) plus `max_bytes`, same
    `record_batch`.  A window is never copied to the host (the reference moves every tensor with `.cpu()`): one
    `sdy_video_accumulate` launch per run of same-shaped variables adds the window to float64 accumulators
    `(n_timesteps, lat, lon)` on the device -- per variable the mean of gen and target, and with `enable_extended_videos` the
    mean squares, the unbiased variance of the error over the rows and the error's extremes.  `get_data()` returns the
    reference's `_get_data(label="")` as float64 device tensors `(n_timesteps, lat, lon)`: `<name>` is a pair
    `{"gen", "target"}`; extended: `bias/<name>`, `rmse/<name>` = sqrt(err_var / n_batches), `min_err/<name>`,
    `max_err/<name>`, `gen_var/<name>` = (E[g^2] - E[g]^2) / (E[t^2] - E[t]^2).  `get_dataset()` gives the same as numpy
    arrays under the reference's dataset keys (`/` -> `_`; the pair stacked `(source, timestep, lat, lon)`, gen first).
    `get_logs` returns {}.

    The accumulators are allocated on the first batch, after comparing statistics x variables x n_timesteps x lat x lon x 8
    bytes with `max_bytes` (default: a quarter of the device's memory): videos are a short-run diagnostic.

    Ensembles.  The reference's class cannot take member-stacked data (its buffers come out `(n_timesteps, time, lat, lon)`
    for 5-D input), so the rule is this library's own: a `(members, samples, time, lat, lon)` gen is POOLED over members x
    samples, as the histogram writer pools it, and the error of row (member, sample) is taken against target row `sample` --
    what the reference computes from flat `(members * samples, ...)` gen and the target repeated per member.

    Ranks: the reference's equal-weight `dist.reduce_mean` (`reduce_min` / `reduce_max` for the extremes); ragged shares with
    `sample_weights` are out of scope."""

    def __init__(self, n_timesteps: int, enable_extended_videos: bool, dist=None, metadata=None,
                 max_bytes: Optional[int] = None):
        super().__init__(n_timesteps, dist=dist, metadata=metadata, max_bytes=max_bytes)
        self._extended = bool(enable_extended_videos)

    def _statistics(self) -> Dict[str, float]:
        stats = {"gen_mean": 0.0, "target_mean": 0.0}
        if self._extended:
            stats.update(gen_sq=0.0, target_sq=0.0, err_var=0.0, err_min=float("inf"), err_max=float("-inf"))
        return stats

    def _elements(self, stat: str, job: tuple) -> int:
        _, H, W = job
        return self._n_timesteps * H * W

    def _launch(self, lay, first: int, last: int, t_start: int) -> None:
        a = SdyVideoArgs()
        fill_window(a.win, lay, first, last)
        a.HW, a.t_start, a.n_timesteps = lay[first].H * lay[first].W, t_start, self._n_timesteps
        for stat in self._acc:
            setattr(a, stat, self._at(stat, first))
        check(lib.sdy_video_accumulate(C.byref(a), current_stream()), "sdy_video_accumulate")

    @torch.no_grad()
    def record_batch(self, loss, target_data, gen_data, target_data_norm=None, gen_data_norm=None, i_time_start: int = 0):
        del loss, target_data_norm, gen_data_norm
        self._record(target_data, gen_data, i_time_start)

    @torch.no_grad()
    def get_data(self) -> Dict[str, object]:
        n = self._counts()[:, None, None]
        red = self._dist.reduce_mean
        data: Dict[str, object] = {}
        for i, name in enumerate(self._names):
            shape = (self._n_timesteps,) + self._grids[i][1:]
            gen, target = red(self._view("gen_mean", i, *shape) / n), red(self._view("target_mean", i, *shape) / n)
            data[name] = {"gen": gen, "target": target}
            if self._extended:
                data[f"bias/{name}"] = gen - target
        if self._extended:
            for stat, label in (("err_var", "rmse"), ("err_min", "min_err"), ("err_max", "max_err")):
                for i, name in enumerate(self._names):
                    x = self._view(stat, i, self._n_timesteps, *self._grids[i][1:])
                    data[f"{label}/{name}"] = (torch.sqrt(red(x / n)) if stat == "err_var" else
                                               self._dist.reduce_min(x) if stat == "err_min" else self._dist.reduce_max(x))
            for i, name in enumerate(self._names):
                shape = (self._n_timesteps,) + self._grids[i][1:]
                var = {}
                for src in ("gen", "target"):
                    mean = red(self._view(f"{src}_mean", i, *shape) / n)
                    var[src] = red(self._view(f"{src}_sq", i, *shape) / n) - mean ** 2
                data[f"gen_var/{name}"] = var["gen"] / var["target"]
        return data

    @torch.no_grad()
    def get_dataset(self) -> Dict[str, np.ndarray]:
        out = {}
        for label, d in self.get_data().items():
            key = label.replace("/", "_")
            if isinstance(d, Mapping):
                out[key] = np.stack([d["gen"].cpu().numpy(), d["target"].cpu().numpy()], axis=0)
            else:
                out[key] = d.cpu().numpy()
        return out


class ZonalMeanAggregator(FieldAccumulator):
    """Zonal means as a function of latitude and time (hovmollers): device mirror of `ZonalMeanAggregator`
    (`src/ace_inference/core/aggregator/inference/zonal_mean.py`) minus the wandb images.

    Same constructor keywords plus `max_bytes`, same `record_batch`; one `sdy_zonal_accumulate` launch per run of same-shaped
    variables adds a window's longitude means to float64 accumulators `(samples, n_timesteps, lat)` (the reference sums in
    fp32).  `get_data()` returns `{"gen/<name>", "error/<name>"}`, each a float64 device tensor `(n_timesteps, lat)`: the
    sample mean of `acc / n_batches`, error = gen - target.  These are the arrays the reference turns into images; its
    transpose-and-flip for the picture (`data.t().flip(dims=[0])`) is NOT applied.  `get_logs` returns {}.

    Ensembles: the reference drops this aggregator for ensembles, so the rule is this library's own -- the zonal mean of a
    `(members, samples, time, lat, lon)` gen is the member mean, per sample.  Ranks: the reference's equal-weight
    `dist.reduce_mean`; ragged shares with `sample_weights` are out of scope."""

    def __init__(self, n_timesteps: int, dist=None, metadata=None, max_bytes: Optional[int] = None):
        super().__init__(n_timesteps, dist=dist, metadata=metadata, max_bytes=max_bytes)

    def _statistics(self) -> Dict[str, float]:
        return {"gen_acc": 0.0, "target_acc": 0.0}

    def _elements(self, stat: str, job: tuple) -> int:
        n1, H, _ = job
        return n1 * self._n_timesteps * H

    def _launch(self, lay, first: int, last: int, t_start: int) -> None:
        a = SdyZonalArgs()
        fill_window(a.win, lay, first, last)
        a.H, a.W, a.t_start, a.n_timesteps = lay[first].H, lay[first].W, t_start, self._n_timesteps
        for stat in self._acc:
            setattr(a, stat, self._at(stat, first))
        check(lib.sdy_zonal_accumulate(C.byref(a), current_stream()), "sdy_zonal_accumulate")

    @torch.no_grad()
    def record_batch(self, loss, target_data, gen_data, target_data_norm=None, gen_data_norm=None, i_time_start: int = 0):
        del loss, target_data_norm, gen_data_norm
        self._record(target_data, gen_data, i_time_start)

    @torch.no_grad()
    def get_data(self) -> Dict[str, torch.Tensor]:
        n = self._counts()[None, :, None]
        data = {}
        for i, name in enumerate(self._names):
            n1, H, _ = self._grids[i]
            gen = self._view("gen_acc", i, n1, self._n_timesteps, H)
            target = self._view("target_acc", i, n1, self._n_timesteps, H)
            data[f"gen/{name}"] = self._dist.reduce_mean(gen / n).mean(dim=0)
            data[f"error/{name}"] = self._dist.reduce_mean((gen - target) / n).mean(dim=0)
        return data


class InferenceAggregator:
    """The aggregator `run_inference` is handed by the reference's entry point (`inference/inference.py:247-262`): `mean`
    (per-step series, denormalised), `mean_norm` (normalised), `time_mean`, and `mean_step_20` when asked for, behind ONE
    `record_batch` / `get_logs` / `get_inference_logs` (`aggregator/inference/main.py:42-168`).  Same constructor keywords;
    `sigma_coordinates` and `metadata` are accepted and unused (they feed derived variables and image captions).  The
    image products of the reference -- snapshots, videos, zonal-mean hovmollers, the time-mean maps as pictures -- are out of
    scope: `log_video` / `log_zonal_mean_images` raise, snapshots are not produced;
    `get_time_mean_maps()` returns what `get_datasets(["time_mean"])` would hold, as device tensors.

    `grad_mag_percent_diff=True` adds the reference's `weighted_grad_mag_percent_diff/<var>` to `mean`, `mean_norm` and
    `mean_step_20`.  It is off by default: the default key set of the logs stays what existing callers rely on, and a
    drop-in caller of the reference passes `grad_mag_percent_diff=True` to get the reference's full key set.

    `video_data=True` (`extended_video_data=True` for the extended statistics too) and `zonal_mean_data=True` add the
    `video` / `zonal_mean` aggregators (`VideoAggregator`, `ZonalMeanAggregator`): the numbers behind the reference's videos
    and hovmollers, accumulated on the device and read with `get_video_data()` / `get_zonal_mean_data()`.  They add no log
    keys, and `log_video` / `enable_extended_videos` / `log_zonal_mean_images` (the rendered products) keep raising.

    `power_spectrum_data=True` adds `power_spectrum` (`sdy_amd.spectrum.PowerSpectrumAggregator` on the grid `spectrum_grid`):
    per-degree power of gen, target and error per lead time, read with `get_power_spectrum_data()`; no log keys either.
    `wind_pairs=<mapping label -> (u_name, v_name)>` (`sdy_amd.spectrum.wind_pairs(names)` builds it) adds `kinetic_energy`
    (`sdy_amd.KineticEnergySpectrumAggregator` on the same grid): the rotational and divergent kinetic-energy spectra of gen,
    target and error winds per lead time, read with `get_kinetic_energy_data()`; no log keys.  The default `None` adds nothing.

    `ensemble_time_mean_data=True` adds `time_mean_ensemble` (`sdy_amd.EnsembleTimeMeanAggregator`): one time-mean map per
    member and the statistics the reference's full-rollout evaluation takes of them (`rmse_member_avg`, `bias_member_avg`,
    `rmse`, `bias`, `crps` per variable; with `ensemble_time_mean_spread=True` also `spread` and `ssr`), under
    `<label>/time_mean_ensemble/...`; the maps are read with `get_ensemble_time_mean_maps()`.  Off by default: the default
    key set of the logs does not change.

    `rank_histogram_data=True` adds `rank_histogram` (`sdy_amd.RankHistogramAggregator`): per variable, lead time and latitude
    the counts of the truth's rank among the members (`rank_histogram_pool_times=True`: one slot for all lead times), read
    with `get_rank_histogram_data()`, and `reliability_index`, `outlier_fraction` and `tie_fraction` per variable under
    `<label>/rank_histogram/...`.  Off by default as well; meaningful with more than one member (one member: two bins).

    `time_variability_data=True` adds `time_variability` (`sdy_amd.TimeVariabilityAggregator`): per member and for the target
    the standard deviation along time and the lag-1 autocorrelation at every grid point, read with
    `get_time_variability_data()`, and `time_std_gen`, `time_std_target`, `time_std_ratio`, `time_std_rmse`, `lag1_gen`,
    `lag1_target`, `lag1_bias` and `lag1_defined_fraction` per variable under `<label>/time_variability/...`.  Off by default as
    well; its windows must arrive in run order.

    `regions=<sdy_amd.Regions>` adds `mean_regional` (`sdy_amd.RegionalMeanAggregator` on the denormalised data): the series of
    `mean` once per region, `<metric>/<region>/<variable>`, as one more table under `<label>/mean_regional/series`; read with
    `get_regional_series()`.  A grid point whose weight in a region is 0 contributes nothing to it, NaN values included.  The
    default `None` adds nothing: the default key set of the logs does not change.

    `events=<sdy_amd.Events>` adds `events` (`sdy_amd.EventVerificationAggregator` on the denormalised data;
    `event_pool_times=True`: one slot for all lead times, `event_frequency_maps=True`: exceedance-frequency maps too): per
    variable and event the table of counts behind Brier score, reliability diagram and ROC curve, read with
    `get_event_data()`, and `brier_score`, `brier_skill_score`, `brier_reliability`, `brier_resolution`, `base_rate`,
    `forecast_rate` and `roc_area` under `<label>/events/<metric>/<event>/<variable>`.  The default `None` adds nothing.
    With events, `event_neighbourhoods=<tuple of radii in grid points>` adds `fss` (`sdy_amd.FractionsSkillAggregator` on the same
    events, with `event_pool_times`): the neighbourhood sums read with `get_fss_data()`, and `fss`, `fbs`, `base_rate`,
    `fss_useful` and `counted_fraction` under `<label>/fss/<metric>_r<radius>/<event>/<variable>`.  The default `None` adds
    nothing.

    `field_scores=True` adds `field_scores` (`sdy_amd.FieldScoreAggregator` on the denormalised data; `climatology=<mapping from
    variable to a (lat, lon) tensor>` turns that variable's pattern correlation into an anomaly correlation): the energy score,
    the member-to-truth and member-to-member distances of whole fields, their ratio, the ensemble-mean RMSE and the
    correlation per lead time, `<metric>/<variable>`, as one more table under `<label>/field_scores/series`; read with
    `get_field_scores()`.  The default `False` adds nothing: the default key set of the logs does not change.

    With events, `event_spells=True` adds `spells` (`sdy_amd.EventSpellAggregator` on the same events): per trajectory and grid
    point the longest spell, the spells and the times in each event, and per latitude the histogram of spell durations, read
    with `get_spell_data()`, and `mean_duration_gen`, `mean_duration_target`, `mean_duration_ratio`, `longest_gen`,
    `longest_target`, `longest_bias`, `onset_rate_gen`, `onset_rate_target`, `time_fraction_gen` and `time_fraction_target` under
    `<label>/spells/<metric>/<event>/<variable>`.  Without events it raises `ValueError`; its windows must arrive in run order.
    The default `False` adds nothing.

    `time_quantiles=<sequence of q in [0, 1]>` adds `time_quantiles` (`sdy_amd.TimeQuantileAggregator` on the denormalised data
    of `time_quantile_variables`, `None`: every generated variable): per grid point the quantiles along time of gen (members
    pooled) and of the target, read with `get_time_quantile_data()`, and `quantile_gen`, `quantile_bias`, `quantile_rmse`,
    `quantile_target` and `defined_fraction` under `<label>/time_quantiles/<metric>/q<q>/<variable>`.  It keeps every counted
    time of every trajectory (4 bytes each): name the variables.  The default `None` adds nothing.

    `space_time_spectra=<sdy_amd.SpaceTimeSpectra>` adds `space_time_spectra` (`sdy_amd.SpaceTimeSpectrumAggregator` on the
    denormalised data of the specification's variables): the wavenumber-frequency power of gen (members pooled) and of the
    target in an equatorial band, symmetric and antisymmetric about the equator, read with `get_space_time_spectrum_data()`,
    and `power_gen`, `power_target` and `power_ratio` per band (and `east_west_ratio_gen` / `east_west_ratio_target`) under
    `<label>/space_time_spectra/...`.  Its windows must arrive in run order.  The default `None` adds nothing: the default key
    set of the logs does not change.

    `eddy_covariances=<sdy_amd.CovarianceGroups>` adds `eddy_covariance` (`sdy_amd.EddyCovarianceAggregator` on the
    denormalised data of the groups' variables): per member and for the target the covariance and the correlation along time
    of every pair of a group's variables at every grid point -- u'v', v'T', v'q', the eddy kinetic energy -- read with
    `get_eddy_covariance_data(label, a, b)`, and `cov_gen`, `cov_target`, `cov_bias`, `cov_rmse`, `corr_gen`, `corr_target`,
    `corr_bias` and `corr_defined_fraction` per group and pair, `time_variance_gen` / `time_variance_target` per group and
    variable and `eke_gen`, `eke_target`, `eke_ratio` per group with winds under `<label>/eddy_covariance/...`.  Its windows
    must arrive in run order.  The default `None` adds nothing: the default key set of the logs does not change.

    `time_bins=<sdy_amd.TimeBins>` adds `time_bins` (`sdy_amd.BinnedTimeMeanAggregator` on the denormalised data of
    `time_bin_variables`, `None`: every generated variable): per bin of the run's times -- months, seasons, years, hours of the
    day -- one time-mean map per member (`time_bin_per_member=False`: one for the pooled members) and the target's, with
    `time_bin_extremes=True` the bin's maximum and minimum too, read with `get_time_bin_data()`, and `rmse`, `bias`,
    `rmse_member_avg`, `bias_member_avg` and `crps` per bin and variable, `bin_range_gen` / `_target` / `_ratio`, `bin_std_gen` /
    `_target` / `_ratio` and `centred_rmse` per variable under `<label>/time_bins/...`.  Per-member maps of every bin are large
    (one bin of 25 members x 63 variables x 180 x 360: 0.85 GB): name the variables.  Its windows must not go back in time.  The
    default `None` adds nothing: the default key set of the logs does not change."""

    accepts_sample_weights = True

    def __init__(self, area_weights: torch.Tensor, sigma_coordinates=None, n_timesteps: Optional[int] = None,
                 n_ensemble_members: int = 1, record_step_20: bool = False, log_video: bool = False,
                 enable_extended_videos: bool = False, log_zonal_mean_images: bool = False, dist=None, metadata=None,
                 device=None, grad_mag_percent_diff: bool = False, video_data: bool = False,
                 extended_video_data: bool = False, zonal_mean_data: bool = False, power_spectrum_data: bool = False,
                 spectrum_grid: str = "equiangular", ensemble_time_mean_data: bool = False,
                 ensemble_time_mean_spread: bool = False, rank_histogram_data: bool = False,
                 rank_histogram_pool_times: bool = False, time_variability_data: bool = False,
                 regions: Optional[Regions] = None, events: Optional[Events] = None, event_pool_times: bool = False,
                 event_frequency_maps: bool = False, field_scores: bool = False, climatology=None,
                 event_neighbourhoods: Optional[Sequence[int]] = None, wind_pairs=None,
                 space_time_spectra: Optional[SpaceTimeSpectra] = None,
                 eddy_covariances: Optional[CovarianceGroups] = None, time_bins: Optional[TimeBins] = None,
                 time_bin_variables: Optional[Sequence[str]] = None, time_bin_extremes: bool = False,
                 time_bin_per_member: bool = True, event_spells: bool = False,
                 time_quantiles: Optional[Sequence[float]] = None,
                 time_quantile_variables: Optional[Sequence[str]] = None):
        if log_video or enable_extended_videos or log_zonal_mean_images:
            raise NotImplementedError("video / zonal-mean image logging is out of scope of sdy_amd (DESIGN.md section 8)")
        if n_timesteps is None:
            raise ValueError("n_timesteps (forward steps + 1) is needed for the per-step series")
        self._is_ensemble = n_ensemble_members > 1
        if device is not None:
            area_weights = area_weights.to(device)
        kw = dict(area_weights=area_weights, dist=dist, is_ensemble=self._is_ensemble,
                  grad_mag_percent_diff=grad_mag_percent_diff)
        self._aggregators = {
            "mean": MeanAggregator(target="denorm", n_timesteps=n_timesteps, **kw),
            "mean_norm": MeanAggregator(target="norm", n_timesteps=n_timesteps, **kw),
            "time_mean": TimeMeanAggregator(area_weights, dist=dist, is_ensemble=self._is_ensemble),
        }
        if record_step_20:
            self._aggregators["mean_step_20"] = OneStepMeanAggregator(target_time=20, **kw)
        if video_data or extended_video_data:
            self._aggregators["video"] = VideoAggregator(n_timesteps=n_timesteps, enable_extended_videos=extended_video_data,
                                                         dist=dist, metadata=metadata)
        if zonal_mean_data:
            self._aggregators["zonal_mean"] = ZonalMeanAggregator(n_timesteps=n_timesteps, dist=dist, metadata=metadata)
        if power_spectrum_data:
            self._aggregators["power_spectrum"] = PowerSpectrumAggregator(n_timesteps=n_timesteps, grid=spectrum_grid,
                                                                          dist=dist, metadata=metadata)
        if wind_pairs is not None:
            self._aggregators["kinetic_energy"] = KineticEnergySpectrumAggregator(
                wind_pairs, n_timesteps=n_timesteps, grid=spectrum_grid, dist=dist, metadata=metadata)
        if ensemble_time_mean_data or ensemble_time_mean_spread:
            self._aggregators["time_mean_ensemble"] = EnsembleTimeMeanAggregator(
                area_weights, dist=dist, metadata=metadata, spread=ensemble_time_mean_spread)
        if rank_histogram_data:
            self._aggregators["rank_histogram"] = RankHistogramAggregator(
                area_weights, n_timesteps=n_timesteps, pool_times=rank_histogram_pool_times, dist=dist, metadata=metadata)
        if time_variability_data:
            self._aggregators["time_variability"] = TimeVariabilityAggregator(area_weights, dist=dist, metadata=metadata)
        if regions is not None:
            self._aggregators["mean_regional"] = RegionalMeanAggregator(regions, target="denorm", n_timesteps=n_timesteps,
                                                                        is_ensemble=self._is_ensemble, dist=dist)
        if events is not None:
            self._aggregators["events"] = EventVerificationAggregator(
                events, area_weights, n_timesteps=n_timesteps, pool_times=event_pool_times,
                frequency_maps=event_frequency_maps, dist=dist, metadata=metadata)
        if event_neighbourhoods is not None:
            if events is None:
                raise ValueError("event_neighbourhoods needs events=<sdy_amd.Events>")
            self._aggregators["fss"] = FractionsSkillAggregator(
                events, tuple(event_neighbourhoods), area_weights, n_timesteps=n_timesteps, pool_times=event_pool_times,
                dist=dist, metadata=metadata)
        if field_scores:
            self._aggregators["field_scores"] = FieldScoreAggregator(
                area_weights, n_timesteps=n_timesteps, is_ensemble=self._is_ensemble, climatology=climatology,
                target="denorm", dist=dist)
        if event_spells:
            if events is None:
                raise ValueError("event_spells needs events=<sdy_amd.Events>")
            self._aggregators["spells"] = EventSpellAggregator(events, area_weights, n_timesteps=n_timesteps, dist=dist,
                                                               metadata=metadata)
        if time_quantiles is not None:
            self._aggregators["time_quantiles"] = TimeQuantileAggregator(
                time_quantiles, area_weights, n_timesteps=n_timesteps, variables=time_quantile_variables, target="denorm",
                dist=dist, metadata=metadata)
        if space_time_spectra is not None:
            self._aggregators["space_time_spectra"] = SpaceTimeSpectrumAggregator(space_time_spectra, dist=dist,
                                                                                  target="denorm", metadata=metadata)
        if eddy_covariances is not None:
            self._aggregators["eddy_covariance"] = EddyCovarianceAggregator(eddy_covariances, area_weights, dist=dist,
                                                                            target="denorm", metadata=metadata)
        if time_bins is not None:
            self._aggregators["time_bins"] = BinnedTimeMeanAggregator(
                time_bins, area_weights, variables=time_bin_variables, per_member=time_bin_per_member,
                extremes=time_bin_extremes, target="denorm", dist=dist, metadata=metadata)

    @torch.no_grad()
    def record_batch(self, loss, target_data, gen_data, target_data_norm, gen_data_norm, i_time_start: int = 0,
                     sample_weights: Optional[Sequence[float]] = None):
        if len(target_data) == 0:
            raise ValueError("No data in target_data")
        if len(gen_data) == 0:
            raise ValueError("No data in gen_data")
        for agg in self._aggregators.values():
            kw = {"sample_weights": sample_weights} if getattr(agg, "accepts_sample_weights", False) else {}
            agg.record_batch(loss=loss, target_data=target_data, gen_data=gen_data, target_data_norm=target_data_norm,
                             gen_data_norm=gen_data_norm, i_time_start=i_time_start, **kw)

    @torch.no_grad()
    def get_logs(self, label: str) -> Dict[str, object]:
        logs: Dict[str, object] = {}
        for name, agg in self._aggregators.items():
            for key, val in agg.get_logs(label=name).items():
                logs[key] = data_to_table(val) if isinstance(val, Mapping) else val     # a series -> the reference's table
        return {f"{label}/{key}": val for key, val in logs.items()}

    @torch.no_grad()
    def get_inference_logs(self, label: str) -> List[Dict[str, float]]:
        return to_inference_logs(self.get_logs(label=label))

    def get_time_mean_maps(self):
        return self._aggregators["time_mean"].time_mean_maps()

    def get_video_data(self):
        """`VideoAggregator.get_data()` of the run (`video_data=True` / `extended_video_data=True`)."""
        return self._aggregators["video"].get_data()

    def get_zonal_mean_data(self):
        """`ZonalMeanAggregator.get_data()` of the run (`zonal_mean_data=True`)."""
        return self._aggregators["zonal_mean"].get_data()

    def get_ensemble_time_mean_maps(self):
        """`EnsembleTimeMeanAggregator.time_mean_maps()` of the run (`ensemble_time_mean_data=True`)."""
        return self._aggregators["time_mean_ensemble"].time_mean_maps()

    def get_rank_histogram_data(self):
        """`RankHistogramAggregator.get_data()` of the run (`rank_histogram_data=True`)."""
        return self._aggregators["rank_histogram"].get_data()

    def get_time_variability_data(self):
        """`TimeVariabilityAggregator.get_data()` of the run (`time_variability_data=True`)."""
        return self._aggregators["time_variability"].get_data()

    def get_event_data(self):
        """`EventVerificationAggregator.get_data()` of the run (`events=...`)."""
        return self._aggregators["events"].get_data()

    def get_fss_data(self):
        """`FractionsSkillAggregator.get_data()` of the run (`events=..., event_neighbourhoods=...`)."""
        return self._aggregators["fss"].get_data()

    def get_spell_data(self):
        """`EventSpellAggregator.get_data()` of the run (`events=..., event_spells=True`)."""
        return self._aggregators["spells"].get_data()

    def get_time_quantile_data(self):
        """`TimeQuantileAggregator.get_data()` of the run (`time_quantiles=...`)."""
        return self._aggregators["time_quantiles"].get_data()

    def get_space_time_spectrum_data(self):
        """`SpaceTimeSpectrumAggregator.get_data()` of the run (`space_time_spectra=...`)."""
        return self._aggregators["space_time_spectra"].get_data()

    def get_eddy_covariance_data(self, label: str, a: str, b: str):
        """`EddyCovarianceAggregator.get_pair_data(label, a, b)` of the run (`eddy_covariances=...`)."""
        return self._aggregators["eddy_covariance"].get_pair_data(label, a, b)

    def get_time_bin_data(self):
        """`{"counts", "means", "extremes"}` of the run's `BinnedTimeMeanAggregator` (`time_bins=...`): `counts()`,
        `get_bin_means()` and, with `time_bin_extremes=True`, `get_extremes()` (else None)."""
        agg = self._aggregators["time_bins"]
        return {"counts": agg.counts(), "means": agg.get_bin_means(),
                "extremes": agg.get_extremes() if agg._extremes else None}

    def get_field_scores(self):
        """`FieldScoreAggregator.get_series()` of the run (`field_scores=True`)."""
        return self._aggregators["field_scores"].get_series()

    def get_regional_series(self):
        """`RegionalMeanAggregator.get_series()` of the run (`regions=...`)."""
        return self._aggregators["mean_regional"].get_series()

    def get_kinetic_energy_data(self):
        """`KineticEnergySpectrumAggregator.get_data()` of the run (`wind_pairs=...`)."""
        return self._aggregators["kinetic_energy"].get_data()

    def get_power_spectrum_data(self):
        """`PowerSpectrumAggregator.get_data()` of the run (`power_spectrum_data=True`)."""
        return self._aggregators["power_spectrum"].get_data()
