"""Regional area-weighted metric series, on the device: `MeanAggregator`'s metrics once per region (tropics against
extratropics, land against ocean, the Nino 3.4 box) from ONE `sdy_region_series` launch per window -- all variables and all
regions, the window read once (include/sdy_amd.h, csrc/region_series.h).  No counterpart in the reference, whose aggregators
are global; a region here is what its `MeanAggregator` gives with `area_weights = area * fraction`.

Zero-weight rule: a grid point whose weight in a region is exactly 0 contributes nothing to that region, whatever its values,
NaN included (deliberately not IEEE's 0 * NaN = NaN, and not the reference's behaviour): an ocean-only field with NaN over
land gives finite numbers for a region that is zero over land.  Anywhere else a NaN propagates.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import SDY_REGION_MAX, SDY_REGION_MAX_MEMBERS, SdyRegionSeriesArgs, check, current_stream, lib, ptr
from .windows import TorchDistributed, fill_window, runs, whole_ics_message, window_layouts

SERIES_METRICS = ("weighted_rmse", "weighted_bias", "weighted_mean_gen", "weighted_mean_target", "weighted_std_gen",
                  "weighted_std_target")
SERIES_METRICS_ENSEMBLE = ("weighted_crps", "weighted_ssr")


def _host_f64(x) -> np.ndarray:
    """A tensor, an array or a sequence as a float64 numpy array on the host."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x).astype(np.float64)


class Regions:
    """Named weight maps of one lat-lon grid, in insertion order.  `lats` (H,) and `lons` (W,) are the cell centres in
    degrees, `area_weights` (H, W) the area weights of the global metrics.  A region's map is `area_weights * fraction`,
    formed in float64 and rounded once to fp32 (what the kernel reads); `fraction` in [0, 1] is the part of a cell that
    belongs to the region.  At most `SDY_REGION_MAX` regions.

    `ValueError`: a region whose weights sum to 0, a negative or non-finite weight, a duplicate name, a name containing "/"
    (names become part of the series keys), one region too many.

    Zero-weight rule: a point where a region's weight is exactly 0 contributes nothing to it, NaN values included."""

    def __init__(self, lats, lons, area_weights):
        self._lats = _host_f64(lats).reshape(-1)
        self._lons = _host_f64(lons).reshape(-1)
        self._area = _host_f64(area_weights)
        if self._area.shape != (self._lats.size, self._lons.size):
            raise ValueError(f"area weights {self._area.shape} against {self._lats.size} latitudes x {self._lons.size} longitudes")
        self._maps: Dict[str, np.ndarray] = {}                    # name -> (H, W) float32
        self._device_cache: Dict[torch.device, Tuple[int, torch.Tensor, torch.Tensor]] = {}

    # -- the set ---------------------------------------------------------------------------------------------------------
    @property
    def names(self) -> List[str]:
        return list(self._maps)

    @property
    def shape(self) -> Tuple[int, int]:
        return self._area.shape

    def __len__(self) -> int:
        return len(self._maps)

    def weight_map(self, name: str) -> torch.Tensor:
        """The region's (H, W) fp32 map (a copy, on the host)."""
        return torch.from_numpy(self._maps[name].copy())

    def add_fraction(self, name: str, fraction) -> "Regions":
        """`fraction` (H, W) in [0, 1], or a bool mask."""
        f = _host_f64(fraction)
        if f.shape != self._area.shape:
            raise ValueError(f"region {name!r}: fraction {f.shape} against a {self._area.shape} grid")
        if not isinstance(name, str) or not name or "/" in name:
            raise ValueError(f"region name {name!r}: a non-empty string without '/'")
        if name in self._maps:
            raise ValueError(f"region {name!r} is already defined")
        if len(self._maps) >= SDY_REGION_MAX:
            raise ValueError(f"at most {SDY_REGION_MAX} regions")
        if not np.isfinite(f).all() or (f < 0.0).any() or (f > 1.0).any():
            raise ValueError(f"region {name!r}: fractions must lie in [0, 1]")
        w = (self._area * f).astype(np.float32)
        if not np.isfinite(w).all() or (w < 0.0).any():
            raise ValueError(f"region {name!r}: negative or non-finite weights")
        if not w.astype(np.float64).sum() > 0.0:
            raise ValueError(f"region {name!r}: the weights sum to 0 (no cell of the grid belongs to it)")
        self._maps[name] = w
        self._device_cache.clear()
        return self

    def add_global(self, name: str = "global") -> "Regions":
        return self.add_fraction(name, np.ones(self._area.shape))

    def add_lat_band(self, name: str, lat_min: float, lat_max: float) -> "Regions":
        """The rows whose centre latitude lies in [lat_min, lat_max]."""
        rows = (self._lats >= lat_min) & (self._lats <= lat_max)
        return self.add_fraction(name, np.broadcast_to(rows[:, None], self._area.shape))

    def add_box(self, name: str, lat: Sequence[float], lon: Sequence[float]) -> "Regions":
        """The cells whose centre c has lo <= c <= hi in latitude and in longitude.  Longitudes (the grid's and the box's) are
        taken mod 360; with lo > hi the box wraps across 0 degrees."""
        rows = (self._lats >= lat[0]) & (self._lats <= lat[1])
        c, lo, hi = np.mod(self._lons, 360.0), float(np.mod(lon[0], 360.0)), float(np.mod(lon[1], 360.0))
        cols = ((c >= lo) & (c <= hi)) if lo <= hi else ((c >= lo) | (c <= hi))
        return self.add_fraction(name, rows[:, None] & cols[None, :])

    @classmethod
    def standard(cls, lats, lons, area_weights) -> "Regions":
        """`global`, `tropics` (|lat| <= 20), `nh_extratropics` (lat > 20), `sh_extratropics` (lat < -20) and `nino34`
        (5S-5N, 190E-240E)."""
        r = cls(lats, lons, area_weights)
        shape = r._area.shape
        r.add_global()
        r.add_fraction("tropics", np.broadcast_to((np.abs(r._lats) <= 20.0)[:, None], shape))
        r.add_fraction("nh_extratropics", np.broadcast_to((r._lats > 20.0)[:, None], shape))
        r.add_fraction("sh_extratropics", np.broadcast_to((r._lats < -20.0)[:, None], shape))
        r.add_box("nino34", lat=(-5.0, 5.0), lon=(190.0, 240.0))
        return r

    # -- what the launch takes ----------------------------------------------------------------------------------------------
    def stacked(self) -> np.ndarray:
        """(n_regions, H, W) fp32, in insertion order."""
        if not self._maps:
            raise ValueError("no regions defined")
        return np.stack(list(self._maps.values()))

    def on_device(self, device) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> ((n_regions, H * W) fp32 maps, (n_regions,) float64 sums of the fp32 maps) on `device`, formed once per device."""
        device = torch.device(device)
        hit = self._device_cache.get(device)
        if hit is None or hit[0] != len(self._maps):
            w = torch.from_numpy(self.stacked()).reshape(len(self._maps), -1).to(device)
            hit = (len(self._maps), w, w.double().sum(dim=1))
            self._device_cache[device] = hit
        return hit[1], hit[2]


class RegionalMeanAggregator:
    """Per-timestep series of `MeanAggregator`'s area-weighted metrics for every region of a `Regions`.

    Same `record_batch(loss, target_data, gen_data, target_data_norm, gen_data_norm, i_time_start)` and bookkeeping as
    `MeanAggregator`: the mean over a window's samples is added at `i_time_start ...`, divided at read-out by the number of
    windows that touched a time index and averaged over ranks (`dist.reduce_mean`).  `is_ensemble=True` needs member-stacked
    `(members, samples, time, lat, lon)` predictions and refuses flat rows.  Metrics and definitions are `MeanAggregator`'s:
    `weighted_rmse`, `weighted_bias` (of the ensemble mean), `weighted_mean_gen / _target`, `weighted_std_gen / _target`, for
    ensembles `weighted_crps` (fair) and `weighted_ssr`.

    Per window: one `sdy_region_series` launch per run of same-shaped variables (normally one) reads the member-stacked view in
    place and writes the eight float64 sums of every (variable, region, sample, time); a fixed handful of torch operations on
    that small tensor, for all variables at once, divides by the regions' weight sums and forms the metrics.  The per-point
    arithmetic is float64 (`MeanAggregator`'s kernel: fp32), so the `global` region agrees with `MeanAggregator` to fp32
    rounding of the points, not to the bit.  The first window fixes the variables; all of them share the sample count and the
    grid of the `Regions`.

    Zero-weight rule: a grid point whose weight in a region is exactly 0 contributes nothing to that region, NaN values
    included; anywhere else a NaN propagates into that region's series.

    `get_series()` -> `{"<metric>/<region>/<variable>": (n_timesteps,) float64}`; `get_logs(label)` -> `{f"{label}/series": ...}`
    with numpy arrays."""

    def __init__(self, regions: Regions, target: str = "denorm", n_timesteps: int = 1, is_ensemble: bool = False, dist=None):
        if target not in ("norm", "denorm"):
            raise ValueError(f"target must be 'norm' or 'denorm', got {target!r}")
        if len(regions) < 1:
            raise ValueError("no regions defined")
        if int(n_timesteps) < 1:
            raise ValueError(f"n_timesteps must be positive, got {n_timesteps}")
        self._regions = regions
        self._target = target
        self._n_timesteps = int(n_timesteps)
        self.is_ensemble = bool(is_ensemble)
        self._dist = TorchDistributed() if dist is None else dist
        self._names: Optional[List[str]] = None
        self._total: Optional[torch.Tensor] = None               # (metrics, nvars, regions, n_timesteps) float64
        self._n_batches: Optional[torch.Tensor] = None           # (n_timesteps,) int32
        self._buffers: Dict[tuple, Tuple[torch.Tensor, torch.Tensor]] = {}
        self._members: Dict[tuple, torch.Tensor] = {}

    @property
    def metric_names(self) -> List[str]:
        return list(SERIES_METRICS + (SERIES_METRICS_ENSEMBLE if self.is_ensemble else ()))

    def _sums(self, lay, device) -> torch.Tensor:
        """The window's raw sums (nvars, regions, n1, T, 8): one launch per run of same-shaped variables."""
        H, W = self._regions.shape
        R, n1, T = len(self._regions), lay[0].n1, lay[0].T
        weights, _ = self._regions.on_device(device)
        key = (device, len(lay), R, n1, T)
        if key not in self._buffers:
            ws_bytes = lib.sdy_region_series_workspace_bytes(min(len(lay), 96), R, n1, T, H * W)
            self._buffers[key] = (torch.empty(len(lay), R, n1, T, 8, dtype=torch.float64, device=device),
                                  torch.empty(max(ws_bytes // 8, 1), dtype=torch.float64, device=device))
        out, ws = self._buffers[key]
        with torch.cuda.device(device):
            for first, last in runs(lay, lambda l: l.extents):
                a = SdyRegionSeriesArgs()
                fill_window(a.win, lay, first, last)
                a.HW, a.n_regions, a.weights = H * W, R, ptr(weights)
                a.out, a.ws, a.ws_bytes = ptr(out[first:last]), ptr(ws), ws.numel() * 8
                check(lib.sdy_region_series(C.byref(a), current_stream()), "sdy_region_series")
        return out

    @torch.no_grad()
    def record_batch(self, loss, target_data, gen_data, target_data_norm=None, gen_data_norm=None, i_time_start: int = 0):
        del loss
        if self._target == "norm":
            target_data, gen_data = target_data_norm, gen_data_norm
        if any(g.dim() != (5 if self.is_ensemble else 4) for g in gen_data.values()):
            if self.is_ensemble:
                raise ValueError(whole_ics_message("RegionalMeanAggregator(is_ensemble=True)"))
            raise ValueError("RegionalMeanAggregator(is_ensemble=False) takes (samples, time, lat, lon) predictions")
        lay = window_layouts(target_data, gen_data)
        names, i_time_start, T = list(gen_data), int(i_time_start), lay[0].T
        if i_time_start < 0 or i_time_start + T > self._n_timesteps:
            raise ValueError(f"times {i_time_start}..{i_time_start + T - 1} outside the aggregator's {self._n_timesteps}")
        if self._names is not None and names != self._names:
            raise ValueError("the variables of a window differ from the first window's")
        for l in lay:
            if (l.H, l.W) != tuple(self._regions.shape) or l.n1 != lay[0].n1:
                raise ValueError(f"a {(l.H, l.W)} grid with {l.n1} samples against regions on {tuple(self._regions.shape)} "
                                 f"and {lay[0].n1} samples")
            if l.n0 > SDY_REGION_MAX_MEMBERS:
                raise ValueError(f"at most {SDY_REGION_MAX_MEMBERS} members, got {l.n0}")
        if not all(l.gen.is_cuda and l.target.is_cuda for l in lay):
            raise RuntimeError("sdy_amd aggregators run on the GPU only (no CPU fallback)")
        device = lay[0].gen.device if self._total is None else self._total.device
        if any(l.gen.device != device or l.target.device != device for l in lay):
            raise ValueError(f"tensors of a window on another device than {device}")

        _, wsum = self._regions.on_device(device)
        s = self._sums(lay, device) / wsum[None, :, None, None, None]                  # (nvars, regions, n1, T, 8)
        mse, var, crps, bias, mg, mg2, mt, mt2 = s.unbind(dim=-1)
        rmse = mse.sqrt()
        vals = [rmse, bias, mg, mt, (mg2 - mg * mg).clamp_min(0.0).sqrt(), (mt2 - mt * mt).clamp_min(0.0).sqrt()]
        if self.is_ensemble:
            members = tuple(l.n0 for l in lay)
            if (device, members) not in self._members:
                E = torch.tensor(members, dtype=torch.float64, device=device)
                self._members[(device, members)] = ((E + 1.0) / E).sqrt()[:, None, None, None]
            vals += [crps, var.sqrt() * self._members[(device, members)] / rmse]
        window = torch.stack(vals).mean(dim=3)                                        # mean over the window's samples
        if self._total is None:
            self._names = names
            self._total = torch.zeros(len(vals), len(names), len(self._regions), self._n_timesteps, dtype=torch.float64,
                                      device=device)
            self._n_batches = torch.zeros(self._n_timesteps, dtype=torch.int32, device=device)
        self._total[..., i_time_start:i_time_start + T] += window
        self._n_batches[i_time_start:i_time_start + T] += 1

    @torch.no_grad()
    def get_series(self) -> Dict[str, torch.Tensor]:
        if self._total is None:
            raise ValueError("No batches have been recorded.")
        series = self._dist.reduce_mean(self._total / self._n_batches)
        return {f"{metric}/{region}/{name}": series[m, v, r]
                for m, metric in enumerate(self.metric_names) for r, region in enumerate(self._regions.names)
                for v, name in enumerate(self._names)}

    @torch.no_grad()
    def get_logs(self, label: str):
        series = self.get_series()
        host = torch.stack(list(series.values())).cpu().numpy()                       # one copy for all series
        data = {k: host[i] for i, k in enumerate(series)}
        return {f"{label}/series": data}
