"""Dry-air conservation diagnostics: host mirror of `compute_dry_air_absolute_differences`
(`src/ace_inference/core/aggregator/climate_data.py:199-233`), `get_dry_air_nonconservation` and `ConservationLossConfig` /
`ConservationLoss` (`core/loss.py:11-101`), and `DerivedMetricsAggregator` / `DryAir`
(`core/aggregator/one_step/derived.py`).

The quantity, per sample b and time t of `(sample, time, lat, lon)` data in physical units:
    gm[b, t] = area-weighted global mean (`metrics.weighted_mean`) of `surface_pressure_due_to_dry_air`
             = ps - g * (1/g) * sum_k dp_k * q_k, from `specific_total_water_<k>` (natural order) and `PRESsfc` | `PS`
and from it `absdiff[t] = mean_b |gm[b, t+1] - gm[b, t]|` (the reference's return value, shape `(time - 1,)`) and its mean
(`get_dry_air_nonconservation`, the factor of `dry_air_penalty`).  One call is two launches (`sdy_dry_air_series`: a reduce
pass that reads the K levels and the pressure once, and one small block that combines), whatever the batch, the number of
times and K; `(B, T, H, W)` tensors, their `[:, 0:2]` views and the stepper's packed tensors are read in place through a
sample and a time stride.  The column quantity is the reference's fp32 chain (csrc/corrector_math.h, shared with the
corrector); the sums are float64 in a fixed order, so a row's global mean depends neither on the batch it is in nor on the
run, and the results are float64 device tensors that stay on the GPU until somebody reads them (the reference sums in fp32).

Everything here is off by default.  The reference wires `ConservationLoss` into its single-module stepper only
(`core/stepper.py:570-572`) and `DerivedMetricsAggregator` into its one-step aggregator; its multi-step stepper
(`stepper_multistep.py`) uses neither.  `MultiStepStepper(..., conservation_loss=...)` here is a capability behind the
reference's class names, not a mirror of that file.

As in the reference: missing water or pressure gives `compute_dry_air_absolute_differences` a NaN of shape `(1,)` (hence a NaN
`dry_air_loss`, and a NaN `loss`: the reference adds it), one time step gives an empty result and a NaN mean, a level count
other than len(ak) - 1 raises the reference's ValueError.  `DryAir.record` on data without the fields raises KeyError: that is
what `ClimateData` does before the NaN branch its docstring promises can be reached.

GPU only: CPU tensors raise, like every module of this package.  ak / bk are rounded to fp32.  The grid size must be a multiple
of 4 (the kernel reads float4).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Any, Dict, List, Mapping, NamedTuple, Optional, Sequence, Tuple

import torch

from ._lib import SDY_DERIVED_MAX_LEVELS, SdyDryAirArgs, check, current_stream, lib, ptr
from .derived import FIELD_NAMES, WATER_PREFIXES, _host_levels, natural_sort

_LEVELS_MESSAGE = "Number of vertical levels in ak, bk, and specific_total_water mustbe the same."
DRY_AIR = "surface_pressure_due_to_dry_air"


class DryAirResult(NamedTuple):
    """float64 device tensors of one launch."""
    gm: torch.Tensor            # (rows, T): global-mean dry-air surface pressure per sample and time
    absdiff: torch.Tensor       # (T - 1,): mean over samples of |gm[:, t+1] - gm[:, t]|
    mean: torch.Tensor          # 0-d: mean of absdiff (NaN with one time step)


def resolve(names: Sequence[str]) -> Optional[Tuple[List[str], str]]:
    """`ClimateData`'s name resolution on a dict with these keys, without touching a tensor: (water levels in natural order,
    surface pressure name), or None where the reference catches its KeyError."""
    water = natural_sort([n for n in names if n.startswith(WATER_PREFIXES[0])])
    keys = set(names)
    ps = next((p for p in FIELD_NAMES["surface_pressure"] if p in keys), None)
    if not water or ps is None:
        return None
    return water, ps


def _rows(t: torch.Tensor) -> Optional[Tuple[int, int, int]]:
    """(rows, row stride, time stride) when `t (..., T, H, W)` can be read in place: (H, W) contiguous, the leading axes fold
    into one stride, every stride a multiple of 4 floats and the first element on a 16-byte boundary; else None."""
    H, W = t.shape[-2:]
    if t.stride()[-2:] != (W, 1) or t.data_ptr() % 16:
        return None
    lead = [(n, s) for n, s in zip(t.shape[:-3], t.stride()[:-3]) if n > 1]
    for (_, s_outer), (n_inner, s_inner) in zip(lead, lead[1:]):
        if s_outer != s_inner * n_inner:
            return None
    rows = 1
    for n in t.shape[:-3]:
        rows *= n
    s_row = lead[-1][1] if lead else 0
    s_time = t.stride(-3) if t.shape[-3] > 1 else 0
    if s_row % 4 or s_time % 4 or s_row < 0 or s_time < 0:
        return None
    return rows, s_row, s_time


class DryAirSeries:
    """The launcher behind every entry of this module: area weights and ak / bk read to the host once."""

    def __init__(self, area: torch.Tensor, sigma_coordinates):
        self._ak, self._bk = _host_levels(sigma_coordinates)
        if len(self._ak) != len(self._bk) or len(self._ak) < 2:
            raise ValueError(_LEVELS_MESSAGE)
        if area.dim() != 2:
            raise ValueError(f"area: expected (n_lat, n_lon), got {tuple(area.shape)}")
        self._area = area.detach().to(torch.float32).contiguous()
        self._area_on: Dict[torch.device, torch.Tensor] = {}

    @property
    def n_levels(self) -> int:
        return len(self._ak) - 1

    def area_on(self, device) -> torch.Tensor:
        if device not in self._area_on:
            self._area_on[device] = self._area.to(device)
        return self._area_on[device]

    def check_levels(self, n_water: int) -> None:
        if n_water != self.n_levels:
            raise ValueError(_LEVELS_MESSAGE)
        if n_water > SDY_DERIVED_MAX_LEVELS:
            raise NotImplementedError(f"sdy_amd.conservation: at most {SDY_DERIVED_MAX_LEVELS} levels of specific total "
                                      f"water, got {n_water}")

    def args(self, water: Sequence[torch.Tensor], ps: torch.Tensor, stats: Optional[Sequence[Tuple[float, float]]] = None,
             channels: Optional[Sequence[int]] = None) -> Tuple[SdyDryAirArgs, list, int, int]:
        """The argument block for K level tensors and the pressure, each `(..., T, H, W)` of one shape (the leading axes are
        pooled into rows), without outputs and workspace: -> (args, tensors that must outlive the launch, rows, T).  `stats`
        (mean, std) and `channels` per tensor, water first and the pressure last, are the packed layout: tensor i is then
        `(..., T, C, H, W)`-like storage whose plane `channels[i]` lies `channels[i] * H * W` floats behind the element."""
        tensors = list(water) + [ps]
        self.check_levels(len(water))
        ref = tensors[0]
        if any(not t.is_cuda for t in tensors):
            raise RuntimeError("sdy_amd conservation diagnostics run on the GPU only (no CPU fallback)")
        if ref.dim() < 3 or tuple(ref.shape[-2:]) != tuple(self._area.shape):
            raise ValueError(f"expected (..., time, {self._area.shape[0]}, {self._area.shape[1]}), got {tuple(ref.shape)}")
        for t in tensors:
            if t.shape != ref.shape or t.dtype != torch.float32 or t.device != ref.device:
                raise ValueError(f"{tuple(t.shape)} {t.dtype} on {t.device}; expected float32 {tuple(ref.shape)} on {ref.device}")
        H, W = ref.shape[-2:]
        HW, T = H * W, ref.shape[-3]
        if HW % 4:
            raise ValueError(f"sdy_amd.conservation: lat * lon must be a multiple of 4, got {H} x {W}")
        a = SdyDryAirArgs()
        a.HW, a.T, a.K = HW, T, len(water)
        for k, (x, y) in enumerate(zip(self._ak, self._bk)):
            a.ak[k], a.bk[k] = x, y
        a.area = ptr(self.area_on(ref.device))
        keep = []
        rows = None
        for i, t in enumerate(tensors):
            lay = _rows(t)
            if lay is None:                      # a view that does not fold into (row, time) strides: one copy
                assert channels is None, "packed tensors are read in place"
                t = t.contiguous()
                keep.append(t)
                lay = _rows(t)
            slot = a.q[i] if i < len(water) else a.ps
            slot.base, slot.stride_b, slot.stride_t = ptr(t), lay[1], lay[2]
            slot.channel = 0 if channels is None else int(channels[i])
            slot.mean, slot.std = (0.0, 1.0) if stats is None else stats[i]
            rows = lay[0]
        a.B = rows
        return a, keep, rows, T

    def launch(self, a: SdyDryAirArgs, rows: int, T: int, device, mean_out: Optional[torch.Tensor] = None,
               accumulate: bool = False) -> DryAirResult:
        """Two launches on the current stream.  `mean_out`: a float64 device tensor of one element that receives (or, with
        `accumulate`, is increased by) the mean instead of the result's own slot; it is left alone when T = 1."""
        if rows == 0:
            nan = torch.full((), float("nan"), dtype=torch.float64, device=device)
            return DryAirResult(torch.empty(0, T, dtype=torch.float64, device=device),
                                torch.full((max(T - 1, 0),), float("nan"), dtype=torch.float64, device=device), nan)
        with torch.cuda.device(device):
            n_ws = lib.sdy_dry_air_workspace_bytes(rows, T, a.HW) // 8
            buf = torch.empty(rows * T + T + n_ws, dtype=torch.float64, device=device)
            gm, absdiff, mean = buf[:rows * T].view(rows, T), buf[rows * T:rows * T + T - 1], buf[rows * T + T - 1]
            if T == 1:
                mean.fill_(float("nan"))          # the mean of an empty difference
            target = mean if mean_out is None else mean_out
            assert target.dtype == torch.float64 and target.device == buf.device and target.numel() == 1
            a.gm, a.absdiff, a.mean_absdiff, a.accumulate = ptr(gm), ptr(absdiff), ptr(target), int(bool(accumulate))
            ws = buf[rows * T + T:]
            a.ws, a.ws_bytes = ptr(ws), n_ws * 8
            check(lib.sdy_dry_air_series(C.byref(a), current_stream()), "sdy_dry_air_series")
        return DryAirResult(gm, absdiff, target.reshape(()) if T > 1 else mean)

    def __call__(self, data: Mapping[str, torch.Tensor], times: Optional[slice] = None,
                 mean_out: Optional[torch.Tensor] = None, accumulate: bool = False) -> Optional[DryAirResult]:
        """The series of a dict of `(..., time, lat, lon)` tensors (`times`: a slice of the time axis, read as a view); None
        when the water or the pressure is missing."""
        names = resolve(list(data))
        if names is None:
            return None
        water, ps = names
        pick = (lambda t: t) if times is None else (lambda t: t[..., times, :, :])
        a, keep, rows, T = self.args([pick(data[n]) for n in water], pick(data[ps]))
        return self.launch(a, rows, T, data[ps].device, mean_out, accumulate)

    def packed(self, x: torch.Tensor, names: Sequence[str], means: Mapping[str, float],
               stds: Mapping[str, float]) -> Optional[DryAirResult]:
        """The global means `gm (B, 1)` of a normalised packed `(B, C, H, W)` tensor whose channels are `names`, as the
        stepper holds a state: every plane is read where it lies and denormalised in the kernel."""
        found = resolve(list(names))
        if found is None:
            return None
        water, ps = found
        used = water + [ps]
        B, n, H, W = x.shape
        assert x.is_contiguous() and n == len(names)
        view = x.as_strided((B, 1, H, W), (n * H * W, 0, W, 1))
        stats = [(means[v], stds[v]) if v in means else (0.0, 1.0) for v in used]
        a, keep, rows, T = self.args([view] * len(water), view, stats=stats, channels=[list(names).index(v) for v in used])
        return self.launch(a, rows, T, x.device)


def _nan() -> torch.Tensor:
    return torch.tensor([float("nan")])


def compute_dry_air_absolute_differences(data: Mapping[str, torch.Tensor], area: torch.Tensor,
                                         sigma_coordinates) -> torch.Tensor:
    """`climate_data.compute_dry_air_absolute_differences` on a dict of `(sample, time, lat, lon)` device tensors: the
    `(time - 1,)` mean over samples of the absolute one-step change of the global-mean dry-air pressure, float64 on the
    device; the reference's `tensor([nan])` when the water or the pressure is missing."""
    if resolve(list(data)) is None:
        return _nan()
    return DryAirSeries(area, sigma_coordinates)(data).absdiff


def get_dry_air_nonconservation(data: Mapping[str, torch.Tensor], area_weights: torch.Tensor, sigma_coordinates) -> torch.Tensor:
    """`loss.get_dry_air_nonconservation`: the mean of the above, a 0-d float64 device tensor (NaN for one time step or
    missing fields)."""
    if resolve(list(data)) is None:
        return _nan().mean()
    return DryAirSeries(area_weights, sigma_coordinates)(data).mean


@dataclasses.dataclass
class ConservationLossConfig:
    """`loss.ConservationLossConfig`.  dry_air_penalty: a constant by which to multiply the one-step non-conservation of
    surface pressure due to dry air in Pa as an L1 penalty; None (the default): no such term."""
    dry_air_penalty: Optional[float] = None

    def build(self, area_weights: torch.Tensor, sigma_coordinates) -> "ConservationLoss":
        return ConservationLoss(config=self, area_weights=area_weights, sigma_coordinates=sigma_coordinates)


class ConservationLoss:
    """`loss.ConservationLoss`: `__call__(gen_data) -> (metrics, loss)` with `metrics["dry_air_loss"]` present only when a
    penalty is set; float32 tensors, like the reference's, on the data's device."""

    def __init__(self, config: ConservationLossConfig, area_weights: torch.Tensor, sigma_coordinates):
        self._config = config
        self._area_weights = area_weights
        self._sigma_coordinates = sigma_coordinates
        self.series = DryAirSeries(area_weights, sigma_coordinates)

    @property
    def config(self) -> ConservationLossConfig:
        return self._config

    @property
    def dry_air_penalty(self) -> Optional[float]:
        return self._config.dry_air_penalty

    def __call__(self, gen_data: Mapping[str, torch.Tensor]) -> Tuple[Dict[str, torch.Tensor], torch.Tensor]:
        metrics: Dict[str, torch.Tensor] = {}
        device = next((t.device for t in gen_data.values() if torch.is_tensor(t)), torch.device("cpu"))
        loss = torch.tensor(0.0, device=device)
        if self._config.dry_air_penalty is not None:
            res = self.series(gen_data)
            mean = _nan().mean().to(device) if res is None else res.mean
            dry_air_loss = (self._config.dry_air_penalty * mean).to(torch.float32)
            metrics["dry_air_loss"] = dry_air_loss
            loss = loss + dry_air_loss
        return metrics, loss

    def window(self, gen_data: Mapping[str, torch.Tensor], mean_out: torch.Tensor) -> None:
        """For `MultiStepStepper`: the mean non-conservation of a window's generated timelines into `mean_out` (one float64
        device element), unscaled, behind the window's launches; NaN where the reference gives NaN.  No host sync."""
        res = self.series(gen_data, mean_out=mean_out)
        if res is None or res.gm.shape[1] < 2:
            mean_out.fill_(float("nan"))

    def get_state(self) -> Dict[str, Any]:
        return {"config": dataclasses.asdict(self._config), "sigma_coordinates": self._sigma_coordinates,
                "area_weights": self._area_weights}

    @classmethod
    def from_state(cls, state) -> "ConservationLoss":
        return cls(config=ConservationLossConfig(**state["config"]), sigma_coordinates=state["sigma_coordinates"],
                   area_weights=state["area_weights"])


class DerivedMetricsAggregator:
    """`one_step.derived.DerivedMetricsAggregator` with its one metric, `DryAir`: per batch the mean over samples of
    |gm[:, 1] - gm[:, 0]| of target and of gen, summed over batches; `get_logs(label)` divides by the batch count and returns
    `<label>/surface_pressure_due_to_dry_air/{target,gen}` as 0-d float64 device tensors.

    Each `record_batch` is one `sdy_dry_air_series` call per side on the `[:, 0:2]` view of the time axis, read in place, and
    the kernel adds the batch's value to the running totals, which stay on the device: no host sync, no torch arithmetic.

    Ensembles.  The reference has no rule for member-stacked data (`[:, 0:2]` of a `(members, samples, time, lat, lon)` gen
    would cut the sample axis).  The rule is this library's own, the one of the video aggregator and the histogram writer: gen
    is POOLED over members x samples, i.e. the first two TIME steps of every (member, sample) row enter one mean -- what the
    reference computes from flat `(members * samples, time, lat, lon)` gen."""

    def __init__(self, area_weights: torch.Tensor, sigma_coordinates):
        self.area_weights = area_weights
        self.sigma_coordinates = sigma_coordinates
        self._series = DryAirSeries(area_weights, sigma_coordinates)
        self._totals: Optional[torch.Tensor] = None          # (target, gen), float64, on the device
        self._n_batches = 0

    @torch.no_grad()
    def record_batch(self, target_data: Mapping[str, torch.Tensor], gen_data: Mapping[str, torch.Tensor],
                     target_data_norm=None, gen_data_norm=None) -> None:
        del target_data_norm, gen_data_norm  # unused
        sides = []
        for d in (target_data, gen_data):
            names = resolve(list(d))
            if names is None:                   # ClimateData raises before DryAir's NaN branch is reached
                raise KeyError(WATER_PREFIXES if not any(n.startswith(WATER_PREFIXES[0]) for n in d) else "surface_pressure")
            sides.append(names)
        device = target_data[sides[0][1]].device
        if self._totals is None and device.type == "cuda":
            self._totals = torch.zeros(2, dtype=torch.float64, device=device)
        for i, d in enumerate((target_data, gen_data)):
            res = self._series(d, times=slice(0, 2), mean_out=None if self._totals is None else self._totals[i:i + 1],
                               accumulate=True)
            if res.gm.shape[1] < 2:
                self._totals[i].fill_(float("nan"))
        self._n_batches += 1

    def get_logs(self, label: str) -> Dict[str, torch.Tensor]:
        if self._totals is None:
            raise ValueError("No batches have been recorded.")
        return {f"{label}/{DRY_AIR}/target": self._totals[0] / self._n_batches,
                f"{label}/{DRY_AIR}/gen": self._totals[1] / self._n_batches}
