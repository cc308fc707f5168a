"""Post-step state corrector: host mirror of `CorrectorConfig` / `Corrector` (`src/ace_inference/core/corrector.py`), which
the reference's single-module stepper applies between the network and the prescriber (`core/stepper.py:542-543`).

Three rules, in the reference's order, per sample and with area-weighted global means (`metrics.weighted_mean`):
  * `conserve_dry_air`: a globally constant offset on the dry-air pressure makes its global mean equal the input's; the
    surface pressure (`PRESsfc` | `PS`) is solved from it, specific total water unchanged;
  * `zero_global_mean_moisture_advection`: `tendency_of_total_water_path_due_to_advection` minus its global mean;
  * `moisture_budget_correction`: precipitation (`PRATEsfc` | `surface_precipitation_rate`) or evaporation (latent heat flux
    `LHTFLsfc` | `LHFLX`) scaled so that the global-mean budget closes, and for the `advection_and_*` modes the advective
    tendency recomputed as the per-column budget residual.
One call is three launches (`sdy_corrector`: reduce, scalar solve, apply) whatever the batch and the number of variables; the
global means stay in a device workspace, summed in float64 in a fixed order (the reference sums in fp32), so a sample's
result depends neither on the batch it is in nor on the run.  Elementwise arithmetic is the reference's fp32 chain.

Off by default everywhere.  The reference's multi-step stepper (`stepper_multistep.py`) does not apply a corrector at all;
`MultiStepStepper(..., corrector=...)` here is a capability behind the reference's class names, not a mirror of that file.

Deviations, both on the strict side: a budget correction without `zero_global_mean_moisture_advection` raises ValueError (the
rule the reference's docstring states and does not check), and the errors for a missing `surface_pressure` /
`specific_total_water` carry the reference's messages as `MissingFieldError`, which is both the ValueError those messages were
written for and the KeyError that `ClimateData` actually raises first.

GPU only: CPU tensors raise, like every module of this package.  ak / bk are rounded to fp32.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Dict, List, Mapping, NamedTuple, Optional, Sequence, Tuple

import torch

from ._lib import (SDY_CORRECTOR_BUDGET, SDY_CORRECTOR_DRY_AIR, SDY_CORRECTOR_ZERO_ADV, SDY_DERIVED_MAX_LEVELS,
                   SdyCorrectorArgs, check, current_stream, lib, ptr)
from .derived import FIELD_NAMES, WATER_PREFIXES, _host_levels, natural_sort

_ADV = "tendency_of_total_water_path_due_to_advection"


class MissingFieldError(KeyError, ValueError):
    """A field the corrector needs is not in the data."""

    def __str__(self):
        return str(self.args[0]) if self.args else ""


@dataclasses.dataclass
class CorrectorConfig:
    """`corrector.CorrectorConfig`: see the module docstring; everything off by default."""
    conserve_dry_air: bool = False
    zero_global_mean_moisture_advection: bool = False
    moisture_budget_correction: Optional[str] = None

    def build(self, area: torch.Tensor, sigma_coordinates) -> "Corrector":
        return Corrector(config=self, area=area, sigma_coordinates=sigma_coordinates)


class CorrectorPlan(NamedTuple):
    """Which entries feed the kernel (None: not needed) and which it rewrites."""
    gen_water: List[str]
    in_water: List[str]
    gen_ps: Optional[str]
    in_ps: Optional[str]
    lhf: Optional[str]
    prate: Optional[str]
    adv: Optional[str]
    written: List[str]            # gen names that get a new tensor, in (ps, lhf, prate, adv) order


def _field(keys, name) -> Optional[str]:
    return next((p for p in FIELD_NAMES[name] if p in keys), None)


def _collapse(t: torch.Tensor) -> Optional[int]:
    """Stride between samples when the leading axes of `(..., H, W)` fold into one, else None."""
    H, W = t.shape[-2:]
    if t.stride()[-2:] != (W, 1):
        return None
    lead = [(n, s) for n, s in zip(t.shape[:-2], t.stride()[:-2]) if n > 1]
    for (_, s_outer), (n_inner, s_inner) in zip(lead, lead[1:]):
        if s_outer != s_inner * n_inner:
            return None
    if lead and lead[-1][1] < H * W:      # an expanded (overlapping) view
        return None
    return lead[-1][1] if lead else H * W


class Corrector:
    def __init__(self, config: CorrectorConfig, area: torch.Tensor, sigma_coordinates):
        if config.moisture_budget_correction not in SDY_CORRECTOR_BUDGET:
            raise ValueError(f"moisture_budget_correction must be one of {list(SDY_CORRECTOR_BUDGET)}, got "
                             f"{config.moisture_budget_correction!r}")
        if config.moisture_budget_correction is not None and not config.zero_global_mean_moisture_advection:
            raise ValueError("zero_global_mean_moisture_advection must be True when moisture_budget_correction is set: the "
                             "budget closure assumes a zero global-mean moisture advection")
        self._config = config
        self._ak, self._bk = _host_levels(sigma_coordinates)
        if len(self._ak) != len(self._bk) or len(self._ak) < 2:
            raise ValueError("Number of vertical levels in ak, bk, and specific_total_water mustbe the same.")
        if area.dim() != 2:
            raise ValueError(f"area: expected (n_lat, n_lon), got {tuple(area.shape)}")
        self._area = area.detach().to(torch.float32).contiguous()
        self._area_on: Dict[torch.device, torch.Tensor] = {}
        self.flags = ((SDY_CORRECTOR_DRY_AIR if config.conserve_dry_air else 0)
                      | (SDY_CORRECTOR_ZERO_ADV if config.zero_global_mean_moisture_advection else 0))
        self.budget = SDY_CORRECTOR_BUDGET[config.moisture_budget_correction]

    @property
    def config(self) -> CorrectorConfig:
        return self._config

    @property
    def enabled(self) -> bool:
        return bool(self.flags or self.budget)

    def area_on(self, device) -> torch.Tensor:
        if device not in self._area_on:
            self._area_on[device] = self._area.to(device)
        return self._area_on[device]

    # ---- names ------------------------------------------------------------------------------------------------------
    def resolve(self, input_names: Sequence[str], gen_names: Sequence[str]) -> CorrectorPlan:
        """Name resolution of `Corrector.__call__` on dicts with these keys, without touching a tensor; raises what the
        reference raises for a missing field (module docstring)."""
        cfg = self._config
        ik, gk = set(input_names), set(gen_names)
        water = cfg.conserve_dry_air or self.budget != 0
        gen_water = natural_sort([n for n in gen_names if n.startswith(WATER_PREFIXES[0])])
        in_water = natural_sort([n for n in input_names if n.startswith(WATER_PREFIXES[0])])
        gen_ps, in_ps = _field(gk, "surface_pressure"), _field(ik, "surface_pressure")
        lhf = prate = adv = None
        written = []
        if cfg.conserve_dry_air:
            if in_ps is None:
                raise MissingFieldError("surface_pressure is required to force dry air conservation")
            if not gen_water:
                raise MissingFieldError("specific_total_water is required for conservation")
        if water:
            if gen_ps is None or in_ps is None:
                raise KeyError("surface_pressure")
            if not gen_water or not in_water:
                raise KeyError(WATER_PREFIXES)
            if len(gen_water) != len(self._ak) - 1 or len(in_water) != len(gen_water):
                raise ValueError("Number of vertical levels in ak, bk, and specific_total_water mustbe the same.")
            if len(gen_water) > SDY_DERIVED_MAX_LEVELS:
                raise NotImplementedError(f"sdy_amd.corrector: at most {SDY_DERIVED_MAX_LEVELS} levels of specific total "
                                          f"water, got {len(gen_water)}")
        if cfg.conserve_dry_air:
            written.append(gen_ps)
        if cfg.zero_global_mean_moisture_advection:
            adv = _field(gk, _ADV)
            if adv is None:
                raise KeyError(_ADV)
        if self.budget:
            lhf, prate = _field(gk, "latent_heat_flux"), _field(gk, "precipitation_rate")
            for name, found in (("latent_heat_flux", lhf), ("precipitation_rate", prate)):
                if found is None:
                    raise KeyError(name)
            written.append(lhf if self.budget in (2, 4) else prate)
        if adv is not None:
            written.append(adv)
        order = [gen_ps, lhf, prate, adv]
        written = [n for n in order if n in written]
        if not water:
            gen_water, in_water, gen_ps, in_ps = [], [], None, None
        return CorrectorPlan(gen_water, in_water, gen_ps, in_ps, lhf, prate, adv, written)

    def _args(self, plan: CorrectorPlan, B: int, HW: int, area: torch.Tensor, ws: torch.Tensor) -> SdyCorrectorArgs:
        a = SdyCorrectorArgs()
        a.B, a.HW, a.K, a.flags, a.budget = B, HW, max(len(plan.gen_water), 1), self.flags, self.budget
        for k, (x, y) in enumerate(zip(self._ak, self._bk)):
            if k <= SDY_DERIVED_MAX_LEVELS:
                a.ak[k], a.bk[k] = x, y
        a.area = ptr(area)
        a.ws, a.ws_bytes = ptr(ws), ws.numel() * ws.element_size()
        return a

    # ---- dicts ------------------------------------------------------------------------------------------------------
    def __call__(self, input_data: Mapping[str, torch.Tensor], gen_data: Mapping[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """`Corrector.__call__(input_data, gen_data)`: a new dict; the corrected entries are new tensors, every other entry
        is the tensor it was.  Device fp32 tensors of one shape `(..., n_lat, n_lon)`."""
        new = dict(gen_data)
        if not self.enabled:
            return new
        plan = self.resolve(list(input_data), list(gen_data))
        gen_names = plan.gen_water + [n for n in (plan.gen_ps, plan.lhf, plan.prate, plan.adv) if n is not None]
        in_names = plan.in_water + ([plan.in_ps] if plan.in_ps is not None else [])
        used = [(n, gen_data[n]) for n in gen_names] + [(n, input_data[n]) for n in in_names]
        ref_name, ref = used[0]
        if any(not t.is_cuda for _, t in used):
            raise RuntimeError("sdy_amd corrector runs on the GPU only (no CPU fallback)")
        if ref.dim() < 2 or ref.shape[-2:] != self._area.shape:
            raise ValueError(f"expected (..., {self._area.shape[0]}, {self._area.shape[1]}), got {tuple(ref.shape)}")
        for n, t in used:
            if t.shape != ref.shape or t.dtype != torch.float32 or t.device != ref.device:
                raise ValueError(f"{n}: {tuple(t.shape)} {t.dtype} on {t.device}; expected float32 {tuple(ref.shape)} on "
                                 f"{ref.device} like {ref_name}")
        HW = ref.shape[-2] * ref.shape[-1]
        B = ref.numel() // HW
        if B == 0:
            return new
        keep = []     # tensors that must outlive the launch (copies of views that do not fold into one stride)

        def var(slot, t):
            s = _collapse(t)
            if s is None:
                t = t.contiguous()
                keep.append(t)
                s = HW
            slot.base, slot.stride, slot.channel, slot.mean, slot.std = ptr(t), s, 0, 0.0, 1.0

        with torch.cuda.device(ref.device):
            ws = torch.empty(lib.sdy_corrector_workspace_bytes(B, HW) // 8, dtype=torch.float64, device=ref.device)
            a = self._args(plan, B, HW, self.area_on(ref.device), ws)
            for k, n in enumerate(plan.gen_water):
                var(a.gen_q[k], gen_data[n])
            for k, n in enumerate(plan.in_water):
                var(a.in_q[k], input_data[n])
            for slot, out, n, src in ((a.gen_ps, a.out_ps, plan.gen_ps, gen_data), (a.in_ps, None, plan.in_ps, input_data),
                                      (a.gen_lhf, a.out_lhf, plan.lhf, gen_data), (a.gen_prate, a.out_prate, plan.prate, gen_data),
                                      (a.gen_adv, a.out_adv, plan.adv, gen_data)):
                if n is None:
                    continue
                var(slot, src[n])
                if out is not None and n in plan.written:
                    new[n] = torch.empty(ref.shape, dtype=torch.float32, device=ref.device)
                    out.base, out.stride, out.channel = ptr(new[n]), HW, 0
            check(lib.sdy_corrector(C.byref(a), current_stream()), "sdy_corrector")
        return new

    # ---- the stepper's packed tensors ---------------------------------------------------------------------------------
    def bind(self, in_names: Sequence[str], out_names: Sequence[str], means: Mapping[str, float],
             stds: Mapping[str, float]) -> "PackedCorrector":
        """For `MultiStepStepper`: the corrector on the normalised packed tensors `state (B, n_in, H, W)` /
        `g (B, n_out, H, W)`, in place in `g`.  Every variable a rule touches must be in both packers."""
        plan = self.resolve(list(out_names), list(out_names)) if self.enabled else None
        if plan is not None:
            needed = plan.gen_water + [n for n in (plan.gen_ps, plan.lhf, plan.prate, plan.adv) if n is not None]
            missing = [n for n in needed if n not in in_names or n not in out_names]
            if missing:
                raise ValueError(f"Variables the corrector reads or rewrites must be in in_names and out_names, but {missing} "
                                 "are not.")
        return PackedCorrector(self, plan, list(in_names), list(out_names), dict(means), dict(stds))


class PackedCorrector:
    def __init__(self, corrector: Corrector, plan: Optional[CorrectorPlan], in_names, out_names, means, stds):
        self.corrector, self.plan = corrector, plan
        self.in_names, self.out_names, self.means, self.stds = in_names, out_names, means, stds

    def workspace(self, B: int, HW: int, device) -> torch.Tensor:
        return torch.empty(lib.sdy_corrector_workspace_bytes(B, HW) // 8, dtype=torch.float64, device=device)

    def __call__(self, state: torch.Tensor, g: torch.Tensor, ws: torch.Tensor) -> None:
        """Corrects the contiguous `g (B, n_out, H, W)` in place against `state (B, n_in, H, W)`; three launches."""
        plan = self.plan
        if plan is None:
            return
        B, n_out, H, W = g.shape
        n_in, HW = state.shape[1], H * W
        assert g.is_contiguous() and state.is_contiguous() and state.shape == (B, n_in, H, W)
        if (H, W) != tuple(self.corrector._area.shape):
            raise ValueError(f"corrector area is {tuple(self.corrector._area.shape)}, the window's grid is {(H, W)}")
        a = self.corrector._args(plan, B, HW, self.corrector.area_on(g.device), ws)

        def stat(n) -> Tuple[float, float]:
            return (self.means[n], self.stds[n]) if n in self.means else (0.0, 1.0)

        def gen_var(slot, n):
            slot.base, slot.stride, slot.channel = ptr(g), n_out * HW, self.out_names.index(n)
            slot.mean, slot.std = stat(n)

        def in_var(slot, n):
            slot.base, slot.stride, slot.channel = ptr(state), n_in * HW, self.in_names.index(n)
            slot.mean, slot.std = stat(n)

        for k, n in enumerate(plan.gen_water):
            gen_var(a.gen_q[k], n)
            in_var(a.in_q[k], n)
        if plan.gen_ps is not None:
            in_var(a.in_ps, plan.gen_ps)
        for slot, out, n in ((a.gen_ps, a.out_ps, plan.gen_ps), (a.gen_lhf, a.out_lhf, plan.lhf),
                             (a.gen_prate, a.out_prate, plan.prate), (a.gen_adv, a.out_adv, plan.adv)):
            if n is None:
                continue
            gen_var(slot, n)
            if n in plan.written:
                out.base, out.stride, out.channel = slot.base, slot.stride, slot.channel
        check(lib.sdy_corrector(C.byref(a), current_stream()), "sdy_corrector")
