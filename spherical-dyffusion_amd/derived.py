"""Derived water-budget variables of the inference loop: host mirror of `compute_derived_quantities`
(`src/ace_inference/inference/derived_variables.py`, called by `inference/loop.py:197,245` on the targets and on the
member-stacked predictions of every window).

Three variables, in the reference's registry order, from `specific_total_water_<k>` (levels in natural sort order),
surface pressure (`PRESsfc` | `PS`), latent heat flux (`LHTFLsfc` | `LHFLX`), precipitation rate (`PRATEsfc` |
`surface_precipitation_rate`) and `tendency_of_total_water_path_due_to_advection` (`ClimateData`,
`core/aggregator/climate_data.py`):
  * `surface_pressure_due_to_dry_air` = ps - g * twp;
  * `total_water_path` twp = (1/g) * sum_k dp_k * q_k, dp_k = (ak[k+1] + ps*bk[k+1]) - (ak[k] + ps*bk[k]);
  * `total_water_path_budget_residual` = (twp_t - twp_{t-1}) / 21600 s - (LHF / 2.5e6 - PRATE + advection), 0 at the first
    time.
All requested outputs of one dict come from ONE launch (`sdy_derived_water`) that reads every input element once; the
window driver's member-stacked view is read in place.  Same rules as the reference: a variable whose inputs are missing is
skipped with a warning, a derived name already in the dict raises ValueError, a level count other than len(ak) - 1 raises
ValueError, and the new keys follow the existing ones in registry order.

One deliberate deviation.  The reference takes the residual's time difference as `[:, 1:] - [:, :-1]` of whatever it is
handed; for the member-stacked predictions of an ensemble `(members, samples, time, lat, lon)` that is the SAMPLE axis (an
all-zero residual with one initial condition, a meaningless one with more).  Here the difference is always along the TIME
axis: axis 2 of 5-D member-stacked data, axis 1 of 4-D `(rows, time, lat, lon)` data.  So a trajectory's values do not
depend on how it is stacked, sharded or relayed, and each member gets exactly what the reference computes for that member
run alone.  Targets `(samples, time, ...)` and deterministic predictions are what the reference computes.

GPU only: CPU tensors raise, like every module of this package.  ak / bk are rounded to fp32 (the reference's are fp32
tensors, `data_loading/_xarray.py:57`).
"""
from __future__ import annotations

import ctypes as C
import logging
import re
from typing import Dict, List, Mapping, NamedTuple, Optional, Sequence, Tuple

import torch

from ._lib import SDY_DERIVED_MAX_LEVELS, SdyDerivedArgs, check, current_stream, lib, ptr

DRY_AIR = "surface_pressure_due_to_dry_air"
TOTAL_WATER_PATH = "total_water_path"
BUDGET_RESIDUAL = "total_water_path_budget_residual"
DERIVED_NAMES = (DRY_AIR, TOTAL_WATER_PATH, BUDGET_RESIDUAL)          # the reference's registry order

# ClimateData's prefixes (CLIMATE_FIELD_NAME_PREFIXES) of the inputs used here
WATER_PREFIXES = ["specific_total_water_"]
FIELD_NAMES = {
    "surface_pressure": ["PRESsfc", "PS"],
    "latent_heat_flux": ["LHTFLsfc", "LHFLX"],
    "precipitation_rate": ["PRATEsfc", "surface_precipitation_rate"],
    "tendency_of_total_water_path_due_to_advection": ["tendency_of_total_water_path_due_to_advection"],
}
_BUDGET_FIELDS = ("latent_heat_flux", "precipitation_rate", "tendency_of_total_water_path_due_to_advection")


def natural_sort(names: Sequence[str]) -> List[str]:
    """`climate_data.natural_sort`: alphabetical, numbers compared as numbers (`_10` after `_2`)."""
    def key(item: str):
        return [int(c) if c.isdigit() else c.lower() for c in re.split("([0-9]+)", item)]

    return sorted(names, key=key)


class DerivedPlan(NamedTuple):
    """Which dict entries feed the kernel and which outputs it writes (None: skipped)."""
    water: List[str]                  # specific total water, natural order
    surface_pressure: Optional[str]
    budget: Optional[Tuple[str, str, str]]   # latent heat flux, precipitation rate, advective tendency
    outputs: List[str]                # subset of DERIVED_NAMES, registry order


def resolve(names: Sequence[str], n_ak: int, n_bk: int) -> DerivedPlan:
    """Name resolution of `compute_derived_quantities` on a dict with keys `names`, without touching any tensor:
    raises ValueError for a derived name already present or a level count other than len(ak) - 1 (= len(bk) - 1), logs
    the reference's warning for every variable whose inputs are missing."""
    keys = set(names)
    water = natural_sort([n for n in names if n.startswith(WATER_PREFIXES[0])])

    def field(name):
        return next((p for p in FIELD_NAMES[name] if p in keys), None)

    ps = field("surface_pressure")
    budget = tuple(field(n) for n in _BUDGET_FIELDS)
    outputs = []
    for label in DERIVED_NAMES:
        if label in keys:
            raise ValueError(f"Variable {label} already exists. It is not permitted to overwrite existing variables with "
                             "derived variables.")
        # the first input the reference's function would fail to find (its KeyError argument)
        missing = WATER_PREFIXES if not water else "surface_pressure" if ps is None else None
        if missing is None and label == BUDGET_RESIDUAL:
            missing = next((n for n, b in zip(_BUDGET_FIELDS, budget) if b is None), None)
        if missing is not None:
            logging.warning(f"Could not compute {label} because {missing!r} is missing")
            continue
        if label == DRY_AIR and (len(water) != n_ak - 1 or n_bk != n_ak):
            raise ValueError("Number of vertical levels in ak, bk, and specific_total_water mustbe the same.")
        outputs.append(label)
        keys.add(label)
    return DerivedPlan(water, ps, budget if BUDGET_RESIDUAL in outputs else None, outputs)


def _host_levels(sigma_coordinates) -> Tuple[List[float], List[float]]:
    ak, bk = sigma_coordinates.ak, sigma_coordinates.bk
    as_list = lambda v: [float(x) for x in (v.detach().cpu().tolist() if torch.is_tensor(v) else v)]  # noqa: E731
    return as_list(ak), as_list(bk)


def _layout(ts: List[torch.Tensor]) -> Tuple[List[torch.Tensor], int, int, int, int]:
    """-> (tensors, n0, n1, s0, s1): 5-D (n0, n1, T, H, W) or 4-D (n1, T, H, W) with n0 = 1, sharing one set of row strides,
    (T, H, W) contiguous and 16-byte aligned; otherwise every input is copied to a contiguous tensor."""
    t0 = ts[0]
    shape = t0.shape

    def fits(t):
        return (t.stride() == t0.stride() and t.stride()[-3:] == (shape[-2] * shape[-1], shape[-1], 1)
                and t.data_ptr() % 16 == 0 and all(s % 4 == 0 for s in t.stride()[:-3]))

    if not all(fits(t) for t in ts):
        ts = [t.clone(memory_format=torch.contiguous_format) for t in ts]
    st = ts[0].stride()
    if len(shape) == 5:
        return ts, shape[0], shape[1], st[0], st[1]
    return ts, 1, shape[0], 0, st[0]


def _apply(data: Mapping[str, torch.Tensor], ak: Sequence[float], bk: Sequence[float]) -> Dict[str, torch.Tensor]:
    plan = resolve(list(data), len(ak), len(bk))
    new = dict(data)
    if not plan.outputs:
        return new
    K = len(plan.water)
    if K > SDY_DERIVED_MAX_LEVELS:
        raise NotImplementedError(f"sdy_amd.derived: at most {SDY_DERIVED_MAX_LEVELS} levels of specific total water, "
                                  f"got {K}")
    names = plan.water + [plan.surface_pressure] + list(plan.budget or ())
    ins = [data[n] for n in names]
    ps = ins[K]
    if any(not t.is_cuda for t in ins):
        raise RuntimeError("sdy_amd derived variables run on the GPU only (no CPU fallback)")
    if ps.dim() not in (4, 5):
        raise ValueError(f"expected (rows, time, lat, lon) or (members, samples, time, lat, lon), got {tuple(ps.shape)}")
    for n, t in zip(names, ins):
        if t.shape != ps.shape or t.dtype != torch.float32 or t.device != ps.device:
            raise ValueError(f"{n}: {tuple(t.shape)} {t.dtype} on {t.device}; expected float32 {tuple(ps.shape)} on "
                             f"{ps.device} like {plan.surface_pressure}")
    ins, n0, n1, s0, s1 = _layout(ins)
    outs = {label: torch.empty(ps.shape, dtype=torch.float32, device=ps.device) for label in plan.outputs}
    a = SdyDerivedArgs()
    for k in range(K):
        a.q[k] = ptr(ins[k])
    a.ps = ptr(ins[K])
    if plan.budget is not None:
        a.lhf, a.prate, a.adv = (ptr(t) for t in ins[K + 1:])
    a.s0, a.s1, a.n0, a.n1 = s0, s1, n0, n1
    a.T, a.HW, a.K = ps.shape[-3], ps.shape[-2] * ps.shape[-1], K
    for k in range(K + 1):
        a.ak[k], a.bk[k] = ak[k], bk[k]
    a.dry, a.twp, a.resid = (ptr(outs.get(label)) for label in DERIVED_NAMES)
    with torch.cuda.device(ps.device):
        check(lib.sdy_derived_water(C.byref(a), current_stream()), "sdy_derived_water")
    new.update(outs)
    return new


def compute_derived_quantities(data: Mapping[str, torch.Tensor], sigma_coordinates) -> Dict[str, torch.Tensor]:
    """`derived_variables.compute_derived_quantities(data, sigma_coordinates)`: a new dict with the derived variables
    added (see the module docstring, deviation included).  `sigma_coordinates`: any object with `.ak` / `.bk` (tensors or
    sequences).  Reads ak / bk to the host on every call; a loop should use `deriver`."""
    ak, bk = _host_levels(sigma_coordinates)
    return _apply(data, ak, bk)


def deriver(sigma_coordinates):
    """The one-argument callable `run_inference(derive=...)` takes: `compute_derived_quantities` with ak / bk read to the
    host ONCE, here, so that applying it per window never waits for the device."""
    ak, bk = _host_levels(sigma_coordinates)
    return lambda data: _apply(data, ak, bk)


def chain(*derivers):
    """One callable for `run_inference(derive=...)` out of several, applied left to right: each takes the dict the one before it
    returned (`chain(deriver(sigma_coordinates), helmholtz.deriver(names))`: the water budget, then the winds' fields)."""
    def derive(data):
        for d in derivers:
            data = d(data)
        return data

    return derive
