"""Where a wind rotates and where it diverges: `helmholtz(u, v)` gives relative vorticity, divergence, streamfunction and
velocity potential of horizontal winds on the device, and `deriver` adds them to the dicts of `run_inference(derive=...)` so that
every diagnostic of the package applies to them.  The reference has no counterpart; the definition is the library's own
(include/sdy_amd.h above `sdy_helmholtz_coefficients`).

A wind (u eastward, v northward) on a sphere of radius a is V = grad chi + r x grad psi: u = -d psi/dy + d chi/dx,
v = d psi/dx + d chi/dy, zeta = laplace psi, delta = laplace chi.  With the spheroidal and toroidal coefficients s, t of
`sdy_amd.spectrum` (V_theta = -v, V_lambda = u; the two analyses of `sdy_vector_legendre_fwd`)

    zeta(l,m) = -sqrt(l (l + 1)) t / a     delta(l,m) = -sqrt(l (l + 1)) s / a
    psi(l,m)  = a t / sqrt(l (l + 1))      chi(l,m)   = a s / sqrt(l (l + 1))          all zero at l = 0

so psi and chi have zero mean, and solid-body rotation u = U cos(lat) gives zeta = 2 U sin(lat) / a, psi = -a U sin(lat).  On a
latitude-longitude grid none of the four follows from u and v point by point without finite differences that break at the poles.

The chain per chunk of winds: pack the rows (u run, then v run, each padded to a multiple of four fields), `sdy_rfft_lon` with a
per-field power-of-two factor, `sdy_vector_legendre_fwd`, ONE `sdy_helmholtz_coefficients` launch (the factor undone there, in
float64), `sdy_legendre_inv`, `sdy_irfft_lon`.  Everything runs on ONE cached plan in fp32 GEMM mode: psi of a real wind is of
order 1e8 m^2/s, far outside what the split-fp16 synthesis stages behind its fixed pre-scale, and the vector analysis runs on the
fp32 GEMM anyway.  Fields are independent columns of every stage: a wind's values do not depend on its company, and a
non-finite value stays in its own wind.

Aliasing: on the equiangular grid with lmax = nlat the analysis is exact only for winds band-limited below about nlat / 2 (as
for the spectra), and vorticity and divergence weight the highest, least trustworthy degrees most.  `truncate=L` zeroes every
degree above L in all outputs (a triangular truncation)."""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, Iterable, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import SdyHelmholtzArgs, check, current_stream, lib, ptr
from .sht import ShtPlan
from .spectrum import (DEFAULT_MAX_WORKSPACE_BYTES, _MAX_FIELDS, _MAX_ROWS_PER_CALL, _SLACK, VectorShtPlan, _Workspace,
                       _floats_per_field, _round_up, wind_pairs)

OUTPUTS = ("vorticity", "divergence", "streamfunction", "velocity_potential")
DEFAULT_RADIUS = 6.371e6
_PART = {"vorticity": 1, "divergence": 0, "streamfunction": 1, "velocity_potential": 0}       # 0: spheroidal s, 1: toroidal t
_KIND = {"vorticity": 0, "divergence": 0, "streamfunction": 1, "velocity_potential": 1}       # sdy_helmholtz_factors_host

_factor_cache: Dict[tuple, torch.Tensor] = {}
_ws = _Workspace()


def _pow2_scales(x: torch.Tensor):
    """Per field of x (F, H, W): (1 / s, s) with s the power of two at or above the field's largest magnitude, as
    `spectrum._field_scales` chooses it (1 for a field of zeros, exponents within +-100), but assembled from the exponent's
    bits: `torch.ldexp` multiplies by a `pow` that the device does not evaluate exactly for every exponent, and a factor one
    ulp off a power of two costs the chain its exact homogeneity (outputs of 2^k (u, v) are 2^k times those of (u, v), bit for
    bit)."""
    amax = torch.linalg.vector_norm(x, ord=float("inf"), dim=(1, 2))
    _, e = torch.frexp(amax)
    e = e.clamp(-100, 100).to(torch.int32)
    return ((127 - e) << 23).view(torch.float32), ((127 + e) << 23).view(torch.float32)


def _outputs(outputs: Iterable[str]) -> Tuple[str, ...]:
    outputs = (outputs,) if isinstance(outputs, str) else tuple(outputs)
    if not outputs or len(set(outputs)) != len(outputs) or not set(outputs) <= set(OUTPUTS):
        raise ValueError(f"outputs must be distinct names among {OUTPUTS}, got {outputs}")
    return outputs


def _factors(outputs: Tuple[str, ...], lmax: int, radius: float, truncate: Optional[int], device) -> torch.Tensor:
    """The factor table (n_out, lmax) float64 on the device, rows by `sdy_helmholtz_factors_host`; built once per key."""
    key = (outputs, lmax, radius, truncate, device)
    if key not in _factor_cache:
        table = np.empty((len(outputs), lmax), dtype=np.float64)
        for q, name in enumerate(outputs):
            check(lib.sdy_helmholtz_factors_host(lmax, radius, _KIND[name], -1 if truncate is None else truncate,
                                                 table[q].ctypes.data), "sdy_helmholtz_factors_host")
        _factor_cache[key] = torch.from_numpy(table).to(device)
    return _factor_cache[key]


@torch.no_grad()
def _transform(us: Sequence[torch.Tensor], vs: Sequence[torch.Tensor], outputs: Tuple[str, ...], grid: str, lmax: Optional[int],
               truncate: Optional[int], radius: float, max_workspace_bytes: Optional[int]) -> List[Dict[str, torch.Tensor]]:
    """The chain of the module docstring for the winds of several same-shaped (u, v) pairs of tensors, in one row space (pair
    after pair); one dict of outputs per pair."""
    u0 = us[0]
    for t in (*us, *vs):
        if not t.is_cuda:
            raise RuntimeError("sdy_amd.helmholtz runs on the GPU only (no CPU fallback); got a CPU tensor")
        if t.dim() < 2 or tuple(t.shape) != tuple(u0.shape):
            raise ValueError(f"expected u and v of one shape (..., nlat, nlon), got {tuple(u0.shape)} and {tuple(t.shape)}")
        if t.device != u0.device:
            raise ValueError(f"tensors on {u0.device} and {t.device}")
        if t.dtype != torch.float32:
            raise ValueError(f"expected float32, got {t.dtype}")
    if truncate is not None and int(truncate) < 0:
        raise ValueError(f"truncate must be None or a degree >= 0, got {truncate}")
    truncate = None if truncate is None else int(truncate)
    radius = float(radius)
    if not (radius > 0.0 and np.isfinite(radius)):
        raise ValueError(f"radius must be positive and finite, got {radius}")
    H, W = u0.shape[-2:]
    lead = tuple(u0.shape[:-2])
    n = int(np.prod(lead)) if lead else 1
    if n < 1:
        raise ValueError("empty tensor")
    N, n_out, device = n * len(us), len(outputs), u0.device
    limit = DEFAULT_MAX_WORKSPACE_BYTES if max_workspace_bytes is None else int(max_workspace_bytes)
    with torch.cuda.device(device):
        idx = device.index if device.index is not None else torch.cuda.current_device()
        plan = ShtPlan.get(H, W, lmax or H, W // 2 + 1, grid, idx, "f32")
        per_x, per_cs = _floats_per_field(plan)
        per_yf = plan.mtr * plan.nlat * 2
        # two fields with two coefficient tensors each, as kinetic_energy_spectrum; the output coefficients, their
        # grid-frequency tensor and (used with more than one chunk) the staged grids of every output
        per_wind = 2 * (per_x + 2 * per_cs + 1) + n_out * (per_cs + per_yf + H * W)
        step = min(max(limit - _SLACK, 0) // (4 * per_wind), _MAX_ROWS_PER_CALL, _MAX_FIELDS // 4,
                   ((1 << 31) - 1) // (max(2, n_out) * H * W)) // 4 * 4
        if step < 4:
            raise ValueError(f"helmholtz: four winds need {16 * per_wind} bytes of workspace, more than "
                             f"max_workspace_bytes = {limit}")
        one_chunk = N <= step
        store = torch.empty(n_out, _round_up(N, 4) if one_chunk else N, H, W, dtype=torch.float32, device=device)
        factor = _factors(outputs, plan.lmax, radius, truncate, device)
        flat: Dict[int, torch.Tensor] = {}
        for r0 in range(0, N, step):
            k = min(step, N - r0)
            Fh = _round_up(k, 4)
            F, Fo = 2 * Fh, n_out * Fh
            xb, Xf, Cd, Cm, Co, Yf, stage, zeros = _ws.parts(device, F * H * W, F * plan.mtr * H * 2, F * per_cs, F * per_cs,
                                                             Fo * per_cs, Fo * per_yf, 0 if one_chunk else Fo * H * W, F)
            xb = xb.view(2, Fh, H, W)
            for c, side in enumerate((us, vs)):
                for p, t in enumerate(side):
                    lo, hi = max(r0, p * n), min(r0 + k, (p + 1) * n)
                    if lo >= hi:
                        continue
                    dst = xb[c, lo - r0:hi - r0]
                    if hi - lo == n:
                        dst.view(*lead, H, W).copy_(t)                       # the whole tensor, whatever its strides
                    else:
                        if id(t) not in flat:
                            flat[id(t)] = t.reshape(-1, H, W)
                        dst.copy_(flat[id(t)][lo - p * n:hi - p * n])
            xb[:, k:].zero_()
            zeros.zero_()
            x = xb.view(F, H, W)
            inv, scale = _pow2_scales(x)
            s = current_stream()
            check(lib.sdy_rfft_lon(plan.handle, ptr(x), ptr(inv), ptr(zeros), None, ptr(Xf), 1, F, s), "sdy_rfft_lon")
            check(lib.sdy_vector_legendre_fwd(VectorShtPlan.get(plan).handle, ptr(Xf), ptr(Cd), ptr(Cm), 1, F, s),
                  "sdy_vector_legendre_fwd")
            a = SdyHelmholtzArgs()
            a.Cs_d, a.Cs_m, a.scale, a.factor, a.out = ptr(Cd), ptr(Cm), ptr(scale), ptr(factor), ptr(Co)
            a.lmax, a.mtr = plan.lmax, plan.mtr
            a.fields, a.u_offset, a.v_offset, a.n_winds = F, 0, Fh, k
            a.out_fields, a.out_stride, a.n_out = Fo, Fh, n_out
            for q, name in enumerate(outputs):
                a.part[q] = _PART[name]
            check(lib.sdy_helmholtz_coefficients(C.byref(a), s), "sdy_helmholtz_coefficients")
            check(lib.sdy_legendre_inv(plan.handle, ptr(Co), ptr(Yf), 1, Fo, s), "sdy_legendre_inv")
            y = store if one_chunk else stage
            check(lib.sdy_irfft_lon(plan.handle, ptr(Yf), None, ptr(y), 1, Fo, s), "sdy_irfft_lon")
            if not one_chunk:
                store[:, r0:r0 + k].copy_(stage.view(n_out, Fh, H, W)[:, :k])
    return [{name: store[q, p * n:(p + 1) * n].view(*lead, H, W) for q, name in enumerate(outputs)} for p in range(len(us))]


def helmholtz(u: torch.Tensor, v: torch.Tensor, outputs: Iterable[str] = OUTPUTS, grid: str = "equiangular",
              lmax: Optional[int] = None, truncate: Optional[int] = None, radius: float = DEFAULT_RADIUS,
              max_workspace_bytes: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """u, v (..., nlat, nlon) float32 on the device, eastward and northward in m/s, any strides in the leading axes ->
    {name: (..., nlat, nlon) float32, contiguous} for the names in `outputs` (module docstring): vorticity and divergence in
    1/s, streamfunction and velocity potential in m^2/s on a sphere of `radius` metres.  `lmax`: degrees of the transform
    (default nlat); `truncate`: the highest degree kept.  Winds are cut into chunks whose workspace stays within
    `max_workspace_bytes` (default `spectrum.DEFAULT_MAX_WORKSPACE_BYTES`); the workspace is one grow-only buffer."""
    return _transform([u], [v], _outputs(outputs), grid, lmax, truncate, radius, max_workspace_bytes)[0]


def deriver(names: Iterable[str], outputs: Iterable[str] = ("vorticity", "divergence"), levels: Optional[Iterable] = None,
            **kw) -> Callable[[Mapping[str, torch.Tensor]], Dict[str, torch.Tensor]]:
    """The callable `run_inference(derive=...)` takes.  The winds are `spectrum.wind_pairs(names)`, restricted to `levels` when
    given (what follows `wind_`: 0, 7, "10m").  For `wind_<k>` it adds `vorticity_<k>`, `divergence_<k>`, `streamfunction_<k>`,
    `velocity_potential_<k>` (those in `outputs`) to a NEW dict, after the existing keys, pair after pair; `kw` goes to
    `helmholtz`.  ValueError if a derived name is already present; a pair with a missing component is skipped.  It takes the 4-D
    target dicts and the 5-D member-stacked prediction dicts alike; all winds of one shape share one chain."""
    outputs = _outputs(outputs)
    pairs = wind_pairs(names)
    if levels is not None:
        keep = {str(k) for k in levels}
        pairs = {label: uv for label, uv in pairs.items() if label[len("wind_"):] in keep}
    opts = dict(grid="equiangular", lmax=None, truncate=None, radius=DEFAULT_RADIUS, max_workspace_bytes=None)
    unknown = set(kw) - set(opts)
    if unknown:
        raise TypeError(f"deriver: unexpected arguments {sorted(unknown)}")
    opts.update(kw)

    def derive(data: Mapping[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        new = dict(data)
        present = [(label[len("wind_"):], un, vn) for label, (un, vn) in pairs.items() if un in data and vn in data]
        for k, _, _ in present:
            for name in outputs:
                if f"{name}_{k}" in data:
                    raise ValueError(f"Variable {name}_{k} already exists. It is not permitted to overwrite existing variables "
                                     "with derived variables.")
        groups: Dict[tuple, list] = {}
        for item in present:
            u = data[item[1]]
            groups.setdefault((tuple(u.shape), u.device), []).append(item)
        done = {}
        for items in groups.values():
            outs = _transform([data[un] for _, un, _ in items], [data[vn] for _, _, vn in items], outputs, opts["grid"],
                              opts["lmax"], opts["truncate"], opts["radius"], opts["max_workspace_bytes"])
            for (k, _, _), out in zip(items, outs):
                done[k] = out
        for k, _, _ in present:
            for name in outputs:
                new[f"{name}_{k}"] = done[k][name]
        return new

    return derive
