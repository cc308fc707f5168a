"""Spherical power spectra on the device: `power_spectrum` of a field and `PowerSpectrumAggregator`, the per-degree power of
generated, target and error fields as a function of lead time -- whether a rollout blurs (loses power at high degree).

The reference has no counterpart: its only measure of blurring is `weighted_grad_mag_percent_diff`
(`src/ace_inference/core/metrics.py:210-241`).  Here the network's own forward transform does the work: the longitude FFT
and the Legendre analysis of the cached `ShtPlan` (`sdy_rfft_lon`, `sdy_legendre_fwd`) leave the coefficients in the internal
layout `Cs[l][m][ri][field]`, and one `sdy_degree_power` launch reduces them to

    P(l) = |a[l,0]|^2 + 2 sum_{m = 1 .. min(l, mmax - 1)} |a[l,m]|^2          l < lmax

in float64 (`csrc/spectrum.hip`).  The `(rows, lmax, mmax)` complex tensors of `RealSHT` are never formed.  With the transform's
`norm="ortho"`, sum_l P(l) is the integral of the squared field over the sphere for a band-limited field on the
Legendre-Gauss grid (not an identity on the equiangular grid with lmax = nlat).

Fields in physical units: the split-fp16 Legendre analysis stages its input as fp16 behind a fixed pre-scale, so a surface
pressure in Pa would leave its range.  Every field is therefore handed to the FFT divided by the power of two at or above its
largest magnitude (the FFT's fused per-field factor), and the reduction multiplies the coefficients back in float64; both
steps are exact, so the result is what the unscaled fp32 arithmetic would give.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import torch

from ._lib import SdySpectrumArgs, check, current_stream, lib, ptr
from .windows import FieldAccumulator
from .sht import ShtPlan

#: default `max_workspace_bytes`: packed rows, grid-frequency tensor and the coefficients of both sides of one chunk
DEFAULT_MAX_WORKSPACE_BYTES = 1 << 30
_MAX_FIELDS = 1 << 18          # fields of one transform call (far inside the 32-bit offsets of the Legendre kernels)
_MAX_ROWS_PER_CALL = 32768     # rows of one `power_spectrum` call (a grid extent of the reduction)
_SLACK = 2048                  # the parts of the workspace start on 256-byte boundaries


def _round_up(n: int, k: int) -> int:
    return (n + k - 1) // k * k


class _Workspace:
    """One grow-only float32 device buffer, carved into 256-byte aligned parts."""

    def __init__(self):
        self._buf: Optional[torch.Tensor] = None

    def parts(self, device, *floats: int) -> List[torch.Tensor]:
        sizes = [_round_up(n, 64) for n in floats]
        total = sum(sizes)
        if self._buf is None or self._buf.device != device or self._buf.numel() < total:
            self._buf = None
            self._buf = torch.empty(total, dtype=torch.float32, device=device)
        out, at = [], 0
        for n, padded in zip(floats, sizes):
            out.append(self._buf[at:at + n])
            at += padded
        return out

    @property
    def bytes(self) -> int:
        return 0 if self._buf is None else 4 * self._buf.numel()


def _field_scales(x: torch.Tensor):
    """Per field of x (F, H, W): (1 / s, s) with s the power of two at or above the field's largest magnitude (1 for a field of
    zeros; exponents kept within +-100 so that both are normal fp32 numbers)."""
    amax = torch.linalg.vector_norm(x, ord=float("inf"), dim=(1, 2))
    _, e = torch.frexp(amax)
    e = e.clamp(-100, 100)
    one = torch.ones_like(amax)
    return torch.ldexp(one, -e), torch.ldexp(one, e)


def _analyse(plan: ShtPlan, x: torch.Tensor, Xf: torch.Tensor, Cs: torch.Tensor, zeros: torch.Tensor) -> torch.Tensor:
    """Coefficients of the fields x (F, H, W), F % 4 == 0, into Cs; returns the per-field scale to undo."""
    F = x.shape[0]
    inv, scale = _field_scales(x)
    check(lib.sdy_rfft_lon(plan.handle, ptr(x), ptr(inv), ptr(zeros), None, ptr(Xf), 1, F, current_stream()), "sdy_rfft_lon")
    check(lib.sdy_legendre_fwd(plan.handle, ptr(Xf), ptr(Cs), 1, F, current_stream()), "sdy_legendre_fwd")
    return scale


def _floats_per_field(plan: ShtPlan):
    """(packed rows + grid-frequency tensor, coefficients) of one field, in floats."""
    return plan.nlat * plan.nlon + plan.mtr * plan.nlat * 2, plan.lmax * plan.mtr * 2


def _plan(H: int, W: int, lmax: Optional[int], mmax: Optional[int], grid: str, device) -> ShtPlan:
    idx = device.index if device.index is not None else torch.cuda.current_device()
    return ShtPlan.get(H, W, lmax or H, mmax or W // 2 + 1, grid, idx, None)      # gemm_mode: the package default


@torch.no_grad()
def power_spectrum(x: torch.Tensor, grid: str = "equiangular", lmax: Optional[int] = None, mmax: Optional[int] = None,
                   max_workspace_bytes: Optional[int] = None) -> torch.Tensor:
    """x (..., nlat, nlon) float32 on the device -> P (..., lmax) float64: the per-degree power of every field (module
    docstring), of the coefficients `RealSHT(nlat, nlon, lmax, mmax, grid)` would return."""
    if not x.is_cuda:
        raise RuntimeError("sdy_amd spectra run on the GPU only (no CPU fallback); got a CPU tensor")
    if x.dim() < 2:
        raise ValueError(f"expected (..., nlat, nlon), got {tuple(x.shape)}")
    H, W = x.shape[-2:]
    lead = tuple(x.shape[:-2])
    rows = x.reshape(-1, H, W).to(torch.float32)
    n = rows.shape[0]
    if n < 1:
        raise ValueError("empty tensor")
    limit = DEFAULT_MAX_WORKSPACE_BYTES if max_workspace_bytes is None else int(max_workspace_bytes)
    with torch.cuda.device(x.device):
        plan = _plan(H, W, lmax, mmax, grid, x.device)
        per_x, per_cs = _floats_per_field(plan)
        step = min(max(limit - _SLACK, 0) // (4 * (per_x + per_cs + 1)) // 4 * 4, _MAX_ROWS_PER_CALL)
        if step < 4:
            raise ValueError(f"power_spectrum: four fields need {16 * (per_x + per_cs)} bytes of workspace, more than "
                             f"max_workspace_bytes = {limit}")
        out = torch.zeros(n, plan.lmax, dtype=torch.float64, device=x.device)
        ws = _Workspace()
        for r0 in range(0, n, step):
            k = min(step, n - r0)
            F = _round_up(k, 4)
            xb, Xf, Cs, zeros = ws.parts(x.device, F * H * W, F * plan.mtr * H * 2, F * per_cs, F)
            xb = xb.view(F, H, W)
            xb[:k].copy_(rows[r0:r0 + k])
            xb[k:].zero_()
            zeros.zero_()
            scale = _analyse(plan, xb, Xf, Cs, zeros)
            unused = torch.zeros(k, plan.lmax, dtype=torch.float64, device=x.device)
            a = SdySpectrumArgs()
            a.gen = a.target = ptr(Cs)
            a.gen_scale = a.target_scale = ptr(scale)
            a.lmax, a.mtr, a.gen_fields, a.target_fields = plan.lmax, plan.mtr, F, F
            a.gen_var_stride = a.target_var_stride = 0
            a.gen_time_stride = a.target_time_stride = 1
            a.nvars, a.n0, a.n1, a.T, a.t_start, a.n_timesteps = 1, 1, 1, k, 0, k
            a.gen_power, a.target_power, a.err_power = out[r0:r0 + k].data_ptr(), unused.data_ptr(), None
            check(lib.sdy_degree_power(C.byref(a), current_stream()), "sdy_degree_power")
    return out.view(*lead, plan.lmax)


class PowerSpectrumAggregator(FieldAccumulator):
    """Per-degree power spectra of the generated and the target fields and of their difference, per variable and lead time.

    Same `record_batch` as the other inference aggregators, on the denormalised dicts: gen `(samples, time, lat, lon)` or
    member-stacked `(members, samples, time, lat, lon)`, targets `(samples, time, lat, lon)`, contiguous or the time-sliced
    views of the window driver.  A window is cut into chunks of variables; a chunk's rows are packed into one field batch
    per side (the rows of one (variable, time) consecutive, each such group padded with zero fields to a multiple of four),
    transformed with `sdy_rfft_lon` and `sdy_legendre_fwd` of the cached `ShtPlan` (its `gemm_mode` the package default) and
    reduced by ONE `sdy_degree_power` launch: three launches per side and chunk plus the packing copies.  Chunks are sized so
    that packed rows, grid-frequency tensor and both sides' coefficients stay within `max_workspace_bytes` (default
    `DEFAULT_MAX_WORKSPACE_BYTES`, 1 GiB; at 180 x 360 one variable of 25 members x 7 times takes 51 MB of generated and
    7 MB of target coefficients plus 51 MB each of packed rows and grid-frequency tensor, 160 MB in all: six variables to a
    chunk); the workspace is one grow-only buffer, reused by every window.

    Per variable, time and degree l < lmax (default: lat), float64 accumulators `(n_timesteps, lmax)` on the device add
      gen    the mean over the generated rows of P(l)          target    the mean over the target rows of P(l)
      error  the mean over the generated rows of P(l) of (gen row - its target row), from the coefficient differences.
    `get_data()` returns `{name: {"gen", "target", "error"}}`, each divided by the number of batches seen at that time and
    combined over ranks with the equal-weight `dist.reduce_mean`.  The cross spectrum of gen and target (the numerator of the
    spectral coherence) is `(gen + target - error) / 2`.  `get_logs` returns {}: no log keys are added.

    Ensembles: a member-stacked gen is POOLED over members x samples, and the error of row (member, sample) is taken against
    target row `sample` (the rule of `VideoAggregator`).  Ragged rank shares with `sample_weights` are not supported.
    The accumulators are allocated on the first batch (`max_bytes` as for the other field aggregators); they are tiny."""

    def __init__(self, n_timesteps: int, grid: str = "equiangular", lmax: Optional[int] = None, dist=None, metadata=None,
                 max_bytes: Optional[int] = None, max_workspace_bytes: Optional[int] = None):
        super().__init__(n_timesteps, dist=dist, metadata=metadata, max_bytes=max_bytes)
        self._grid = grid
        self._lmax = None if lmax is None else int(lmax)
        self._limit = DEFAULT_MAX_WORKSPACE_BYTES if max_workspace_bytes is None else int(max_workspace_bytes)
        self._ws = _Workspace()

    def _statistics(self) -> Dict[str, float]:
        return {"gen_power": 0.0, "target_power": 0.0, "err_power": 0.0}

    def _elements(self, stat: str, job: tuple) -> int:
        return self._n_timesteps * self._degrees(job)

    def _degrees(self, job: tuple) -> int:
        _, H, _ = job
        return self._lmax or H

    @property
    def workspace_bytes(self) -> int:
        """Bytes of the workspace as it stands (it only grows)."""
        return self._ws.bytes

    def _chunk(self, lay, first: int, last: int, t_start: int, device) -> None:
        """Variables first .. last - 1 (one shape): pack, transform and reduce both sides."""
        _, _, n0, n1, gs0, gs1, ts1, T, H, W = lay[first]
        nv, R = last - first, n0 * n1
        Rp, Sp = _round_up(R, 4), _round_up(n1, 4)
        Fg, Ft = nv * T * Rp, nv * T * Sp
        plan = _plan(H, W, self._lmax, None, self._grid, device)
        per_cs = plan.lmax * plan.mtr * 2
        Fx = max(Fg, Ft)
        xb, Xf, Cg, Ct, zeros = self._ws.parts(device, Fx * H * W, Fx * plan.mtr * H * 2, Fg * per_cs, Ft * per_cs, Fx)
        zeros.zero_()
        scales = []
        for side, F, rows, rows_p, Cs in (("gen", Fg, R, Rp, Cg), ("target", Ft, n1, Sp, Ct)):
            x = xb[:F * H * W].view(nv, T, rows_p, H, W)
            if rows_p != rows:
                x[:, :, rows:].zero_()
            for k in range(nv):
                v = getattr(lay[first + k], side)
                if side == "gen":
                    src = torch.as_strided(v, (n0, n1, T, H, W), (gs0, gs1, H * W, W, 1)).permute(2, 0, 1, 3, 4)
                    x[k, :, :rows].view(T, n0, n1, H, W).copy_(src)
                else:
                    src = torch.as_strided(v, (n1, T, H, W), (ts1, H * W, W, 1)).permute(1, 0, 2, 3)
                    x[k, :, :rows].copy_(src)
            scales.append(_analyse(plan, x.view(F, H, W), Xf[:F * plan.mtr * H * 2], Cs, zeros))
        a = SdySpectrumArgs()
        a.gen, a.target, a.gen_scale, a.target_scale = ptr(Cg), ptr(Ct), ptr(scales[0]), ptr(scales[1])
        a.lmax, a.mtr, a.gen_fields, a.target_fields = plan.lmax, plan.mtr, Fg, Ft
        a.gen_var_stride, a.gen_time_stride, a.target_var_stride, a.target_time_stride = T * Rp, Rp, T * Sp, Sp
        a.nvars, a.n0, a.n1, a.T, a.t_start, a.n_timesteps = nv, n0, n1, T, t_start, self._n_timesteps
        for stat in self._acc:
            setattr(a, stat, self._at(stat, first))
        check(lib.sdy_degree_power(C.byref(a), current_stream()), "sdy_degree_power")

    def _vars_per_chunk(self, l, device) -> int:
        _, _, n0, n1, _, _, _, T, H, W = l
        plan = _plan(H, W, self._lmax, None, self._grid, device)
        per_x, per_cs = _floats_per_field(plan)
        fg, ft = T * _round_up(n0 * n1, 4), T * _round_up(n1, 4)
        if fg > _MAX_FIELDS or fg * H * W > (1 << 31) - 1:
            raise ValueError(f"PowerSpectrumAggregator: one variable of a window is {fg} fields of {H} x {W}; one transform "
                             f"call takes at most {_MAX_FIELDS} fields and 2^31 - 1 grid values")
        per_var = 4 * (fg * per_x + (fg + ft) * per_cs + fg)
        n = min(max(self._limit - _SLACK, 0) // per_var, _MAX_FIELDS // fg, ((1 << 31) - 1) // (fg * H * W))
        if n < 1:
            raise ValueError(f"PowerSpectrumAggregator: one variable of a window ({fg} + {ft} fields of {H} x {W}) needs "
                             f"{per_var} bytes of workspace, more than max_workspace_bytes = {self._limit} allows")
        return n

    def _launch(self, lay, first: int, last: int, t_start: int) -> None:
        """A run of same-shaped variables (`FieldAccumulator._record`), in chunks that fit the workspace."""
        device = lay[first].gen.device
        step = self._vars_per_chunk(lay[first], device)
        for c0 in range(first, last, step):
            self._chunk(lay, c0, min(c0 + step, last), t_start, device)

    @torch.no_grad()
    def record_batch(self, loss, target_data, gen_data, target_data_norm=None, gen_data_norm=None, i_time_start: int = 0):
        del loss, target_data_norm, gen_data_norm
        self._record(target_data, gen_data, i_time_start)

    @torch.no_grad()
    def get_data(self) -> Dict[str, Dict[str, torch.Tensor]]:
        n = self._counts()[:, None]
        red = self._dist.reduce_mean
        data = {}
        for i, name in enumerate(self._names):
            shape = (self._n_timesteps, self._degrees(self._grids[i]))
            data[name] = {label: red(self._view(stat, i, *shape) / n)
                          for label, stat in (("gen", "gen_power"), ("target", "target_power"), ("error", "err_power"))}
        return data
