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

Winds: `kinetic_energy_spectrum` and `KineticEnergySpectrumAggregator` give the rotational and the divergent kinetic-energy
spectrum of a horizontal wind (u eastward, v northward).  A wind is a vector: on a latitude-longitude grid u and v are not
scalars on the sphere, and their scalar spectra neither add up to its energy spectrum nor separate rotation from divergence.
With V_theta = -v, V_lambda = u and the analyses A_D, A_M by the derivative table and the m / sin(theta) table of the plan's
vector plan (`sdy_vsht_plan_create`, `sdy_vector_legendre_fwd`; include/sdy_amd.h),

    s = A_D[V_theta] - i A_M[V_lambda]      t = A_D[V_lambda] + i A_M[V_theta]
    E_div(l) = 1/2 (|s[l,0]|^2 + 2 sum_m |s[l,m]|^2)      E_rot(l) the same of t          l < lmax

reduced by one `sdy_vector_degree_power` launch (`csrc/vector_spectrum.hip`).  sum_l (E_rot + E_div) is half the integral of
u^2 + v^2 over the unit sphere for a band-limited wind on the Legendre-Gauss grid; divide by 4 pi for a mean energy per unit
mass.  The u rows and the v rows of a side are two equal runs of ONE field batch, so one FFT and one stage call serve both.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, List, Mapping, Optional, Tuple

import torch

from ._lib import SdySpectrumArgs, SdyVectorSpectrumArgs, check, current_stream, lib, ptr
from .windows import FieldAccumulator, runs, window_layouts
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


def _fill_rows(rows, plan, gen_scale, target_scale, gen_side, target_side, nvars: int, n0: int, n1: int, T: int, t_start: int,
               n_timesteps: int) -> None:
    """The `sdy_coef_rows` of an argument structure (include/sdy_amd.h).  plan: anything with `lmax` and `mtr`; the scales:
    addresses or None; gen_side / target_side: (fields, var_stride, time_stride) of the side's coefficient tensors."""
    rows.gen_scale, rows.target_scale = gen_scale, target_scale
    rows.lmax, rows.mtr = plan.lmax, plan.mtr
    rows.gen_fields, rows.gen_var_stride, rows.gen_time_stride = gen_side
    rows.target_fields, rows.target_var_stride, rows.target_time_stride = target_side
    rows.nvars, rows.n0, rows.n1, rows.T, rows.t_start, rows.n_timesteps = nvars, n0, n1, T, t_start, n_timesteps


class _SpectrumAggregator(FieldAccumulator):
    """What `PowerSpectrumAggregator` and `KineticEnergySpectrumAggregator` share: the transform's grid and truncation, the
    grow-only workspace and its limit, the `(n_timesteps, lmax)` accumulators and `get_data`, the sizing of a chunk, and the
    chunk itself -- pack the rows of both sides, transform, fill the `sdy_coef_rows`, ONE reduction launch.  A row has
    `_COMPONENTS` fields (1: a scalar; 2: u and v); the fields of one component are one run of a side's field batch (the rows
    of one (variable, time) consecutive, each such group padded with zero fields to a multiple of four), the next component's
    an equal run behind it; a side is analysed into `_TENSORS` coefficient tensors."""

    _STATS: Tuple[Tuple[str, str], ...] = ()      # (label of get_data, field of the argument structure)
    _COMPONENTS = 1
    _TENSORS = 1
    _WORD = "variable"                            # what the refusals call one row of `_STATS` accumulators

    def __init__(self, n_timesteps: int, grid: str, lmax: Optional[int], dist, metadata, max_bytes: Optional[int],
                 max_workspace_bytes: Optional[int]):
        super().__init__(n_timesteps, dist=dist, metadata=metadata, max_bytes=max_bytes)
        self._grid = grid
        self._lmax = None if lmax is None else int(lmax)
        self._limit = DEFAULT_MAX_WORKSPACE_BYTES if max_workspace_bytes is None else int(max_workspace_bytes)
        self._ws = _Workspace()

    # -- to be provided: the transform of one side's field batch; the argument structure of one chunk
    def _analyse(self, plan: ShtPlan, x: torch.Tensor, Xf: torch.Tensor, *rest) -> torch.Tensor:
        """x (F, H, W) into the `_TENSORS` coefficient tensors (`rest`: they, then the zeros of the FFT); returns the scale."""
        raise NotImplementedError

    def _args(self, Cg: List[torch.Tensor], Ct: List[torch.Tensor], run_g: int, run_t: int):
        """(argument structure with everything but `rows` and the accumulators, name of the entry point); run_g, run_t: the
        fields of one component's run of the generated / the target side."""
        raise NotImplementedError

    def _statistics(self) -> Dict[str, float]:
        return {stat: 0.0 for _, stat in self._STATS}

    def _elements(self, stat: str, job: tuple) -> int:
        return self._n_timesteps * self._degrees(job)

    def _degrees(self, job: tuple) -> int:
        _, H, _ = job
        return self._lmax or H

    @property
    def workspace_bytes(self) -> int:
        """Bytes of the workspace as it stands (it only grows)."""
        return self._ws.bytes

    def _per_chunk(self, l, device) -> int:
        """How many variables (pairs) shaped like `l` one chunk takes."""
        n0, n1, T, H, W = l.n0, l.n1, l.T, l.H, l.W
        who, word = type(self).__name__, self._WORD
        plan = _plan(H, W, self._lmax, None, self._grid, device)
        per_x, per_cs = _floats_per_field(plan)
        fg, ft = self._COMPONENTS * T * _round_up(n0 * n1, 4), self._COMPONENTS * T * _round_up(n1, 4)
        if fg > _MAX_FIELDS or fg * H * W > (1 << 31) - 1:
            raise ValueError(f"{who}: one {word} of a window is {fg} fields of {H} x {W}; one transform call takes at most "
                             f"{_MAX_FIELDS} fields and 2^31 - 1 grid values")
        per_one = 4 * (fg * per_x + self._TENSORS * (fg + ft) * per_cs + fg)
        n = min(max(self._limit - _SLACK, 0) // per_one, _MAX_FIELDS // fg, ((1 << 31) - 1) // (fg * H * W))
        if n < 1:
            raise ValueError(f"{who}: one {word} of a window ({fg} + {ft} fields of {H} x {W}) needs {per_one} bytes of "
                             f"workspace, more than max_workspace_bytes = {self._limit} allows")
        return n

    def _chunk(self, lays, first: int, last: int, t_start: int, device) -> None:
        """Variables (pairs) first .. last - 1 (one shape) of `lays`, one list of layouts per component: pack, transform and
        reduce both sides."""
        l0 = lays[0][first]
        n0, n1, T, H, W = l0.n0, l0.n1, l0.T, l0.H, l0.W
        nv, R, k = last - first, n0 * n1, self._TENSORS
        Rp, Sp = _round_up(R, 4), _round_up(n1, 4)
        run_g, run_t = nv * T * Rp, nv * T * Sp                  # one component's run of a side; the next one's follows
        Fg, Ft = len(lays) * run_g, len(lays) * run_t
        plan = _plan(H, W, self._lmax, None, self._grid, device)
        per_cs = plan.lmax * plan.mtr * 2
        Fx = max(Fg, Ft)
        xb, Xf, *Cs, zeros = self._ws.parts(device, Fx * H * W, Fx * plan.mtr * H * 2, *[Fg * per_cs] * k, *[Ft * per_cs] * k,
                                            Fx)
        Cg, Ct = Cs[:k], Cs[k:]
        zeros.zero_()
        scales = []
        for side, F, rows, rows_p, C_side in (("gen", Fg, R, Rp, Cg), ("target", Ft, n1, Sp, Ct)):
            x = xb[:F * H * W].view(len(lays), nv, T, rows_p, H, W)
            if rows_p != rows:
                x[:, :, :, rows:].zero_()
            for c, lay in enumerate(lays):
                for j in range(nv):
                    l = lay[first + j]
                    if side == "gen":
                        src = torch.as_strided(l.gen, (n0, n1, T, H, W), (l.gs0, l.gs1, H * W, W, 1)).permute(2, 0, 1, 3, 4)
                        x[c, j, :, :rows].view(T, n0, n1, H, W).copy_(src)
                    else:
                        src = torch.as_strided(l.target, (n1, T, H, W), (l.ts1, H * W, W, 1)).permute(1, 0, 2, 3)
                        x[c, j, :, :rows].copy_(src)
            scales.append(self._analyse(plan, x.view(F, H, W), Xf[:F * plan.mtr * H * 2], *C_side, zeros))
        a, entry = self._args(Cg, Ct, run_g, run_t)
        _fill_rows(a.rows, plan, ptr(scales[0]), ptr(scales[1]), (Fg, T * Rp, Rp), (Ft, T * Sp, Sp), nv, n0, n1, T, t_start,
                   self._n_timesteps)
        for stat in self._acc:
            setattr(a, stat, self._at(stat, first))
        check(getattr(lib, entry)(C.byref(a), current_stream()), entry)

    def _run(self, lays, first: int, last: int, t_start: int) -> None:
        """A run of same-shaped variables (pairs), in chunks that fit the workspace."""
        device = lays[0][first].gen.device
        step = self._per_chunk(lays[0][first], device)
        for c0 in range(first, last, step):
            self._chunk(lays, c0, min(c0 + step, last), t_start, device)

    @torch.no_grad()
    def get_data(self) -> Dict[str, Dict[str, torch.Tensor]]:
        n = self._counts()[:, None]
        red = self._dist.reduce_mean
        data = {}
        for i, name in enumerate(self._names):
            shape = (self._n_timesteps, self._degrees(self._grids[i]))
            data[name] = {label: red(self._view(stat, i, *shape) / n) for label, stat in self._STATS}
        return data


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
            _fill_rows(a.rows, plan, ptr(scale), ptr(scale), (F, 0, 1), (F, 0, 1), 1, 1, 1, k, 0, k)
            a.gen_power, a.target_power, a.err_power = out[r0:r0 + k].data_ptr(), unused.data_ptr(), None
            check(lib.sdy_degree_power(C.byref(a), current_stream()), "sdy_degree_power")
    return out.view(*lead, plan.lmax)


class PowerSpectrumAggregator(_SpectrumAggregator):
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

    _STATS = (("gen", "gen_power"), ("target", "target_power"), ("error", "err_power"))
    _analyse = staticmethod(_analyse)

    def __init__(self, n_timesteps: int, grid: str = "equiangular", lmax: Optional[int] = None, dist=None, metadata=None,
                 max_bytes: Optional[int] = None, max_workspace_bytes: Optional[int] = None):
        super().__init__(n_timesteps, grid, lmax, dist, metadata, max_bytes, max_workspace_bytes)

    def _args(self, Cg, Ct, run_g, run_t):
        a = SdySpectrumArgs()
        a.gen, a.target = ptr(Cg[0]), ptr(Ct[0])
        return a, "sdy_degree_power"

    def _launch(self, lay, first: int, last: int, t_start: int) -> None:
        """A run of same-shaped variables (`FieldAccumulator._record`)."""
        self._run((lay,), first, last, t_start)

    @torch.no_grad()
    def record_batch(self, loss, target_data, gen_data, target_data_norm=None, gen_data_norm=None, i_time_start: int = 0):
        del loss, target_data_norm, gen_data_norm
        self._record(target_data, gen_data, i_time_start)


# ---- winds: rotational and divergent kinetic-energy spectra ------------------------------------------------------------------
class VectorShtPlan:
    """The vector plan of a cached `ShtPlan` (`sdy_vsht_plan`): the two quadrature-weighted fp32 tables of the vector Legendre
    analysis on the device.  It keeps its base plan alive; the longitude FFT stays the base plan's."""

    _cache: Dict[int, "VectorShtPlan"] = {}

    def __init__(self, base: ShtPlan):
        h = C.c_void_p()
        check(lib.sdy_vsht_plan_create(base.handle, C.byref(h)), "sdy_vsht_plan_create")
        self.handle, self.base = h, base

    @classmethod
    def get(cls, base: ShtPlan) -> "VectorShtPlan":
        """The vector plan of `base`, created on the current device (the caller is inside `torch.cuda.device`)."""
        if id(base) not in cls._cache:
            cls._cache[id(base)] = cls(base)
        return cls._cache[id(base)]

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                lib.sdy_vsht_plan_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def wind_pairs(names: Iterable[str]) -> Dict[str, Tuple[str, str]]:
    """`label -> (u_name, v_name)` of the winds among `names`, in their order: `eastward_wind_<k>` / `northward_wind_<k>` as
    `wind_<k>`, `UGRD10m` / `VGRD10m` as `wind_10m`.  A component without its partner is left out."""
    names = list(names)
    have, out = set(names), {}
    for n in names:
        if n.startswith("eastward_wind_") and "northward_wind_" + n[len("eastward_wind_"):] in have:
            k = n[len("eastward_wind_"):]
            out[f"wind_{k}"] = (n, f"northward_wind_{k}")
        elif n == "UGRD10m" and "VGRD10m" in have:
            out["wind_10m"] = ("UGRD10m", "VGRD10m")
    return out


def _vector_analyse(plan: ShtPlan, x: torch.Tensor, Xf: torch.Tensor, Cd: torch.Tensor, Cm: torch.Tensor,
                    zeros: torch.Tensor) -> torch.Tensor:
    """A_D and A_M of the fields x (F, H, W), F % 4 == 0, into Cd and Cm; returns the per-field scale to undo."""
    F = x.shape[0]
    inv, scale = _field_scales(x)
    check(lib.sdy_rfft_lon(plan.handle, ptr(x), ptr(inv), ptr(zeros), None, ptr(Xf), 1, F, current_stream()), "sdy_rfft_lon")
    check(lib.sdy_vector_legendre_fwd(VectorShtPlan.get(plan).handle, ptr(Xf), ptr(Cd), ptr(Cm), 1, F, current_stream()),
          "sdy_vector_legendre_fwd")
    return scale


@torch.no_grad()
def kinetic_energy_spectrum(u: torch.Tensor, v: torch.Tensor, grid: str = "equiangular", lmax: Optional[int] = None,
                            max_workspace_bytes: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """u, v (..., nlat, nlon) float32 on the device, eastward and northward -> {"rot", "div"} float64 (..., lmax): the
    rotational and the divergent kinetic-energy spectrum of every wind (module docstring)."""
    if not (u.is_cuda and v.is_cuda):
        raise RuntimeError("sdy_amd spectra run on the GPU only (no CPU fallback); got a CPU tensor")
    if u.dim() < 2 or tuple(u.shape) != tuple(v.shape):
        raise ValueError(f"expected u and v of one shape (..., nlat, nlon), got {tuple(u.shape)} and {tuple(v.shape)}")
    if u.device != v.device:
        raise ValueError(f"u on {u.device}, v on {v.device}")
    H, W = u.shape[-2:]
    lead = tuple(u.shape[:-2])
    ru, rv = u.reshape(-1, H, W).to(torch.float32), v.reshape(-1, H, W).to(torch.float32)
    n = ru.shape[0]
    if n < 1:
        raise ValueError("empty tensor")
    limit = DEFAULT_MAX_WORKSPACE_BYTES if max_workspace_bytes is None else int(max_workspace_bytes)
    with torch.cuda.device(u.device):
        plan = _plan(H, W, lmax, None, grid, u.device)
        per_x, per_cs = _floats_per_field(plan)
        per_wind = 2 * (per_x + 2 * per_cs + 1)                # two fields, two coefficient tensors each
        step = min(max(limit - _SLACK, 0) // (4 * per_wind) // 4 * 4, _MAX_ROWS_PER_CALL)
        if step < 4:
            raise ValueError(f"kinetic_energy_spectrum: four winds need {16 * per_wind} bytes of workspace, more than "
                             f"max_workspace_bytes = {limit}")
        rot = torch.zeros(n, plan.lmax, dtype=torch.float64, device=u.device)
        div = torch.zeros_like(rot)
        ws = _Workspace()
        for r0 in range(0, n, step):
            k = min(step, n - r0)
            Fh = _round_up(k, 4)
            F = 2 * Fh
            xb, Xf, Cd, Cm, zeros = ws.parts(u.device, F * H * W, F * plan.mtr * H * 2, F * per_cs, F * per_cs, F)
            xb = xb.view(2, Fh, H, W)
            xb[0, :k].copy_(ru[r0:r0 + k])
            xb[1, :k].copy_(rv[r0:r0 + k])
            xb[:, k:].zero_()
            zeros.zero_()
            scale = _vector_analyse(plan, xb.view(F, H, W), Xf, Cd, Cm, zeros)
            unused = torch.zeros(2, k, plan.lmax, dtype=torch.float64, device=u.device)
            a = SdyVectorSpectrumArgs()
            a.gen_d = a.target_d = ptr(Cd)
            a.gen_m = a.target_m = ptr(Cm)
            _fill_rows(a.rows, plan, ptr(scale), ptr(scale), (F, 0, 1), (F, 0, 1), 1, 1, 1, k, 0, k)
            a.gen_v_offset = a.target_v_offset = Fh
            a.gen_rot, a.gen_div = rot[r0:r0 + k].data_ptr(), div[r0:r0 + k].data_ptr()
            a.target_rot, a.target_div, a.err_rot, a.err_div = unused[0].data_ptr(), unused[1].data_ptr(), None, None
            check(lib.sdy_vector_degree_power(C.byref(a), current_stream()), "sdy_vector_degree_power")
    return {"rot": rot.view(*lead, plan.lmax), "div": div.view(*lead, plan.lmax)}


class KineticEnergySpectrumAggregator(_SpectrumAggregator):
    """Rotational and divergent kinetic-energy spectra of the generated and the target winds and of their difference, per wind
    pair and lead time (module docstring; no counterpart in the reference).

    `pairs` maps a label to `(u_name, v_name)`, eastward and northward (`wind_pairs(names)` builds it from the names of the
    headline job).  Same `record_batch` as the other field aggregators, on the denormalised dicts -- member-stacked or flat
    gen, contiguous or the time-sliced views of the window driver, `i_time_start` -- but only the paired variables are read.
    A window is cut into chunks of pairs; per side a chunk's rows are packed into ONE field batch, the u rows of every (pair,
    time) first and the v rows as a second, equal run (each group of rows padded with zero fields to a multiple of four),
    transformed with `sdy_rfft_lon` of the cached `ShtPlan` and `sdy_vector_legendre_fwd` of its vector plan (fp32 MFMA GEMM)
    and reduced by ONE `sdy_vector_degree_power` launch.  Chunks are sized so that packed rows, grid-frequency tensor and the
    two coefficient tensors of both sides stay within `max_workspace_bytes` (default `DEFAULT_MAX_WORKSPACE_BYTES`); the
    workspace is one grow-only buffer, reused by every window.

    Per pair, time and degree l < lmax (default: lat) six float64 accumulators `(n_timesteps, lmax)` on the device add the
    mean over the rows of E_rot and E_div of the generated winds, of the target winds, and of (generated row - its target
    row), taken from the coefficient differences.  `get_data()` returns `{label: {"gen_rot", "gen_div", "target_rot",
    "target_div", "error_rot", "error_div"}}`, each divided by the number of batches seen at that time and combined over ranks
    with the equal-weight `dist.reduce_mean`.  `get_logs` returns {}: no log keys are added.

    Ensembles are pooled over members x samples, the error of row (member, sample) taken against target row `sample`, as
    `PowerSpectrumAggregator` does.  `ValueError` for a pair whose variable is missing from either dict, whose u and v differ
    in shape or layout, or that names one variable twice."""

    _STATS = (("gen_rot", "gen_rot"), ("gen_div", "gen_div"), ("target_rot", "target_rot"), ("target_div", "target_div"),
              ("error_rot", "err_rot"), ("error_div", "err_div"))
    _COMPONENTS = 2                 # u and v
    _TENSORS = 2                    # A_D and A_M
    _WORD = "pair"
    _analyse = staticmethod(_vector_analyse)

    def __init__(self, pairs: Mapping[str, Tuple[str, str]], n_timesteps: int, grid: str = "equiangular",
                 lmax: Optional[int] = None, dist=None, metadata=None, max_bytes: Optional[int] = None,
                 max_workspace_bytes: Optional[int] = None):
        super().__init__(n_timesteps, grid, lmax, dist, metadata, max_bytes, max_workspace_bytes)
        self._pairs = {str(label): (str(uv[0]), str(uv[1])) for label, uv in dict(pairs).items()}
        if not self._pairs:
            raise ValueError("KineticEnergySpectrumAggregator: no wind pairs")
        for label, (un, vn) in self._pairs.items():
            if un == vn:
                raise ValueError(f"wind pair {label!r} names {un!r} twice")

    def _args(self, Cg, Ct, run_g, run_t):
        a = SdyVectorSpectrumArgs()
        a.gen_d, a.gen_m, a.target_d, a.target_m = ptr(Cg[0]), ptr(Cg[1]), ptr(Ct[0]), ptr(Ct[1])
        a.gen_v_offset, a.target_v_offset = run_g, run_t           # the u run of a side; its v run follows
        return a, "sdy_vector_degree_power"

    def _layouts(self, target_data, gen_data):
        """The `WindowLayout`s of the u and of the v variables, pair by pair, everything checked."""
        for label, (un, vn) in self._pairs.items():
            for name in (un, vn):
                if name not in gen_data or name not in target_data:
                    raise ValueError(f"wind pair {label!r}: no {'generated' if name not in gen_data else 'target'} "
                                     f"variable {name!r}")
        lay_u = window_layouts({k: target_data[un] for k, (un, _) in self._pairs.items()},
                               {k: gen_data[un] for k, (un, _) in self._pairs.items()})
        lay_v = window_layouts({k: target_data[vn] for k, (_, vn) in self._pairs.items()},
                               {k: gen_data[vn] for k, (_, vn) in self._pairs.items()})
        for (label, (un, vn)), a, b in zip(self._pairs.items(), lay_u, lay_v):
            if gen_data[un].dim() != gen_data[vn].dim() or self._extents(a) != self._extents(b):
                raise ValueError(f"wind pair {label!r}: {un!r} {tuple(gen_data[un].shape)} and {vn!r} "
                                 f"{tuple(gen_data[vn].shape)} differ in shape or layout")
        if lay_v[0].T != lay_u[0].T:
            raise ValueError("the variables of one window differ in their number of times")
        return lay_u, lay_v

    @staticmethod
    def _extents(l) -> tuple:
        return (l.n0, l.n1, l.T, l.H, l.W)

    @torch.no_grad()
    def record_batch(self, loss, target_data, gen_data, target_data_norm=None, gen_data_norm=None, i_time_start: int = 0):
        del loss, target_data_norm, gen_data_norm
        i_time_start = int(i_time_start)
        lay_u, lay_v = self._layouts(target_data, gen_data)
        T = lay_u[0].T
        if i_time_start < 0 or i_time_start + T > self._n_timesteps:
            raise ValueError(f"times {i_time_start}..{i_time_start + T - 1} outside the aggregator's {self._n_timesteps}")
        if not all(l.gen.is_cuda and l.target.is_cuda for l in lay_v):
            raise RuntimeError("sdy_amd aggregators run on the GPU only (no CPU fallback)")
        first_device = lay_u[0].gen.device
        for l in lay_v:
            if l.gen.device != first_device or l.target.device != first_device:
                raise ValueError(f"tensors on {l.gen.device} / {l.target.device}, the pair's u on {first_device}")
        device = self._prepare(list(self._pairs), lay_u)
        with torch.cuda.device(device):
            for first, last in runs(lay_u, self._extents):
                self._run((lay_u, lay_v), first, last, i_time_start)
        for t in range(i_time_start, i_time_start + T):
            self._n_batches[t] += 1
