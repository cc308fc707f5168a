"""Scores of a forecast AS A FIELD, on the device: the energy score (the multivariate sibling of the CRPS), the member-to-truth
and member-to-member distances of whole fields and the anomaly (pattern) correlation, all read from one small object per
(variable, sample, lead time): the area-weighted Gram matrix of the member errors and the truth anomaly, formed by ONE
`sdy_member_gram` launch per window (include/sdy_amd.h, csrc/member_gram.h).  No counterpart in the reference.

With members g_0 .. g_{M-1}, target y, area weights w (non-negative, not normalised) and an optional climatology c (absent:
0), N = M + 2 float64 vectors over the grid points:

    a_0 = 1        a_{1+m} = g_m - y        a_{M+1} = y - c        Gamma[i][j] = sum_p w(p) a_i(p) a_j(p)

The errors, not the fields, enter the Gram: their differences are exact in float64, and a squared distance formed as Gamma_ii
+ Gamma_jj - 2 Gamma_ij does not cancel the magnitude of the field itself.

Zero-weight rule: a grid point whose weight is exactly 0 contributes nothing, NaN and Inf included; anywhere else a NaN
propagates into the entries of its own row and column only (a NaN in member m: index 1 + m).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Mapping, Optional, Tuple

import torch

from ._lib import SDY_GRAM_MAX_MEMBERS, SdyMemberGramArgs, check, current_stream, lib, ptr
from .windows import TorchDistributed, fill_window, runs, whole_ics_message, window_layouts

SCORES = ("error_distance", "energy_score", "ensemble_mean_rmse")
SCORES_ENSEMBLE = ("member_distance", "distance_ratio")


def gram_index(i: int, j: int, N: int) -> int:
    """Entry (i, j), 0 <= i <= j < N, of the packed upper triangle (`sdy_gram_index`, csrc/member_gram.h)."""
    return i * N - i * (i - 1) // 2 + (j - i)


def unpack(packed: torch.Tensor, N: int) -> torch.Tensor:
    """(..., N (N + 1) / 2) packed upper triangles -> (..., N, N) symmetric matrices."""
    if packed.shape[-1] != N * (N + 1) // 2:
        raise ValueError(f"{packed.shape[-1]} entries are not the upper triangle of a {N} x {N} matrix")
    i, j = torch.triu_indices(N, N, device=packed.device)        # row-major in (i, j >= i): the packed order
    full = packed.new_zeros(*packed.shape[:-1], N, N)
    full[..., i, j] = packed
    full[..., j, i] = packed
    return full


def _correlation(var_y, cov_ey, var_e):
    """Centred correlation of f' = y' + e with y'; NaN where a variance is not positive."""
    var_f = var_y + 2.0 * cov_ey + var_e
    ok = (var_y > 0.0) & (var_f > 0.0)
    r = (var_y + cov_ey) / (var_f * var_y).sqrt()
    return torch.where(ok, r, torch.full_like(r, float("nan")))


def scores(gram: torch.Tensor, M: int, climatology: bool = False) -> Dict[str, torch.Tensor]:
    """The field scores of `(..., N, N)` symmetric float64 Gram matrices, N = M + 2; a pure function of torch operations, on
    any device.  With Wt = Gamma_00, D = Gamma[1..M, 1..M] / Wt (the members' error covariance about the truth) and the truth
    row likewise divided:

    - `error_distance`: mean_m sqrt(D_mm), the members' mean RMS distance to the truth
    - `member_distance`: mean_{i<j} sqrt(max(D_ii + D_jj - 2 D_ij, 0)); NaN for M = 1
    - `energy_score`: error_distance - member_distance / 2 (the fair estimator); for M = 1 error_distance
    - `distance_ratio`: member_distance / error_distance: 1 when the truth is exchangeable with the members, below 1 for an
      ensemble that is under-dispersive as fields; NaN at 0 / 0
    - `ensemble_mean_rmse`: sqrt(mean_ij D_ij) (`MeanAggregator`'s `weighted_rmse`)
    - `anomaly_correlation` (of the ensemble mean) and `anomaly_correlation_member_avg` (the mean of the members' own): the
      centred correlation of y' + e with y' = y - c, every moment from Gamma; NaN where a variance is 0.  With
      `climatology=False` the Gram was formed with c = 0 and the keys are `pattern_correlation[_member_avg]`."""
    N = M + 2
    if M < 1 or tuple(gram.shape[-2:]) != (N, N):
        raise ValueError(f"{tuple(gram.shape)} is not (..., {N}, {N}) for {M} members")
    g = gram.double()
    wt = g[..., 0, 0]
    D = g[..., 1:M + 1, 1:M + 1] / wt[..., None, None]
    b = g[..., 0, 1:M + 1] / wt[..., None]                        # the mean error of every member
    ty = g[..., 0, M + 1] / wt                                    # the truth anomaly: mean, second moment, with the errors
    tyy = g[..., M + 1, M + 1] / wt
    tey = g[..., 1:M + 1, M + 1] / wt[..., None]
    d = torch.diagonal(D, dim1=-2, dim2=-1)
    out = {"error_distance": d.sqrt().mean(dim=-1)}
    if M > 1:
        i, j = torch.triu_indices(M, M, offset=1, device=g.device)
        pair = (d[..., i] + d[..., j] - 2.0 * D[..., i, j]).clamp_min(0.0).sqrt()
        out["member_distance"] = pair.mean(dim=-1)
        out["energy_score"] = out["error_distance"] - 0.5 * out["member_distance"]
    else:
        out["member_distance"] = torch.full_like(wt, float("nan"))
        out["energy_score"] = out["error_distance"].clone()
    out["distance_ratio"] = out["member_distance"] / out["error_distance"]
    mean_D = D.mean(dim=(-2, -1))
    out["ensemble_mean_rmse"] = mean_D.sqrt()
    var_y = tyy - ty * ty
    key = "anomaly_correlation" if climatology else "pattern_correlation"
    bm = b.mean(dim=-1)
    out[key] = _correlation(var_y, tey.mean(dim=-1) - bm * ty, mean_D - bm * bm)
    out[key + "_member_avg"] = _correlation(var_y[..., None], tey - b * ty[..., None], d - b * b).mean(dim=-1)
    return out


def _workspace(nvars: int, n0: int, n1: int, T: int, HW: int, device) -> torch.Tensor:
    ws_bytes = lib.sdy_member_gram_workspace_bytes(nvars, n0, n1, T, HW)
    if ws_bytes == 0:
        raise ValueError(f"sdy_member_gram takes 1..{SDY_GRAM_MAX_MEMBERS} members, got {n0}")
    return torch.empty(ws_bytes // 8, dtype=torch.float64, device=device)


def _launch(lay, first: int, last: int, weights: torch.Tensor, clim, out: torch.Tensor, ws: torch.Tensor) -> None:
    """One `sdy_member_gram` launch for the run of same-shaped variables first .. last - 1; `clim`: per variable a device
    tensor or None."""
    a = SdyMemberGramArgs()
    fill_window(a.win, lay, first, last)
    a.HW, a.weights = lay[first].H * lay[first].W, ptr(weights)
    for k in range(first, last):
        a.climatology[k - first] = ptr(clim[k])
    a.out, a.ws, a.ws_bytes = ptr(out), ptr(ws), ws.numel() * 8
    check(lib.sdy_member_gram(C.byref(a), current_stream()), "sdy_member_gram")


def _device_map(x: torch.Tensor, device) -> torch.Tensor:
    return x.detach().to(device=device, dtype=torch.float32).contiguous()


@torch.no_grad()
def member_gram(target: torch.Tensor, gen: torch.Tensor, area_weights: torch.Tensor,
                climatology: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The Gram matrices of one field: `target` (samples, time, lat, lon), `gen` the same or member-stacked (members, samples,
    time, lat, lon), `area_weights` and the optional `climatology` (lat, lon) -> (samples, time, N, N) symmetric float64 on the
    device, N = members + 2 (see the module).  Useful on its own: the eigenvalues of the centred member block are the
    ensemble's own EOF spectrum."""
    lay = window_layouts({"x": target}, {"x": gen})
    l = lay[0]
    if not (l.gen.is_cuda and l.target.is_cuda):
        raise RuntimeError("sdy_amd aggregators run on the GPU only (no CPU fallback)")
    device = l.gen.device
    for what, m in (("area_weights", area_weights), ("climatology", climatology)):
        if m is not None and tuple(m.shape) != (l.H, l.W):
            raise ValueError(f"{what} {tuple(m.shape)} against a {(l.H, l.W)} grid")
    if l.n0 > SDY_GRAM_MAX_MEMBERS:
        raise ValueError(f"at most {SDY_GRAM_MAX_MEMBERS} members, got {l.n0}")
    N = l.n0 + 2
    w = _device_map(area_weights, device)
    c = None if climatology is None else _device_map(climatology, device)
    out = torch.empty(l.n1, l.T, N * (N + 1) // 2, dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        _launch(lay, 0, 1, w, [c], out, _workspace(1, l.n0, l.n1, l.T, l.H * l.W, device))
    return unpack(out, N)


class FieldScoreAggregator:
    """Per-lead-time series of the field scores (`scores`) of every variable.

    Same `record_batch(loss, target_data, gen_data, target_data_norm, gen_data_norm, i_time_start)` and bookkeeping as
    `MeanAggregator`: the mean over a window's samples is added at `i_time_start ...`, divided at read-out by the number of
    windows that touched a time index and averaged over ranks (`dist.reduce_mean`).  The initial condition is counted like any
    time: its distances are exactly 0 and its ratios NaN.  `is_ensemble=True` needs member-stacked `(members, samples, time,
    lat, lon)` predictions and refuses flat rows; it adds `member_distance`, `distance_ratio` and the `_member_avg`
    correlation to `error_distance`, `energy_score`, `ensemble_mean_rmse` and the correlation of the ensemble mean.

    `climatology`: a mapping from variable to a `(lat, lon)` tensor, uploaded once; its variables report
    `anomaly_correlation[_member_avg]`, the others `pattern_correlation[_member_avg]` (the same formula with c = 0).  Any
    other shape raises `ValueError`, and so does a name that is not a generated variable of the first window.

    Per window: one `sdy_member_gram` launch per run of same-shaped variables (normally one) reads the member-stacked view in
    place and writes the packed Gram of every (variable, sample, time); `scores` runs on that small tensor for all variables
    at once.  The first accepted window fixes variables, grids, member count and sample count; a refused window changes
    nothing.

    `get_series()` -> `{"<metric>/<variable>": (n_timesteps,) float64}`; `get_logs(label)` -> `{f"{label}/series": ...}` with
    numpy arrays."""

    def __init__(self, area_weights: torch.Tensor, n_timesteps: int, is_ensemble: bool = False,
                 climatology: Optional[Mapping[str, torch.Tensor]] = None, target: str = "denorm", dist=None):
        if target not in ("norm", "denorm"):
            raise ValueError(f"target must be 'norm' or 'denorm', got {target!r}")
        if int(n_timesteps) < 1:
            raise ValueError(f"n_timesteps must be positive, got {n_timesteps}")
        if area_weights.dim() != 2:
            raise ValueError(f"area_weights must be (lat, lon), got {tuple(area_weights.shape)}")
        self._area = area_weights
        self._climatology = dict(climatology or {})
        for name, c in self._climatology.items():
            if not isinstance(c, torch.Tensor) or tuple(c.shape) != tuple(area_weights.shape):
                raise ValueError(f"climatology of {name!r}: expected a {tuple(area_weights.shape)} tensor, got "
                                 f"{tuple(getattr(c, 'shape', ()))}")
        self._target = target
        self._n_timesteps = int(n_timesteps)
        self.is_ensemble = bool(is_ensemble)
        self._dist = TorchDistributed() if dist is None else dist
        self._names: Optional[List[str]] = None
        self._jobs: Optional[List[tuple]] = None
        self._keys: List[List[str]] = []                         # per variable the score behind each metric row
        self._weights: Optional[torch.Tensor] = None
        self._clim: List[Optional[torch.Tensor]] = []
        self._total: Optional[torch.Tensor] = None               # (metrics, nvars, n_timesteps) float64
        self._n_batches: Optional[torch.Tensor] = None           # (n_timesteps,) int32
        self._buffers: Dict[tuple, Tuple[torch.Tensor, torch.Tensor]] = {}

    @property
    def metric_names(self) -> List[str]:
        """The rows of the accumulator; `correlation` is spelled per variable (`_metric_key`)."""
        return list(SCORES + (SCORES_ENSEMBLE if self.is_ensemble else ()) + ("correlation",)
                    + (("correlation_member_avg",) if self.is_ensemble else ()))

    def _metric_key(self, metric: str, name: str) -> str:
        if metric.startswith("correlation"):
            return ("anomaly_" if name in self._climatology else "pattern_") + metric
        return metric

    def _grams(self, lay, device, weights, clim) -> torch.Tensor:
        """The window's packed Grams (nvars, n1, T, entries): one launch per run of same-shaped variables."""
        l = lay[0]
        N = l.n0 + 2
        key = (device, len(lay), l.n0, l.n1, l.T)
        if key not in self._buffers:
            self._buffers[key] = (torch.empty(len(lay), l.n1, l.T, N * (N + 1) // 2, dtype=torch.float64, device=device),
                                  _workspace(min(len(lay), 96), l.n0, l.n1, l.T, l.H * l.W, device))
        out, ws = self._buffers[key]
        with torch.cuda.device(device):
            for first, last in runs(lay, lambda x: x.extents):
                _launch(lay, first, last, weights, clim, out[first:last], ws)
        return out

    @torch.no_grad()
    def record_batch(self, loss, target_data, gen_data, target_data_norm=None, gen_data_norm=None, i_time_start: int = 0):
        del loss
        if self._target == "norm":
            target_data, gen_data = target_data_norm, gen_data_norm
        if any(g.dim() != (5 if self.is_ensemble else 4) for g in gen_data.values()):
            if self.is_ensemble:
                raise ValueError(whole_ics_message("FieldScoreAggregator(is_ensemble=True)"))
            raise ValueError("FieldScoreAggregator(is_ensemble=False) takes (samples, time, lat, lon) predictions")
        lay = window_layouts(target_data, gen_data)
        names, i_time_start, T = list(gen_data), int(i_time_start), lay[0].T
        if i_time_start < 0 or i_time_start + T > self._n_timesteps:
            raise ValueError(f"times {i_time_start}..{i_time_start + T - 1} outside the aggregator's {self._n_timesteps}")
        jobs = [(l.n0, l.n1, l.H, l.W) for l in lay]
        if self._names is not None and (names != self._names or jobs != self._jobs):
            raise ValueError("the variables, member count, sample count or grids of a window differ from the first window's")
        for l in lay:
            if (l.H, l.W) != tuple(self._area.shape) or (l.n0, l.n1) != (lay[0].n0, lay[0].n1):
                raise ValueError(f"a {(l.H, l.W)} grid with {l.n0} members and {l.n1} samples against area weights on "
                                 f"{tuple(self._area.shape)}, {lay[0].n0} members and {lay[0].n1} samples")
            if l.n0 > SDY_GRAM_MAX_MEMBERS:
                raise ValueError(f"at most {SDY_GRAM_MAX_MEMBERS} members, got {l.n0}")
        unknown = [k for k in self._climatology if k not in gen_data]
        if unknown:
            raise ValueError(f"climatology of {unknown}: not generated variables ({names})")
        if not all(l.gen.is_cuda and l.target.is_cuda for l in lay):
            raise RuntimeError("sdy_amd aggregators run on the GPU only (no CPU fallback)")
        device = lay[0].gen.device if self._total is None else self._total.device
        if any(l.gen.device != device or l.target.device != device for l in lay):
            raise ValueError(f"tensors of a window on another device than {device}")

        first_window = self._total is None
        weights = _device_map(self._area, device) if first_window else self._weights
        clim = ([_device_map(self._climatology[k], device) if k in self._climatology else None for k in names]
                if first_window else self._clim)
        M = lay[0].n0
        sc = scores(unpack(self._grams(lay, device, weights, clim), M + 2), M)          # every score (nvars, n1, T)
        rows = [sc[m] for m in SCORES + (SCORES_ENSEMBLE if self.is_ensemble else ())] + [sc["pattern_correlation"]]
        if self.is_ensemble:
            rows.append(sc["pattern_correlation_member_avg"])
        window = torch.stack(rows).mean(dim=2)                                         # mean over the window's samples
        if first_window:
            self._names, self._jobs, self._weights, self._clim = names, jobs, weights, clim
            self._total = torch.zeros(len(rows), len(names), self._n_timesteps, dtype=torch.float64, device=device)
            self._n_batches = torch.zeros(self._n_timesteps, dtype=torch.int32, device=device)
        self._total[..., i_time_start:i_time_start + T] += window
        self._n_batches[i_time_start:i_time_start + T] += 1

    @torch.no_grad()
    def get_series(self) -> Dict[str, torch.Tensor]:
        if self._total is None:
            raise ValueError("No batches have been recorded.")
        series = self._dist.reduce_mean(self._total / self._n_batches)
        return {f"{self._metric_key(metric, name)}/{name}": series[m, v]
                for m, metric in enumerate(self.metric_names) for v, name in enumerate(self._names)}

    @torch.no_grad()
    def get_logs(self, label: str):
        series = self.get_series()
        host = torch.stack(list(series.values())).cpu().numpy()                       # one copy for all series
        data = {k: host[i] for i, k in enumerate(series)}
        return {f"{label}/series": data}
