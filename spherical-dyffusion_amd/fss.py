"""Neighbourhood verification of threshold events on the device: the fractions skill score (FSS) as a function of the
neighbourhood's size.  The reference has nothing of the kind.

Point by point (`sdy_amd.events`) a rain band forecast one grid cell off is punished twice, once as a miss and once as a false
alarm, so a sharper member scores worse than a smooth one: the double penalty.  Here the fraction of a neighbourhood that is in
the event is compared instead -- the ensemble's fraction F = K / (M n) against the truth's Of = O / n, with K, O the box sums
of the members and of the truth in the event over the n points of the neighbourhood -- and the skill is read as a function of
the radius.  The device accumulates six integers per row (count, sum K, sum O, sum K^2, sum K O, sum O^2) exactly; every score
is a few float64 operations on them at read-out (`scores`).

Out of scope: per-member FSS (box sums per member), neighbourhoods in kilometres or of equal area, events over several
variables, plots.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import torch

from ._lib import SDY_FSS_MAX_RADII, SdyFssArgs, check, current_stream, lib
from .events import EventAccumulator, Events
from .windows import runs

#: what `FractionsSkillAggregator.get_logs` reports per variable, event and radius, in this order
LOG_METRICS = ("fss", "fbs", "base_rate", "fss_useful", "counted_fraction")
#: what `get_data` reports per slot, in this order (after `sums`)
SLOT_METRICS = ("fss", "fbs", "base_rate", "forecast_rate", "fss_useful", "counted_fraction")
#: the six sums of a row, in accumulator order
TERMS = ("count", "sum_k", "sum_o", "sum_kk", "sum_ko", "sum_oo")

DEFAULT_WORKSPACE_BYTES = 256 << 20


def neighbourhood_sizes(H: int, radii: Sequence[int]) -> torch.Tensor:
    """n(lat, r) = (2r + 1) (min(H - 1, lat + r) - max(0, lat - r) + 1) as a float64 `(len(radii), H)` tensor: the grid points
    of a neighbourhood whose longitudes wrap and whose latitudes are clipped at the poles."""
    lat = torch.arange(H, dtype=torch.float64)
    r = torch.as_tensor(list(radii), dtype=torch.float64)[:, None]
    return (2 * r + 1) * (torch.clamp(lat + r, max=H - 1) - torch.clamp(lat - r, min=0) + 1)


def scores(sums: torch.Tensor, M: int, radii: Sequence[int], lat_weights: torch.Tensor,
           centres: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """The scores of the sums `(..., radius, lat, 6)` -- per row the count of its counted centres and the sums of K, O, K^2,
    K O and O^2 over them -- of an M-member ensemble under `(lat,)` weights; float64 on the sums' device, CPU included.

    With n = n(lat, r) (`neighbourhood_sizes`), F = K / (M n) and Of = O / n:
    num = sum_lat w (sum K^2 / M^2 - 2 sum K O / M + sum O^2) / n^2 (the weighted sum of (F - Of)^2),
    ref = sum_lat w (sum K^2 / M^2 + sum O^2) / n^2, cnt = sum_lat w count;
    `fss` = 1 - num / ref, NaN when ref = 0;  `fbs` = num / cnt;  `base_rate` = sum_lat w sum O / n / cnt;  `forecast_rate` =
    sum_lat w sum K / (M n) / cnt;  `fss_useful` = 0.5 + base_rate / 2, the value above which a forecast is commonly called
    useful;  `counted_fraction` = cnt / (sum_lat w x centres), where `centres` `(...)` is the number of centres a row has seen,
    counted or not (planes added x longitudes: the caller's bookkeeping); NaN without it.  Everything is `(..., radius)`.
    Without counts everything is NaN."""
    t = sums.to(torch.float64)
    w = lat_weights.to(device=t.device, dtype=torch.float64)
    radii = [int(r) for r in radii]
    if t.dim() < 3 or t.shape[-1] != 6 or t.shape[-2] != w.numel() or t.shape[-3] != len(radii):
        raise ValueError(f"sums are (..., radius, lat, 6) with (lat,) weights, got {tuple(t.shape)}, {len(radii)} radii and "
                         f"{tuple(w.shape)}")
    n = neighbourhood_sizes(t.shape[-2], radii).to(t.device)                       # (radius, lat)
    count, k, o, kk, ko, oo = t.unbind(dim=-1)
    m = float(M)
    num = (w * (kk / (m * m) - 2.0 * ko / m + oo) / (n * n)).sum(dim=-1)
    ref = (w * (kk / (m * m) + oo) / (n * n)).sum(dim=-1)
    cnt = (w * count).sum(dim=-1)
    nan = torch.full_like(cnt, float("nan"))
    some = cnt > 0
    safe = torch.where(some, cnt, torch.ones_like(cnt))
    base = torch.where(some, (w * o / n).sum(dim=-1) / safe, nan)
    out = {"fss": torch.where(some & (ref > 0), 1.0 - num / torch.where(ref > 0, ref, torch.ones_like(ref)), nan),
           "fbs": torch.where(some, num / safe, nan), "base_rate": base,
           "forecast_rate": torch.where(some, (w * k / (m * n)).sum(dim=-1) / safe, nan), "fss_useful": 0.5 + base / 2.0}
    if centres is None:
        out["counted_fraction"] = nan
    else:
        seen = w.sum() * torch.as_tensor(centres, dtype=torch.float64, device=t.device)[..., None]
        out["counted_fraction"] = torch.where(some & (seen > 0), cnt / torch.where(seen > 0, seen, torch.ones_like(seen)), nan)
    return out


class FractionsSkillAggregator(EventAccumulator):
    """Per variable, event, lead time, radius and latitude: the six integer sums behind the fractions skill score of an
    ensemble's event probabilities -- and the scores that follow from them.

    Definition (csrc/fss.h; events and counted points are those of `EventVerificationAggregator`, csrc/events.h).  For one
    (variable, sample, time, event) a grid point q has c(q) = 1 when it is counted (neither its target nor its threshold is
    NaN), k(q) = the members in the event and o(q) = 1 when the truth is in it, both 0 where c = 0.  The neighbourhood of radius
    r of a centre (lat, lon) is the points (lat', (lon + d) mod W) with |lat' - lat| <= r, 0 <= lat' < H and |d| <= r: longitude
    wraps, latitude is clipped at the poles.  It is measured in GRID POINTS, not kilometres, as FSS on a lat-lon grid usually
    is: towards the poles the same radius spans less distance east-west.  n(lat, r) = (2r + 1) (min(H - 1, lat + r) - max(0, lat
    - r) + 1); K, O, C are the sums of k, o, c over the neighbourhood.  A centre is counted when C = n(lat, r): when every point
    of its neighbourhood is counted.  A NaN target or a NaN in a threshold map therefore removes the centres within r of it (it
    is never read as "not in the event"), which makes the denominator of a fraction a function of (lat, r) alone and keeps
    every accumulated number an integer.  The consequence: for an ocean-only field with NaN over land, coastal centres drop out
    as r grows (`counted_fraction` says how many are left).  A NaN member is simply not in the event.

    `radii`: 1 .. 4 integers, strictly ascending, 0 allowed (the point-by-point limit: `fbs` is then the Brier score of
    `EventVerificationAggregator`); 2r + 1 may not exceed the number of longitudes, and M (2 r_max + 1)^2 may not exceed 65535
    (M = 64 allows r <= 15, M = 25 r <= 25).

    `record_batch(loss, target_data, gen_data, target_data_norm, gen_data_norm, i_time_start)` is what `run_inference` calls
    once per window: targets `(samples, time, lat, lon)`, gen `(members, samples, time, lat, lon)` (a 4-D gen is one member).
    Only the variables with events are read.  One `sdy_fss_accumulate` call per run of variables with equal extents and equal
    event count -- cut into chunks of variables so that the 16-bit code workspace (2 bytes per variable, sample, time, event and
    grid point) stays within `workspace_bytes` -- reads the window once, in place, and adds it to float64 sums `(n_slots,
    events, radii, lat, 6)` per variable on the device.  The thresholds go to the device once, at the first accepted window.
    Slots, `pool_times`, the uncounted first time of a run, the first window fixing the job, refused windows changing nothing
    and ragged shares being refused: as for `EventVerificationAggregator`.  The sums are integers held as float64: the same
    bits in any layout, batch, chunking, run and rank count, exact while a row's sums stay below 2^53 (above that they round;
    one call's contribution is checked, the total is not).

    `get_data()` returns float64 device tensors, added over ranks (`dist.reduce_sum`), per variable, event and radius:
    `sums_r<radius>/<event>/<var>` `(n_slots, lat, 6)` (`TERMS`) and `fss_r<radius>`, `fbs_r<radius>`, `base_rate_r<radius>`,
    `forecast_rate_r<radius>`, `fss_useful_r<radius>` and `counted_fraction_r<radius>` `(n_slots,)` (see `scores`).
    `get_logs(label)` returns Python floats from the sums pooled over all slots, `<metric>_r<radius>/<event>/<variable>` for
    the metrics of `LOG_METRICS`."""

    def __init__(self, events: Events, radii: Sequence[int], area_weights: torch.Tensor, n_timesteps: int,
                 pool_times: bool = False, dist=None, metadata=None, max_bytes: Optional[int] = None,
                 workspace_bytes: int = DEFAULT_WORKSPACE_BYTES):
        super().__init__(events, area_weights, n_timesteps, pool_times=pool_times, dist=dist, metadata=metadata,
                         max_bytes=max_bytes)
        radii = list(radii)
        if not 1 <= len(radii) <= SDY_FSS_MAX_RADII or any(int(r) != r or r < 0 for r in radii) or \
                any(b <= a for a, b in zip(radii, radii[1:])):
            raise ValueError(f"radii are 1 .. {SDY_FSS_MAX_RADII} non-negative integers, strictly ascending, got {radii!r}")
        if workspace_bytes < 1:
            raise ValueError(f"workspace_bytes must be positive, got {workspace_bytes}")
        self._radii = [int(r) for r in radii]
        self._workspace_bytes = int(workspace_bytes)
        self._ws: Optional[torch.Tensor] = None
        self._planes = [0] * self._n_slots               # per slot the (sample, time) planes added on this rank

    def _statistics(self) -> Dict[str, float]:
        return {"sums": 0.0}

    def _elements(self, stat: str, job: tuple) -> int:
        _, _, H, _, E = job
        return self._n_slots * E * len(self._radii) * H * 6

    def _size_words(self, names, jobs) -> str:
        return (f"{sum(j[4] for j in jobs)} events of {len(names)} variables, {len(self._radii)} radii x {self._n_slots} "
                f"slots")

    @staticmethod
    def _code_bytes(l) -> int:
        """The workspace one variable of a window takes (`sdy_fss_workspace_bytes` of one variable)."""
        return int(lib.sdy_fss_workspace_bytes(1, l.n_events, l.n1, l.T, l.H, l.W))

    def _check_window(self, lay) -> None:
        r = self._radii[-1]
        for l in lay:
            if 2 * r + 1 > l.W:
                raise ValueError(f"radius {r}: a neighbourhood of {2 * r + 1} longitudes on a grid of {l.W}")
            if l.n0 * (2 * r + 1) ** 2 > 65535:
                raise ValueError(f"{l.n0} members x (2 x {r} + 1)^2 points exceed 65535: the box sums would not fit 16 bits")
            need = self._code_bytes(l)
            if need == 0 or need > self._workspace_bytes:
                raise ValueError(f"one variable's codes need {need or 'more than 2^50'} bytes, more than workspace_bytes = "
                                 f"{self._workspace_bytes}")

    def _args(self, lay, first: int, last: int, t0: int, i_time_start: int) -> SdyFssArgs:
        a = SdyFssArgs()
        self._fill(a, lay, first, last, t0, i_time_start)
        a.n_radii = len(self._radii)
        for j, r in enumerate(self._radii):
            a.radii[j] = r
        a.acc = self._at("sums", first)
        a.ws, a.ws_bytes = self._ws.data_ptr(), self._ws.numel()
        return a

    def _chunks(self, lay):
        """(first, last) of what one call takes: a run of variables with equal extents and event count, cut so that its codes
        fit the workspace."""
        for first, last in runs(lay, lambda l: (l.extents, l.n_events)):
            step = max(1, self._workspace_bytes // self._code_bytes(lay[first]))
            for at in range(first, last, step):
                yield at, min(at + step, last)

    @torch.no_grad()
    def record_batch(self, loss, target_data, gen_data, target_data_norm=None, gen_data_norm=None, i_time_start: int = 0,
                     sample_weights: Optional[Sequence[float]] = None):
        del loss, target_data_norm, gen_data_norm
        i_time_start = int(i_time_start)
        lay, t0, device = self._begin(target_data, gen_data, i_time_start, sample_weights)
        chunks = list(self._chunks(lay))
        need = max((last - first) * self._code_bytes(lay[first]) for first, last in chunks)
        with torch.cuda.device(device):
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=device)
            for first, last in chunks:
                a = self._args(lay, first, last, t0, i_time_start)
                check(lib.sdy_fss_accumulate(C.byref(a), current_stream()), "sdy_fss_accumulate")
        for t in range(i_time_start + t0, i_time_start + lay[0].T):
            self._n_batches[t] += 1
            self._planes[0 if self._pool_times else t] += lay[0].n1

    def _sums(self, acc: Dict[str, torch.Tensor], i: int) -> torch.Tensor:
        """-> the (n_slots, E, radii, lat, 6) sums of variable i inside the flat (reduced) buffer."""
        _, _, H, _, E = self._grids[i]
        n = self._n_slots * E * len(self._radii) * H * 6
        at = self._offsets["sums"][i]
        return acc["sums"][at:at + n].view(self._n_slots, E, len(self._radii), H, 6)

    def _centres(self, device) -> List[torch.Tensor]:
        """Per variable the centres a row has seen per slot, added over ranks: planes x longitudes."""
        planes = self._dist.reduce_sum(torch.tensor(self._planes, dtype=torch.float64, device=device))
        return [planes * self._grids[i][3] for i in range(len(self._names))]

    @torch.no_grad()
    def get_data(self) -> Dict[str, torch.Tensor]:
        acc = self._reduced()
        centres = self._centres(acc["sums"].device)
        data: Dict[str, torch.Tensor] = {}
        for i, name in enumerate(self._names):
            M = self._grids[i][0]
            sums = self._sums(acc, i)
            w = self._lat_weights(i, sums.device)
            for e, event in enumerate(self._events[name]):
                s = scores(sums[:, e], M, self._radii, w, centres[i])
                for j, r in enumerate(self._radii):
                    tail = f"_r{r}/{event.name}/{name}"
                    data["sums" + tail] = sums[:, e, j]
                    for metric in SLOT_METRICS:
                        data[metric + tail] = s[metric][:, j]
        return data

    @torch.no_grad()
    def get_logs(self, label: str) -> Dict[str, float]:
        acc = self._reduced()
        centres = self._centres(acc["sums"].device)
        parts = [self._sums(acc, i).sum(dim=0).reshape(-1) for i in range(len(self._names))]      # (E, radii, lat, 6) each
        packed = torch.cat(parts + [torch.stack([c.sum() for c in centres])]).cpu()               # one copy for everything
        seen = packed[-len(self._names):]
        logs: Dict[str, float] = {}
        at = 0
        for i, name in enumerate(self._names):
            M, H = self._grids[i][0], self._grids[i][2]
            w = self._lat_weights(i, packed.device)
            n = len(self._radii) * H * 6
            for event in self._events[name]:
                s = scores(packed[at:at + n].view(len(self._radii), H, 6), M, self._radii, w, seen[i])
                at += n
                for j, r in enumerate(self._radii):
                    for metric in LOG_METRICS:
                        logs[f"{metric}_r{r}/{event.name}/{name}"] = float(s[metric][j])
        return {f"{label}/{k}": v for k, v in logs.items()} if len(label) != 0 else logs
