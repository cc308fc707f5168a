"""Transient-eddy covariances of groups of variables at every grid point of a rollout, on the device: how two variables move
together in time -- the momentum flux u'v', the poleward heat flux v'T', the moisture flux v'q', the eddy kinetic energy
(u'u' + v'v') / 2 and the correlation of any two variables at a point.  A member can have the right mean, the right variance of
v and of T and the right spectra and still transport no heat poleward; these are the statistics that show it.  The reference has
nothing of the kind; the definition is `csrc/time_covariance.h`.
"""
from __future__ import annotations

import ctypes as C
import math
import re
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import torch

from ._lib import (SDY_MAX_VARS, SDY_TC_MAX_GROUPS, SDY_TC_MAX_K, SDY_TC_SLOTS, SdyTimeCovarianceArgs,
                   SdyTimeCovarianceMapsArgs, SdyTimeCovarianceStatsArgs, check, current_stream, lib, ptr)
from .windows import FieldAccumulator, WindowLayout, fill_window, whole_ics_message, window_layouts


def n_pairs(K: int) -> int:
    return K * (K + 1) // 2


def pair_index(K: int, i: int, j: int) -> int:
    """The place of (i, j), i <= j, in the pair order (0,0), (0,1), .., (0,K-1), (1,1), .. of `csrc/time_covariance.h`."""
    return i * K - i * (i - 1) // 2 + (j - i)


class CovarianceGroups:
    """The groups of an `EddyCovarianceAggregator`: per label an ordered mapping from a short name to a variable, 2 to 4
    entries, e.g. `add("level_3", {"u": "eastward_wind_3", "v": "northward_wind_3", "T": "air_temperature_3"})`.  Every pair
    of a group's variables gets its covariance and correlation; a variable that takes part in several pairs is read once."""

    STANDARD = (("u", "eastward_wind"), ("v", "northward_wind"), ("T", "air_temperature"), ("q", "specific_total_water"))

    def __init__(self):
        self._groups: Dict[str, Dict[str, str]] = {}

    def add(self, label: str, variables: Mapping[str, str]) -> "CovarianceGroups":
        label = str(label)
        if label in self._groups:
            raise ValueError(f"group {label!r} twice")
        if len(label) == 0 or "/" in label:
            raise ValueError(f"a group label is a non-empty string without '/', got {label!r}")
        pairs = [(str(a), str(v)) for a, v in (variables.items() if isinstance(variables, Mapping) else variables)]
        shorts, names = [a for a, _ in pairs], [v for _, v in pairs]
        if not 2 <= len(pairs) <= SDY_TC_MAX_K:
            raise ValueError(f"group {label!r}: 2 to {SDY_TC_MAX_K} variables, got {len(pairs)}")
        if len(set(shorts)) != len(shorts) or len(set(names)) != len(names):
            raise ValueError(f"group {label!r}: a short name or a variable twice: {pairs}")
        if any(len(a) == 0 or "/" in a or "_" in a for a in shorts):
            raise ValueError(f"group {label!r}: a short name is a non-empty string without '/' and '_', got {shorts}")
        self._groups[label] = dict(pairs)
        return self

    @classmethod
    def standard(cls, names: Sequence[str]) -> "CovarianceGroups":
        """`level_<k>` for every level k whose `eastward_wind_<k>` and `northward_wind_<k>` are both among `names`, in
        ascending k, with `air_temperature_<k>` and `specific_total_water_<k>` where present: shorts u, v, T, q."""
        have = set(names)
        levels = sorted(int(m[1]) for n in have if (m := re.fullmatch(r"eastward_wind_(\d+)", n)) and f"northward_wind_{m[1]}" in have)
        out = cls()
        for k in levels:
            out.add(f"level_{k}", {a: f"{stem}_{k}" for a, stem in cls.STANDARD if f"{stem}_{k}" in have})
        return out

    def __len__(self) -> int:
        return len(self._groups)

    def __iter__(self):
        return iter(self._groups.items())

    @property
    def labels(self) -> List[str]:
        return list(self._groups)

    def variables(self, label: str) -> Dict[str, str]:
        return dict(self._groups[label])


class _Block:
    """The groups of one K: their state `(n_groups, K | NP, rows, H W)` in one buffer each, what one launch takes."""

    def __init__(self, K: int, labels: List[str]):
        self.K, self.labels = K, labels
        self.sums = self.products = self.origins = None


class EddyCovarianceAggregator(FieldAccumulator):
    """Per member and for the target: the covariance and the correlation along time of every pair of variables of every group,
    at every grid point, and area-weighted summaries of them.

    `record_batch(loss, target_data, gen_data, target_data_norm, gen_data_norm, i_time_start)` is what `run_inference` calls
    once per window: targets `(samples, time, lat, lon)`, gen `(members, samples, time, lat, lon)` (a 4-D gen is one
    member).  One `sdy_time_covariance_accumulate` launch per K present (groups of 2, 3 and 4 variables) reads the window in
    place -- the member-stacked transposed view included -- and advances the state of every group, trajectory and grid point:
    with the counted times `x_k,1 .. x_k,n` and the origins `c_k = x_k,1`, the float64 sums of `d_k,t = x_k,t - c_k` and of
    `d_i,t d_j,t` for `i <= j`, and the fp32 origins: K + K (K + 1) / 2 doubles and K floats, 128 bytes at K = 4 (25 members and
    the target on 180 x 360: 216 MB per group of four).  The shift by the first value keeps the covariance of fields with
    large means to float64 rounding of the deviations.  The state carries the run across window boundaries and its bits do
    not depend on how the run is cut into windows.  The first time of a run (`i_time_start == 0`) is the initial condition
    and is not counted; a window that holds nothing else counts nothing.  The first window that is accepted may start anywhere
    and fixes variables, grid, member count and sample count; every later one must repeat them and start where the one before
    ended (`ValueError` otherwise).  A variable of a group that the window lacks, and a group whose variables differ in their
    grid, are refused.  The state is allocated on the first window, after comparing its bytes with `max_bytes` (default: a
    quarter of the device's memory).  A refused window changes nothing.  Variables of one launch whose strides differ are
    copied once.

    `get_pair_data(label, a, b)` returns float64 device tensors of one pair of shorts of one group: `gen_cov`, `gen_corr`
    `(members, samples, lat, lon)`, `target_cov`, `target_corr` `(samples, lat, lon)` (`sdy_time_covariance_maps`: population
    covariance; correlation clamped to [-1, 1], NaN where a variance is 0), and `gen_cov_zonal`, `target_cov_zonal` `(samples,
    lat)`, the member mean and the longitude mean of the covariance: the `[v'T'](lat)` profile.  `get_means(label)` returns the
    time means `c_k + S_k / n` per short, `{"gen": .., "target": ..}`: what a stationary-eddy decomposition starts from.

    `get_logs(label)` returns Python floats.  Per group and off-diagonal pair `<a>_<b>`: `cov_gen/<group>/<a>_<b>`,
    `cov_target/..` (area-weighted means of the member-mean and of the target covariance), `cov_bias/..`, `cov_rmse/..` (root of
    the weighted mean of (member-mean cov - target cov)^2), `corr_gen/..`, `corr_target/..` (weighted means over the points
    where the target and every member have a correlation), `corr_bias/..` and `corr_defined_fraction/..` (those points' share
    of the weight).  Per group and variable: `time_variance_gen/<group>/<a>`, `time_variance_target/<group>/<a>`.  For a group
    with shorts `u` and `v`: `eke_gen/<group>`, `eke_target/<group>` (half the sum of the two variances) and
    `eke_ratio/<group>`.  One `sdy_time_covariance_stats` call per K; sums run over samples and grid points in float64.  Fewer
    than two counted times: `ValueError`.

    Ranks hold whole initial conditions: the raw weighted sums and `samples * sum(weights)` are added over ranks
    (`dist.reduce_sum`) in one reduce before any root or division.  Ragged shares (flat rows with `sample_weights`) are
    refused.  Lagged covariances, band-pass filters, vertical integrals, plots and masks are out of scope."""

    accepts_sample_weights = True      # (to see, and refuse, a ragged share)

    _job_words = "member count, sample count"

    PAIR_KEYS = ("cov_gen", "cov_target", "cov_bias", "cov_rmse", "corr_gen", "corr_target", "corr_bias",
                 "corr_defined_fraction")
    VARIABLE_KEYS = ("time_variance_gen", "time_variance_target")
    EKE_KEYS = ("eke_gen", "eke_target", "eke_ratio")

    def __init__(self, groups: CovarianceGroups, area_weights: torch.Tensor, dist=None, target: str = "denorm", metadata=None,
                 max_bytes: Optional[int] = None):
        if target not in ("norm", "denorm"):
            raise ValueError(f"target must be 'norm' or 'denorm', got {target!r}")
        if not isinstance(groups, CovarianceGroups) or len(groups) == 0:
            raise ValueError("groups: a sdy_amd.CovarianceGroups with at least one group")
        super().__init__(dist=dist, metadata=metadata, max_bytes=max_bytes)      # (no time axis)
        self._groups = {label: dict(v) for label, v in groups}
        self._area_weights = area_weights
        self._target = target
        self._n_times = 0                          # counted times so far
        self._next_start: Optional[int] = None     # where the next window has to start (None before the first window)
        self._job_fixed: Optional[tuple] = None    # (members, samples, lat, lon) of the first window
        # one block per K present, in ascending K; a group's place: (block, index within it)
        self._blocks = [_Block(K, [l for l, v in self._groups.items() if len(v) == K])
                        for K in sorted({len(v) for v in self._groups.values()})]
        self._place = {l: (b, i) for b in self._blocks for i, l in enumerate(b.labels)}

    @property
    def n_times(self) -> int:
        """Counted times so far."""
        return self._n_times

    @property
    def groups(self) -> Dict[str, Dict[str, str]]:
        return {l: dict(v) for l, v in self._groups.items()}

    def state_bytes(self, M: int, n1: int, H: int, W: int) -> int:
        """Bytes of the state of all groups for M members and n1 samples on an H x W grid."""
        return sum((8 * (K + n_pairs(K)) + 4 * K) * (M + 1) * n1 * H * W for K in (len(v) for v in self._groups.values()))

    # -- one window -------------------------------------------------------------------------------------------------------------
    def _check_window(self, target_data, gen_data, start: int) -> Tuple[List[str], Dict[str, WindowLayout], tuple]:
        """Everything that can refuse a window, before anything changes -> (window names, layouts of the groups' variables, job)."""
        needed = [v for g in self._groups.values() for v in g.values()]
        for v in needed:
            if v not in gen_data or v not in target_data:
                raise ValueError(f"EddyCovarianceAggregator: variable {v!r} of a group is missing from the window")
        unique = list(dict.fromkeys(needed))
        lay = dict(zip(unique, window_layouts(target_data, {v: gen_data[v] for v in unique})))
        for label, g in self._groups.items():
            grids = {(lay[v].H, lay[v].W) for v in g.values()}
            if len(grids) != 1:
                raise ValueError(f"EddyCovarianceAggregator: the variables of group {label!r} differ in their grid: {sorted(grids)}")
        jobs = {(l.n0, l.n1, l.H, l.W) for l in lay.values()}
        if len(jobs) != 1:
            raise ValueError(f"EddyCovarianceAggregator: the groups' variables differ in member count, sample count or grid: {sorted(jobs)}")
        job = next(iter(jobs))
        names = list(gen_data)
        if self._names is not None and (names != self._names or job != self._job_fixed):
            raise ValueError(f"the variables, {self._job_words} or grids of a window differ from the first window's")
        if self._next_start is not None and start != self._next_start:
            raise ValueError(f"EddyCovarianceAggregator: a window that starts at time {start}, where the one before ended at "
                             f"{self._next_start}: the state needs every window of a run, in order")
        return names, lay, job

    def _allocate(self, names: List[str], lay: Dict[str, WindowLayout], job: tuple) -> torch.device:
        on_device = all(l.gen.is_cuda and l.target.is_cuda for l in lay.values())
        first = next(iter(lay.values()))
        device = first.gen.device if self._names is None else self._blocks[0].sums.device
        if self._names is None:
            need = self.state_bytes(*job)
            limit = self._max_bytes
            if limit is None and on_device:
                limit = torch.cuda.get_device_properties(device).total_memory // 4
            if limit is not None and need > limit:
                raise ValueError(f"EddyCovarianceAggregator: {len(self._groups)} groups of {job[0]} members need {need} bytes of "
                                 f"state, more than max_bytes = {limit}")
        if not on_device:
            raise RuntimeError("sdy_amd aggregators run on the GPU only (no CPU fallback)")
        for l in lay.values():
            if l.gen.device != device or l.target.device != device:
                raise ValueError(f"tensors on {l.gen.device} / {l.target.device}, state on {device}")
        if self._names is None:
            M, n1, H, W = job
            n = (M + 1) * n1 * H * W
            for b in self._blocks:
                G, K = len(b.labels), b.K
                b.sums = torch.zeros(G * K * n, dtype=torch.float64, device=device)
                b.products = torch.zeros(G * n_pairs(K) * n, dtype=torch.float64, device=device)
                b.origins = torch.zeros(G * K * n, dtype=torch.float32, device=device)
            self._names, self._job_fixed = names, job
            self._grids = [job] * len(self._groups)
            self._acc = {"sums": self._blocks[0].sums}      # (what FieldAccumulator's helpers look at)
        return device

    @staticmethod
    def _launches(b: _Block, groups: Dict[str, Dict[str, str]]):
        """(first, last) group of every launch of a block: at most SDY_TC_MAX_GROUPS groups and SDY_MAX_VARS unique variables."""
        first, seen = 0, set()
        for i, label in enumerate(b.labels):
            more = seen | set(groups[label].values())
            if i - first == SDY_TC_MAX_GROUPS or len(more) > SDY_MAX_VARS:
                yield first, i
                first, more = i, set(groups[label].values())
            seen = more
        yield first, len(b.labels)

    @torch.no_grad()
    def record_batch(self, loss, target_data, gen_data, target_data_norm=None, gen_data_norm=None, i_time_start: int = 0,
                     sample_weights: Optional[Sequence[float]] = None):
        del loss
        if self._target == "norm":
            target_data, gen_data = target_data_norm, gen_data_norm
        ragged = sample_weights is not None or any(
            g.dim() == 4 and k in target_data and target_data[k].dim() == 4 and g.shape[0] != target_data[k].shape[0]
            for k, g in gen_data.items())
        if ragged:
            raise ValueError(whole_ics_message("EddyCovarianceAggregator"))
        start = int(i_time_start)
        if start < 0:
            raise ValueError(f"i_time_start must not be negative, got {start}")
        names, lay, job = self._check_window(target_data, gen_data, start)
        device = self._allocate(names, lay, job)
        T = next(iter(lay.values())).T
        t0 = 1 if start == 0 else 0                   # the very first time of a run is the initial condition
        if T - t0 >= 1:
            with torch.cuda.device(device):
                for a, _ in self._calls(lay, t0):
                    check(lib.sdy_time_covariance_accumulate(C.byref(a), current_stream()), "sdy_time_covariance_accumulate")
            self._n_times += T - t0
        self._next_start = start + T

    def _calls(self, lay: Dict[str, WindowLayout], t0: int):
        """The argument structures of one window's launches, one per K present (more where a block has more groups or unique
        variables than one launch takes), each with the tensors it points into."""
        M, n1, H, W = self._job_fixed
        n = (M + 1) * n1 * H * W
        for b in self._blocks:
            K, NP = b.K, n_pairs(b.K)
            for first, last in self._launches(b, self._groups):
                unique = list(dict.fromkeys(v for l in b.labels[first:last] for v in self._groups[l].values()))
                ls = [lay[v] for v in unique]
                if any(l.extents != ls[0].extents for l in ls):          # one sdy_window has one set of strides
                    ls = [l._replace(gen=l.gen.contiguous(), target=l.target.contiguous()) for l in ls]
                    ls = [l._replace(gs0=l.gen.stride(0) if l.gen.dim() == 5 else 0, gs1=l.gen.stride(-4),
                                     ts1=l.target.stride(0)) for l in ls]
                a = SdyTimeCovarianceArgs()
                fill_window(a.win, ls, 0, len(ls))
                a.HW, a.t0, a.first = H * W, t0, int(self._n_times == 0)
                a.K, a.n_groups = K, last - first
                for g, label in enumerate(b.labels[first:last]):
                    for k, v in enumerate(self._groups[label].values()):
                        a.members[g][k] = unique.index(v)
                a.sums = b.sums.data_ptr() + 8 * first * K * n
                a.products = b.products.data_ptr() + 8 * first * NP * n
                a.origins = b.origins.data_ptr() + 4 * first * K * n
                yield a, ls

    # -- read-out ---------------------------------------------------------------------------------------------------------------
    def _check_recorded(self) -> None:
        # (raised BEFORE any collective: every rank of a job must have recorded at least two counted times)
        if self._names is None or self._n_times < 2:
            raise ValueError(f"No data recorded: covariances and correlations need two counted times, got {self._n_times}.")

    def _index(self, label: str, short: str) -> int:
        shorts = list(self._groups[label])
        if short not in shorts:
            raise KeyError(f"group {label!r} has {shorts}, not {short!r}")
        return shorts.index(short)

    @torch.no_grad()
    def get_pair_data(self, label: str, a: str, b: str) -> Dict[str, torch.Tensor]:
        """Covariance and correlation maps of the shorts `a` and `b` of group `label` (`a == b`: the variance): this rank's maps
        so far, float64 on the device."""
        self._check_recorded()
        blk, g = self._place[label]
        i, j = sorted((self._index(label, a), self._index(label, b)))
        M, n1, H, W = self._job_fixed
        n, K, NP = (M + 1) * n1 * H * W, blk.K, n_pairs(blk.K)
        cov = torch.empty(n, dtype=torch.float64, device=blk.sums.device)
        corr = torch.empty_like(cov)
        with torch.cuda.device(cov.device):
            m = SdyTimeCovarianceMapsArgs()
            m.sums, m.products = blk.sums.data_ptr() + 8 * g * K * n, blk.products.data_ptr() + 8 * g * NP * n
            m.K, m.i, m.j, m.n_elems, m.n_times = K, i, j, n, float(self._n_times)
            m.cov, m.corr = ptr(cov), ptr(corr)
            check(lib.sdy_time_covariance_maps(C.byref(m), current_stream()), "sdy_time_covariance_maps")
        ng = M * n1 * H * W
        out = {"gen_cov": cov[:ng].view(M, n1, H, W), "gen_corr": corr[:ng].view(M, n1, H, W),
               "target_cov": cov[ng:].view(n1, H, W), "target_corr": corr[ng:].view(n1, H, W)}
        out["gen_cov_zonal"] = out["gen_cov"].mean(dim=0).mean(dim=-1)
        out["target_cov_zonal"] = out["target_cov"].mean(dim=-1)
        return out

    @torch.no_grad()
    def get_means(self, label: str) -> Dict[str, Dict[str, torch.Tensor]]:
        """{"gen": {short: (members, samples, lat, lon)}, "target": {short: (samples, lat, lon)}}: the time means of the counted
        times, `c_k + S_k / n`, float64 on the device."""
        self._check_recorded()
        blk, g = self._place[label]
        M, n1, H, W = self._job_fixed
        n, ng, K = (M + 1) * n1 * H * W, M * n1 * H * W, blk.K
        out: Dict[str, Dict[str, torch.Tensor]] = {"gen": {}, "target": {}}
        for k, short in enumerate(self._groups[label]):
            at = (g * K + k) * n
            mean = blk.origins[at:at + n].double() + blk.sums[at:at + n] / float(self._n_times)
            out["gen"][short], out["target"][short] = mean[:ng].view(M, n1, H, W), mean[ng:].view(n1, H, W)
        return out

    @torch.no_grad()
    def weighted_sums(self) -> Dict[str, torch.Tensor]:
        """Per group the raw weighted sums of `sdy_time_covariance_stats` (this rank's), `(pairs, 6)` in the pair order (0,0),
        (0,1), .., float64 on the device."""
        self._check_recorded()
        M, n1, H, W = self._job_fixed
        if tuple(self._area_weights.shape) != (H, W):
            raise ValueError(f"area weights {tuple(self._area_weights.shape)} against a {(H, W)} grid")
        device = self._blocks[0].sums.device
        w = self._area_weights.to(device, torch.float32).contiguous()
        n = (M + 1) * n1 * H * W
        out = {}
        with torch.cuda.device(device):
            for b in self._blocks:
                K, NP = b.K, n_pairs(b.K)
                for first in range(0, len(b.labels), SDY_TC_MAX_GROUPS):
                    G = min(SDY_TC_MAX_GROUPS, len(b.labels) - first)
                    res = torch.empty(G, NP, SDY_TC_SLOTS, dtype=torch.float64, device=device)
                    ws_bytes = lib.sdy_time_covariance_workspace_bytes(K, G, n1, H * W)
                    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=device)
                    a = SdyTimeCovarianceStatsArgs()
                    a.K, a.n_groups, a.M, a.n1, a.HW = K, G, M, n1, H * W
                    a.sums = b.sums.data_ptr() + 8 * first * K * n
                    a.products = b.products.data_ptr() + 8 * first * NP * n
                    a.weights, a.n_times, a.out = ptr(w), float(self._n_times), ptr(res)
                    a.ws, a.ws_bytes = ptr(ws), ws_bytes
                    check(lib.sdy_time_covariance_stats(C.byref(a), current_stream()), "sdy_time_covariance_stats")
                    for g in range(G):
                        out[b.labels[first + g]] = res[g]
        return {label: out[label] for label in self._groups}

    @classmethod
    def logs_from_sums(cls, group: str, shorts: Sequence[str], s: Sequence[Sequence[float]], den: float) -> Dict[str, float]:
        """One group's logs from its raw sums `(pairs, 6)` and the total weight `samples * sum(weights)` (both already added
        over ranks): the pairs' keys in pair order, then the variables', then the eddy kinetic energy's."""
        nan = float("nan")
        K = len(shorts)
        logs: Dict[str, float] = {}
        for i in range(K):
            for j in range(i + 1, K):
                q, name = s[pair_index(K, i, j)], f"{group}/{shorts[i]}_{shorts[j]}"
                cov_gen, cov_target = q[0] / den, q[1] / den
                corr_gen, corr_target = (q[3] / q[5], q[4] / q[5]) if q[5] > 0.0 else (nan, nan)
                vals = (cov_gen, cov_target, cov_gen - cov_target, math.sqrt(q[2] / den), corr_gen, corr_target,
                        corr_gen - corr_target, q[5] / den)
                logs.update({f"{key}/{name}": float(v) for key, v in zip(cls.PAIR_KEYS, vals)})
        for i in range(K):
            q = s[pair_index(K, i, i)]
            logs[f"time_variance_gen/{group}/{shorts[i]}"] = float(q[0] / den)
            logs[f"time_variance_target/{group}/{shorts[i]}"] = float(q[1] / den)
        if "u" in shorts and "v" in shorts:
            qu, qv = (s[pair_index(K, i, i)] for i in (list(shorts).index("u"), list(shorts).index("v")))
            gen, target = 0.5 * (qu[0] + qv[0]) / den, 0.5 * (qu[1] + qv[1]) / den
            logs[f"eke_gen/{group}"], logs[f"eke_target/{group}"] = float(gen), float(target)
            logs[f"eke_ratio/{group}"] = float(gen / target) if target > 0.0 else nan
        return logs

    @torch.no_grad()
    def get_logs(self, label: str) -> Dict[str, float]:
        sums = self.weighted_sums()
        device = self._blocks[0].sums.device
        wsum = self._area_weights.to(device, torch.float32).double().sum()
        # ranks hold whole initial conditions: every group's sums and the sample count x sum(w) are added over ranks in ONE
        # reduce, before any root or division, and come to the host in one copy
        parts = [sums[g].reshape(-1) for g in self._groups] + [(self._job_fixed[1] * wsum).reshape(1)]
        packed = self._dist.reduce_sum(torch.cat(parts)).cpu().tolist()
        den, at = packed[-1], 0
        logs: Dict[str, float] = {}
        for group, variables in self._groups.items():
            NP = n_pairs(len(variables))
            s = [packed[at + q * SDY_TC_SLOTS:at + (q + 1) * SDY_TC_SLOTS] for q in range(NP)]
            at += NP * SDY_TC_SLOTS
            logs.update(self.logs_from_sums(group, list(variables), s, den))
        return {f"{label}/{k}": v for k, v in logs.items()} if len(label) != 0 else logs


@torch.no_grad()
def time_covariance(x: torch.Tensor, y: torch.Tensor) -> Dict[str, torch.Tensor]:
    """Covariance and correlation along time of two `(time, lat, lon)` fields on the device, every time counted ->
    {"cov", "corr", "mean_x", "mean_y"}: `(lat, lon)` float64; the arithmetic of `EddyCovarianceAggregator` (population
    covariance, shifted by the first time)."""
    if x.dim() != 3 or x.shape != y.shape or x.shape[0] < 1:
        raise ValueError(f"expected two (time, lat, lon) fields of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    if not (x.is_cuda and y.is_cuda):
        raise RuntimeError("sdy_amd aggregators run on the GPU only (no CPU fallback)")
    if y.device != x.device:
        raise ValueError(f"fields on {x.device} and {y.device}")
    T, H, W = x.shape
    fields = [v.to(torch.float32).contiguous() for v in (x, y)]
    n = 2 * H * W                                      # one generated row and one target row, the same data
    sums = torch.zeros(2 * n, dtype=torch.float64, device=x.device)
    products = torch.zeros(3 * n, dtype=torch.float64, device=x.device)
    origins = torch.zeros(2 * n, dtype=torch.float32, device=x.device)
    cov, corr = torch.empty(n, dtype=torch.float64, device=x.device), torch.empty(n, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        a = SdyTimeCovarianceArgs()
        a.win.nvars = 2
        for k, v in enumerate(fields):
            a.win.gen[k] = a.win.target[k] = ptr(v)
        a.win.n0, a.win.n1, a.win.T, a.win.gs0, a.win.gs1, a.win.ts1 = 1, 1, T, 0, 0, 0
        a.HW, a.t0, a.first, a.K, a.n_groups = H * W, 0, 1, 2, 1
        a.members[0][0], a.members[0][1] = 0, 1
        a.sums, a.products, a.origins = ptr(sums), ptr(products), ptr(origins)
        check(lib.sdy_time_covariance_accumulate(C.byref(a), current_stream()), "sdy_time_covariance_accumulate")
        m = SdyTimeCovarianceMapsArgs()
        m.sums, m.products, m.K, m.i, m.j, m.n_elems, m.n_times = ptr(sums), ptr(products), 2, 0, 1, n, float(T)
        m.cov, m.corr = ptr(cov), ptr(corr)
        check(lib.sdy_time_covariance_maps(C.byref(m), current_stream()), "sdy_time_covariance_maps")
    hw = H * W
    mean = lambda k: (origins[k * n:k * n + hw].double() + sums[k * n:k * n + hw] / float(T)).view(H, W)  # noqa: E731
    return {"cov": cov[:hw].view(H, W), "corr": corr[:hw].view(H, W), "mean_x": mean(0), "mean_y": mean(1)}
