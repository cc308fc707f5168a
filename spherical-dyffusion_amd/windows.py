"""What the aggregators and writers that read a window of `run_inference` in place share: the strided layout of one tensor,
the layouts of a window's variables (`WindowLayout`, the Python side of `sdy_window`, include/sdy_amd.h), the runs of
variables one launch takes, and `FieldAccumulator`, the float64 accumulators that stay on the device.

This module sits below `metrics`, `histogram`, `data_writer`, `spectrum`, `member_mean`, `rank_hist`, `events`, `fss`, `spells`,
`variability`, `eddies`, `time_bins`, `regions`, `field_scores`, `quantiles` and `spacetime` and imports none of them.
"""
from __future__ import annotations

import math
from itertools import accumulate
from typing import Callable, Dict, Iterator, List, NamedTuple, Optional, Sequence, Tuple

import torch

from ._lib import SDY_MAX_VARS, SdyWindow, ptr


class TorchDistributed:
    """`reduce_mean` / `reduce_sum` of the reference's `Distributed` singleton (`src/ace_inference/core/distributed.py:70-94`):
    `torch.distributed.all_reduce` over ranks (RCCL over xGMI on the GPU box; identity without a process group).  The reduce
    is issued on a side stream: it belongs to `get_logs`, not to the sampling path, and never blocks the compute stream."""

    def __init__(self):
        import torch.distributed as dist

        self._dist = dist if dist.is_available() and dist.is_initialized() else None
        self._stream = None

    @property
    def world_size(self) -> int:
        return self._dist.get_world_size() if self._dist is not None else 1

    def reduce_sum(self, tensor: torch.Tensor) -> torch.Tensor:
        return tensor if self._dist is None else self._reduce(tensor, self._dist.ReduceOp.SUM)

    def _reduce(self, tensor: torch.Tensor, op) -> torch.Tensor:
        if self._dist is None:
            return tensor
        if not tensor.is_cuda:
            out = tensor.clone()
            self._dist.all_reduce(out, op=op)
            return out
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=tensor.device)
        self._stream.wait_stream(torch.cuda.current_stream(tensor.device))
        with torch.cuda.stream(self._stream):
            out = tensor.clone()
            self._dist.all_reduce(out, op=op)
        torch.cuda.current_stream(tensor.device).wait_stream(self._stream)
        return out

    def reduce_mean(self, tensor: torch.Tensor) -> torch.Tensor:
        if self._dist is None:
            return tensor
        return self.reduce_sum(tensor) / self.world_size

    def reduce_min(self, tensor: torch.Tensor) -> torch.Tensor:
        """What the reference's `VideoAggregator` asks of its `dist` for the error extremes: all_reduce with MIN (`reduce_max`:
        MAX) on the side stream; identity without a process group."""
        return tensor if self._dist is None else self._reduce(tensor, self._dist.ReduceOp.MIN)

    def reduce_max(self, tensor: torch.Tensor) -> torch.Tensor:
        return tensor if self._dist is None else self._reduce(tensor, self._dist.ReduceOp.MAX)


def whole_ics_message(who: str) -> str:
    """What an ensemble aggregator says to a ragged share (flat rows: an initial condition's members cut by a rank boundary)."""
    return (f"{who} needs member-stacked (members, samples, time, lat, lon) "
            "predictions: ensemble-mean RMSE / CRPS / spread of an initial condition need all of its "
            "members on one rank (shard whole initial conditions, or use TimeMeanAggregator)")


def strided_layout(v: torch.Tensor) -> Tuple[torch.Tensor, int, int, int, int, int, int]:
    """-> (tensor to keep alive, n0, n1, s0, s1, T, HW): element (i0, i1, t, p) at data_ptr + i0*s0 + i1*s1 + t*HW + p.  Any
    leading axes in front of `(time, lat, lon)` are rows; more than two of them, a negative stride or a `(time, lat, lon)`
    block that is not contiguous are copied once.  No device check: the callers make their own."""
    if v.dim() < 3:
        raise ValueError(f"expected (..., time, lat, lon), got {tuple(v.shape)}")
    if v.dtype != torch.float32:
        v = v.to(torch.float32)
    T, H, W = v.shape[-3:]
    lead = tuple(v.shape[:-3])
    st = v.stride()
    inner = all(n == 1 or s == want for n, s, want in zip((T, H, W), st[-3:], (H * W, W, 1)))
    if not inner or len(lead) > 2 or any(s < 0 for s in st[:-3]):
        v = v.contiguous().view(-1, T, H, W)
        lead, st = (v.shape[0],), v.stride()
    if len(lead) == 2:
        return v, lead[0], lead[1], st[0], st[1], T, H * W
    if len(lead) == 1:
        return v, 1, lead[0], 0, st[0], T, H * W
    return v, 1, 1, 0, 0, T, H * W


class WindowLayout(NamedTuple):
    """One generated variable of a window and its target: gen element (i0, i1, t, p) at gen.data_ptr() + i0*gs0 + i1*gs1 +
    t*H*W + p, target element (i1, t, p) at target.data_ptr() + i1*ts1 + t*H*W + p (`sdy_window`)."""
    gen: torch.Tensor
    target: torch.Tensor
    n0: int
    n1: int
    gs0: int
    gs1: int
    ts1: int
    T: int
    H: int
    W: int

    @property
    def extents(self) -> tuple:
        """Everything but the two tensors: variables with equal extents share a launch."""
        return self[2:]


def window_layouts(target_data, gen_data) -> List[WindowLayout]:
    """Per generated variable the `WindowLayout` of one window, everything checked but the place of its times in a run;
    nothing is enqueued."""
    if len(gen_data) == 0:
        raise ValueError("No data in gen_data")
    out = []
    for name, g in gen_data.items():
        if name not in target_data:
            raise ValueError(f"no target for generated variable {name!r}")
        t = target_data[name]
        if g.dim() not in (4, 5) or t.dim() != 4:
            raise ValueError(f"{name!r}: generated data are (samples, time, lat, lon) or (members, samples, time, lat, lon)"
                             f" and targets (samples, time, lat, lon), got {tuple(g.shape)} and {tuple(t.shape)}")
        if tuple(g.shape[-4:]) != tuple(t.shape):
            raise ValueError(f"{name!r}: generated {tuple(g.shape)} against target {tuple(t.shape)}")
        H, W = g.shape[-2:]
        gv, n0, n1, gs0, gs1, T, _ = strided_layout(g)
        tv, _, tn1, _, ts1, _, _ = strided_layout(t)
        if min(n0, n1, T, H, W) < 1:
            raise ValueError("empty tensor")
        if (n0, n1) != (1 if g.dim() == 4 else g.shape[0], tn1):   # (a 5-D view that had to be copied came back flat)
            gv = gv.view(g.shape)
            n0, n1, gs0, gs1 = g.shape[0], g.shape[1], gv.stride(0), gv.stride(1)
        out.append(WindowLayout(gv, tv, n0, n1, gs0, gs1, ts1, T, H, W))
    T = out[0].T
    if any(l.T != T for l in out):
        raise ValueError("the variables of one window differ in their number of times")
    return out


def runs(items: Sequence, key: Callable, limit: int = SDY_MAX_VARS) -> Iterator[Tuple[int, int]]:
    """(first, last) of the runs of consecutive items that one launch takes: equal `key(item)`, at most `limit` of them."""
    first = 0
    while first < len(items):
        last, k = first + 1, key(items[first])
        while last < len(items) and last - first < limit and key(items[last]) == k:
            last += 1
        yield first, last
        first = last


def fill_window(win: SdyWindow, layouts: Sequence[WindowLayout], first: int, last: int) -> None:
    """Variables first .. last - 1 of a window (one run: equal extents) into the `sdy_window` of an argument structure."""
    win.nvars = last - first
    for j in range(first, last):
        win.gen[j - first], win.target[j - first] = ptr(layouts[j].gen), ptr(layouts[j].target)
    l = layouts[first]
    win.n0, win.n1, win.T, win.gs0, win.gs1, win.ts1 = l.n0, l.n1, l.T, l.gs0, l.gs1, l.ts1


def fill_slots(slots, t0: int, i_time_start: int, n_slots: int, pool_times: bool) -> None:
    """Where a window that starts at time `i_time_start` of a run lands, into the `sdy_lead_slots` of an argument structure;
    t0: its first counted time."""
    slots.t0, slots.t_start, slots.n_slots, slots.pool_times = t0, (0 if pool_times else i_time_start), n_slots, pool_times


def check_same_job(names: Sequence[str], jobs: Sequence[tuple], first_names: Sequence[str], first_jobs: Sequence[tuple],
                   what: str = "sample count") -> None:
    """A later window must hold the first window's variables, in its order, with its `jobs` (per variable what the aggregator
    fixes: `what` and the grid)."""
    if list(names) != list(first_names) or list(jobs) != list(first_jobs):
        raise ValueError(f"the variables, {what} or grids of a window differ from the first window's")


class FieldAccumulator:
    """What `VideoAggregator`, `ZonalMeanAggregator`, `PowerSpectrumAggregator`, `EnsembleTimeMeanAggregator`,
    `RankHistogramAggregator`, `EventVerificationAggregator`, `FractionsSkillAggregator`, `EventSpellAggregator`,
    `TimeVariabilityAggregator` and (the memory limit, the ranks and the same-job rule; its state is per group)
    `EddyCovarianceAggregator` share: the float64 accumulators (`self._acc[stat]`: one flat device buffer per statistic, the variables' blocks in dict order at
    `self._offsets[stat]`, so a run of same-shaped variables is one contiguous `(nvars, ...)` block: what one launch takes),
    the memory limit, the device check and the same-job check.  Everything is checked before anything changes: a refused
    window leaves the aggregator as it was.

    `n_timesteps`: the lead times of the accumulators' time axis, with the per-time batch counts (host integers) and
    `_record`, the whole of a `record_batch`; None for accumulators without a time axis."""

    #: what, besides the variables and the grids, a later window must repeat (the words of the refusal)
    _job_words = "sample count"
    #: the element type of every buffer of `_acc`, and what the refusal of the memory limit calls them
    _acc_dtype = torch.float64
    _acc_words = "float64 accumulators"

    def __init__(self, n_timesteps: Optional[int] = None, dist=None, metadata=None, max_bytes: Optional[int] = None):
        if n_timesteps is not None and n_timesteps < 1:
            raise ValueError(f"n_timesteps must be positive, got {n_timesteps}")
        self._n_timesteps = None if n_timesteps is None else int(n_timesteps)
        self._dist = TorchDistributed() if dist is None else dist
        self._metadata = {} if metadata is None else metadata
        self._max_bytes = max_bytes
        self._n_batches = [0] * (self._n_timesteps or 0)
        self._names: Optional[List[str]] = None
        self._grids: List[tuple] = []                  # per variable `_job` of the first window
        self._acc: Dict[str, torch.Tensor] = {}
        self._offsets: Dict[str, List[int]] = {}

    # -- to be provided: statistic name -> fill value; what a job is; the accumulator elements of one variable; the launch
    def _statistics(self) -> Dict[str, float]:
        raise NotImplementedError

    @staticmethod
    def _job(l: WindowLayout) -> tuple:
        """What a later window must repeat.  The member count is not part of it: a later window may change it."""
        return (l.n1, l.H, l.W)

    def _elements(self, stat: str, job: tuple) -> int:
        raise NotImplementedError

    def _size_words(self, names: List[str], jobs: List[tuple]) -> str:
        return f"{len(self._statistics())} statistics x {len(names)} variables x {self._n_timesteps} timesteps"

    def _launch(self, lay: List[WindowLayout], first: int, last: int, t_start: int) -> None:
        raise NotImplementedError

    def _prepare(self, names: List[str], lay: List[WindowLayout]) -> torch.device:
        """First batch: the memory limit, the device check, then the accumulators.  Later batches: the same job as the first.
        Then every tensor on the accumulators' device."""
        on_device = all(l.gen.is_cuda and l.target.is_cuda for l in lay)
        jobs = [self._job(l) for l in lay]
        if self._names is None:
            stats = self._statistics()
            sizes = {stat: [self._elements(stat, j) for j in jobs] for stat in stats}
            need = self._acc_dtype.itemsize * sum(sum(v) for v in sizes.values())
            device = lay[0].gen.device
            limit = self._max_bytes
            if limit is None and on_device:
                limit = torch.cuda.get_device_properties(device).total_memory // 4
            if limit is not None and need > limit:
                raise ValueError(f"{type(self).__name__}: {self._size_words(names, jobs)} need {need} bytes of "
                                 f"{self._acc_words}, more than max_bytes = {limit}")
        else:
            check_same_job(names, jobs, self._names, self._grids, self._job_words)
            device = next(iter(self._acc.values())).device
        if not on_device:
            raise RuntimeError("sdy_amd aggregators run on the GPU only (no CPU fallback)")
        for l in lay:
            if l.gen.device != device or l.target.device != device:
                raise ValueError(f"tensors on {l.gen.device} / {l.target.device}, accumulators on {device}")
        if self._names is None:
            self._acc = {k: torch.full((sum(sizes[k]),), fill, dtype=self._acc_dtype, device=device) for k, fill in stats.items()}
            self._offsets = {k: [0, *accumulate(v)][:-1] for k, v in sizes.items()}
            self._names, self._grids = list(names), jobs
        return device

    def _at(self, stat: str, i: int) -> int:
        """Device address of variable i's block of a statistic."""
        return self._acc[stat].data_ptr() + self._acc_dtype.itemsize * self._offsets[stat][i]

    def _view(self, stat: str, i: int, *shape) -> torch.Tensor:
        at = self._offsets[stat][i]
        return self._acc[stat][at:at + math.prod(shape)].view(*shape)

    def _record(self, target_data, gen_data, i_time_start: int) -> None:
        """One window into accumulators with a time axis: its times must lie inside the aggregator's."""
        i_time_start = int(i_time_start)
        lay = window_layouts(target_data, gen_data)
        T = lay[0].T
        if i_time_start < 0 or i_time_start + T > self._n_timesteps:
            raise ValueError(f"times {i_time_start}..{i_time_start + T - 1} outside the aggregator's {self._n_timesteps}")
        device = self._prepare(list(gen_data), lay)
        with torch.cuda.device(device):
            for first, last in runs(lay, lambda l: l.extents):
                self._launch(lay, first, last, i_time_start)
        for t in range(i_time_start, i_time_start + T):
            self._n_batches[t] += 1

    def _counts(self) -> torch.Tensor:
        if self._names is None:
            raise RuntimeError("No data recorded")
        return torch.tensor(self._n_batches, dtype=torch.float64, device=next(iter(self._acc.values())).device)

    def get_logs(self, label: str) -> Dict[str, object]:
        """{}: the wandb videos / images of the reference are out of scope, and the log key sets stay what they were."""
        return {}
