"""Value histograms of the inference loop on the device: host mirror of `DynamicHistogram`
(`src/ace_inference/core/histogram.py`) and of the data writer's `HistogramDataWriter`
(`src/ace_inference/inference/data_writer/histograms.py`, the sub-writer `DataWriter` always attaches,
`data_writer/main.py:65-134`).

Per variable and lead time: `n_bins` (300) constant-width bins over a range that doubles, to the left and then to the right,
until it holds every value seen; the counts of a doubled range are the pairwise sums of the old ones.  Edges are float32
`np.linspace(start, stop, n_bins + 1)` and a value is binned as `np.histogram(values, bins=edges)` bins it -- the counts are
the reference's integer for integer and the edges bit for bit (tests/golden/fx_histogram.npz).

What stays on the device: the range, the counts and the bookkeeping of every variable.  `add` / `append_batch` enqueue three
launches per dict (`sdy_hist_add`: min / max, range rules, counting -- all variables at once) and return; nothing waits for
the device before `counts`, `bin_edges`, `get_dataset` or `flush` read the result back.  Tensors are read in place: any
leading axes in front of `(time, lat, lon)` are pooled into the sample set, so the window driver's member-stacked
`(members, samples, time, lat, lon)` view needs no copy (more than two leading axes, or a `(time, lat, lon)` block that is not
contiguous, are copied once).

Deviations from the reference, all on purpose:
  * the reference attaches this writer for `n_ensemble_members == 1` only and its reshape expects 4-D data; here member-stacked
    predictions and the flat rows of ragged / relayed shares are accepted, and all trajectories pool into one histogram per
    lead time.  Each process keeps its own histograms; merging ranks whose ranges differ is out of scope (the reference does
    not do it either);
  * where the reference would loop forever or produce NaN edges (a non-finite value, a zero-width float32 range such as a
    constant field too large for +-1e-6 to change it) the variable's range flag is set on the device and reading the result
    raises `SdyError`;
  * `flush()` writes `histograms.npz` (keys `<source>/<name>`, `<source>/<name>_bin_edges`), not `histograms.nc`: netCDF output
    needs xarray / netCDF4, which this package does without.

GPU only: CPU tensors raise, like every module of this package.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import SDY_HIST_FLAG_RANGE, SDY_HIST_MAX_BINS, SdyError, SdyHistArgs, check, current_stream, lib, ptr
from .windows import runs, strided_layout


def bin_edges(start: float, stop: float, n_bins: int) -> np.ndarray:
    """The `n_bins + 1` float32 edges of a range, by the library's own arithmetic (the header the kernels compile)."""
    edges = np.empty(n_bins + 1, dtype=np.float32)
    check(lib.sdy_hist_edges_host(float(start), float(stop), int(n_bins), edges.ctypes.data_as(C.c_void_p)),
          "sdy_hist_edges_host")
    return edges


def _layout(v: torch.Tensor) -> Tuple[torch.Tensor, int, int, int, int, int, int]:
    """-> (tensor to keep alive, n0, n1, s0, s1, T, HW): element (i0, i1, t, p) at data_ptr + i0*s0 + i1*s1 + t*HW + p."""
    if not v.is_cuda:
        raise RuntimeError("sdy_amd histograms run on the GPU only (no CPU fallback)")
    return strided_layout(v)


class _HistogramSet:
    """State and counts of several variables' histograms on one device, fed one dict at a time."""

    def __init__(self, names: Sequence[str], n_times: int, n_bins: int, device):
        if n_bins % 2 or not 2 <= n_bins <= SDY_HIST_MAX_BINS:
            raise ValueError(f"n_bins must be even and within 2..{SDY_HIST_MAX_BINS}, got {n_bins}")
        if n_times < 1:
            raise ValueError(f"n_times must be positive, got {n_times}")
        self.names, self.n_times, self.n_bins = list(names), int(n_times), int(n_bins)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("sdy_amd histograms run on the GPU only (no CPU fallback)")
        self._state_bytes = int(lib.sdy_hist_state_bytes(1))
        self.state = torch.zeros(len(self.names), self._state_bytes, dtype=torch.uint8, device=self.device)
        self.counts = torch.zeros(len(self.names), self.n_times, self.n_bins, dtype=torch.int64, device=self.device)

    def add(self, tensors: Sequence[torch.Tensor], i_time_start: int) -> None:
        """`tensors[i]` feeds variable i.  Consecutive variables of one shape share a call (at most SDY_MAX_VARS each)."""
        assert len(tensors) == len(self.names)
        lay = [_layout(v) for v in tensors]
        for v, *_ in lay:
            if v.device != self.device:
                raise ValueError(f"tensor on {v.device}, histogram on {self.device}")
        i_time_start = int(i_time_start)
        for _, n0, n1, _, _, T, HW in lay:      # every call is checked before the first one is enqueued
            if i_time_start < 0 or i_time_start + T > self.n_times:
                raise ValueError(f"times {i_time_start}..{i_time_start + T - 1} outside the histogram's {self.n_times}")
            if min(n0, n1, T, HW) < 1:
                raise ValueError("empty tensor")
        for first, last in runs(lay, lambda l: l[1:3] + l[5:]):
            a = SdyHistArgs()
            a.nvars = last - first
            for j in range(first, last):
                v, _, _, s0, s1, _, _ = lay[j]
                a.data[j - first], a.s0[j - first], a.s1[j - first] = ptr(v), s0, s1
            _, a.n0, a.n1, _, _, a.T, a.HW = lay[first]
            a.t_start, a.n_times, a.n_bins = i_time_start, self.n_times, self.n_bins
            a.state, a.counts = ptr(self.state[first]), ptr(self.counts[first])
            with torch.cuda.device(self.device):
                check(lib.sdy_hist_add(C.byref(a), current_stream()), "sdy_hist_add")

    def read(self) -> Tuple[np.ndarray, List[Optional[np.ndarray]]]:
        """Synchronises and reads back: counts int64 (variables, n_times, n_bins) and per variable the edges (None: nothing
        added yet).  Raises SdyError for a variable whose range flag is set or that saw a value outside its range."""
        torch.cuda.synchronize(self.device)
        counts = self.counts.cpu().numpy()
        state = np.ascontiguousarray(self.state.cpu().numpy())
        edges: List[Optional[np.ndarray]] = []
        for i, name in enumerate(self.names):
            start, stop, init, flags, outside = C.c_float(), C.c_float(), C.c_int(), C.c_uint(), C.c_ulonglong()
            check(lib.sdy_hist_state_unpack_host(state.ctypes.data_as(C.c_void_p), i, C.byref(start), C.byref(stop),
                                                 C.byref(init), C.byref(flags), C.byref(outside)), "sdy_hist_state_unpack_host")
            if flags.value & SDY_HIST_FLAG_RANGE:
                raise SdyError(f"histogram of {name!r}: a window held non-finite values or a range float32 cannot divide into "
                               f"{self.n_bins} bins (flags {flags.value}, {outside.value} values not counted)")
            if flags.value or outside.value:
                raise SdyError(f"histogram of {name!r}: flags {flags.value}, {outside.value} values outside the range")
            edges.append(bin_edges(start.value, stop.value, self.n_bins) if init.value else None)
        return counts, edges


class DynamicHistogram:
    """`core/histogram.py::DynamicHistogram` on the device: `add(value, i_time_start)`, `.counts`, `.bin_edges`."""

    def __init__(self, n_times: int, n_bins: int = 300, device=None):
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._set = _HistogramSet(["value"], n_times, n_bins, dev)
        self._n_times, self._n_bins = int(n_times), int(n_bins)

    def add(self, value: torch.Tensor, i_time_start: int = 0) -> None:
        """`value`: device tensor (..., time, lat, lon); every leading axis is pooled into the samples of its lead time
        (the reference takes the same numbers as a host array (time, samples))."""
        self._set.add([value], i_time_start)

    @property
    def counts(self) -> np.ndarray:
        return self._set.read()[0][0]

    @property
    def bin_edges(self) -> Optional[np.ndarray]:
        return self._set.read()[1][0]


class HistogramDataWriter:
    """`data_writer/histograms.py::HistogramDataWriter` for `run_inference(writer=...)`: [time, bin] histograms of every
    variable of the targets and of the predictions.  One `sdy_hist_add` per source and `append_batch`; nothing synchronises
    before `get_dataset` / `flush`.  `flush()` writes `<path>/histograms.npz` (no netCDF: see the module docstring); with
    `path=None` it writes nothing."""

    SOURCES = ("target", "prediction")

    def __init__(self, path: Optional[str], n_timesteps: int, metadata: Optional[Mapping[str, object]] = None, n_bins: int = 300):
        if n_bins % 2 or not 2 <= n_bins <= SDY_HIST_MAX_BINS:
            raise ValueError(f"n_bins must be even and within 2..{SDY_HIST_MAX_BINS}, got {n_bins}")
        self.path = path
        self._filename = None if path is None else os.path.join(str(path), "histograms.npz")
        self.metadata = dict(metadata) if metadata else {}
        self._n_times, self._n_bins = int(n_timesteps), int(n_bins)
        self._sets: Dict[str, _HistogramSet] = {}

    def append_batch(self, target: Mapping[str, torch.Tensor], prediction: Mapping[str, torch.Tensor], start_timestep: int,
                     start_sample: int = 0, batch_times=None) -> None:
        del start_sample, batch_times
        for source, data in zip(self.SOURCES, (target, prediction)):
            if source not in self._sets:      # the variables of the first batch, as in the reference
                if not data:
                    continue
                dev = next(iter(data.values())).device
                if dev.type != "cuda":
                    raise RuntimeError("sdy_amd histograms run on the GPU only (no CPU fallback)")
                self._sets[source] = _HistogramSet(list(data), self._n_times, self._n_bins, dev)
            hs = self._sets[source]
            hs.add([data[n] for n in hs.names], start_timestep)

    def get_dataset(self) -> Dict[str, Dict[str, np.ndarray]]:
        """{"target": {...}, "prediction": {...}}, each with `<name>` (int64 counts (n_times, n_bins)) and
        `<name>_bin_edges` (float32 (n_bins + 1,)); a name only one source has gets zero counts and the other's edges
        (`histograms.py:52-69`)."""
        if len(self._sets) < 2:
            raise RuntimeError("No data has been recorded.")
        out: Dict[str, Dict[str, np.ndarray]] = {}
        for source in self.SOURCES:
            counts, edges = self._sets[source].read()
            out[source] = {}
            for i, name in enumerate(self._sets[source].names):
                out[source][name] = counts[i]
                out[source][f"{name}_bin_edges"] = edges[i]
        for a, b in (self.SOURCES, self.SOURCES[::-1]):
            for name in [n for n in out[b] if n not in out[a] and not n.endswith("_bin_edges")]:
                out[a][name] = np.zeros_like(out[b][name])
                out[a][f"{name}_bin_edges"] = out[b][f"{name}_bin_edges"]
        return out

    def flush(self) -> None:
        if self._filename is None:
            return
        flat = {f"{source}/{key}": value for source, d in self.get_dataset().items() for key, value in d.items()}
        for name, meta in self.metadata.items():
            units = getattr(meta, "units", None)
            if units is not None:
                flat[f"units/{name}"] = np.asarray(str(units))
        os.makedirs(os.path.dirname(self._filename), exist_ok=True)
        np.savez(self._filename, **flat)
